// Generated-speaker metrics: set-to-set statistics in speaker-encoder space.
//
//   fs2_cosine_nn       the k nearest rows of b for every row of a by cosine distance, never
//                       storing the Na x Nb matrix
//   fs2_finite_summary  count / median / mean / min / max of the finite entries of a vector
//   fs2_gauss_moments   mean and unbiased covariance of a point set, fp64, two-pass
//   fs2_frechet         Frechet distance of two Gaussians from their moments: two cyclic Jacobi
//                       eigensolves in LDS
//
// House rules of fs2_dtw / fs2_mas: no atomics, every reduction in a fixed order, nothing depends
// on the grid.  Neighbours: a block stages NN_TA rows of a in LDS as fp64, laid out [d][row] so
// that one d reads as consecutive doubles, and sweeps its share of b 256 columns at a time,
// thread t owning column c0 + t and NN_TA fp64 dot products.  |b|^2 rides along in the same loop,
// |a|^2 is formed once per block; each of the three sums runs d = 0 .. D-1 in order, and a product
// of two fp32 values is exact in fp64, so the fused multiply-add rounds exactly where a separate
// multiply and add would.  The 256 distances of a row go through an LDS tile to the row's owner
// thread, which inserts them in column order into a sorted k-list with a strict <: equal
// distances keep the lower index.  Past NN_SPLIT columns b is cut into ranges of NN_SPLIT, one
// block column each; the partial lists are merged by the same insertion, ranges in order, which
// is the insertion sequence of the unsplit sweep with the rejected candidates left out: the
// same list bit for bit.
#include <math.h>

#include "common.hpp"

namespace fs2 {

constexpr int NN_T = 256;        // threads, and columns of b per step
constexpr int NN_TA = 16;        // rows of a per block
constexpr int NN_PITCH = NN_T + 1;
constexpr int NN_SPLIT = 1024;   // columns of b per block column (a multiple of NN_T)

// insert (d, j) into the ascending list of k entries; the caller has checked d < ld[k - 1]
FS2_DEV void nn_insert(float* ld, int* li, int k, float d, int j) {
  int p = k - 1;
  while (p > 0 && d < ld[p - 1]) {
    ld[p] = ld[p - 1];
    li[p] = li[p - 1];
    --p;
  }
  ld[p] = d;
  li[p] = j;
}

struct NnArgs {
  const float* a;
  const float* b;
  const int64_t* ga;
  const int64_t* gb;
  int na, nb, dim, k, mode, nsplit;
  float* dist;      // (na, k)
  int64_t* index;   // (na, k)
  float* part_d;    // (nsplit, na, k) when nsplit > 1
  int* part_i;
};

__global__ __launch_bounds__(NN_T) void cosine_nn_kernel(NnArgs g) {
  __shared__ double as[FS2_NN_MAX_DIM * NN_TA];  // [d][row]
  __shared__ double an[NN_TA];                   // sqrt(|a|^2)
  __shared__ int64_t gas[NN_TA];
  __shared__ float dt[NN_TA * NN_PITCH];
  __shared__ float ld[NN_TA * FS2_NN_MAX_K];
  __shared__ int li[NN_TA * FS2_NN_MAX_K];
  const int tid = threadIdx.x, D = g.dim, k = g.k;
  const int r0 = blockIdx.x * NN_TA;
  const int rows = min(NN_TA, g.na - r0);
  for (int e = tid; e < D * NN_TA; e += NN_T) {
    const int r = e / D, d = e - r * D;  // d fastest: coalesced reads of a
    as[d * NN_TA + r] = r < rows ? (double)g.a[(int64_t)(r0 + r) * D + d] : 0.0;
  }
  for (int e = tid; e < NN_TA * FS2_NN_MAX_K; e += NN_T) ld[e] = INFINITY, li[e] = -1;
  if (tid < NN_TA) gas[tid] = g.ga && tid < rows ? g.ga[r0 + tid] : 0;
  __syncthreads();
  if (tid < NN_TA) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) s = fma(as[d * NN_TA + tid], as[d * NN_TA + tid], s);
    an[tid] = sqrt(s);
  }
  __syncthreads();
  const int c_lo = blockIdx.y * NN_SPLIT;
  const int c_hi = g.nsplit > 1 ? min(g.nb, c_lo + NN_SPLIT) : g.nb;
  for (int c0 = c_lo; c0 < c_hi; c0 += NN_T) {
    const int j = c0 + tid;
    if (j < c_hi) {
      const float* bp = g.b + (int64_t)j * D;
      double dot[NN_TA];
#pragma unroll
      for (int r = 0; r < NN_TA; ++r) dot[r] = 0.0;
      double nb2 = 0.0;
      for (int d = 0; d < D; ++d) {
        const double bv = (double)bp[d];
        nb2 = fma(bv, bv, nb2);
        const double* ar = as + d * NN_TA;
#pragma unroll
        for (int r = 0; r < NN_TA; ++r) dot[r] = fma(ar[r], bv, dot[r]);
      }
      const double bn = sqrt(nb2);
      const int64_t gj = g.gb ? g.gb[j] : 0;
#pragma unroll
      for (int r = 0; r < NN_TA; ++r) {
        const double den = an[r] * bn;
        const double c = den > 0.0 ? dot[r] / den : 0.0;
        const bool same = gas[r] == gj;
        const bool keep = !g.ga || (g.mode == 0 ? !same : same);
        dt[r * NN_PITCH + tid] = keep ? (float)(1.0 - c) : NAN;  // NaN never passes the <
      }
    }
    __syncthreads();
    if (tid < rows) {
      const int n = min(NN_T, c_hi - c0);
      float* rd = ld + tid * FS2_NN_MAX_K;
      int* ri = li + tid * FS2_NN_MAX_K;
      const float* row = dt + tid * NN_PITCH;
      for (int c = 0; c < n; ++c) {
        const float d = row[c];
        if (d < rd[k - 1]) nn_insert(rd, ri, k, d, c0 + c);
      }
    }
    __syncthreads();
  }
  // the lists of this block's rows: to the output, or to this block column's partials
  for (int e = tid; e < rows * k; e += NN_T) {
    const int r = e / k, s = e - r * k;
    const float d = ld[r * FS2_NN_MAX_K + s];
    const int j = li[r * FS2_NN_MAX_K + s];
    const int64_t o = (int64_t)(r0 + r) * k + s;
    if (g.nsplit > 1) {
      const int64_t po = (int64_t)blockIdx.y * g.na * k + o;
      g.part_d[po] = d;
      g.part_i[po] = j;
    } else {
      g.dist[o] = d;
      g.index[o] = j;
    }
  }
}

constexpr int NM_T = 64;
__global__ __launch_bounds__(NM_T) void cosine_nn_merge_kernel(NnArgs g) {
  __shared__ float ld[NM_T * FS2_NN_MAX_K];
  __shared__ int li[NM_T * FS2_NN_MAX_K];
  const int i = blockIdx.x * NM_T + threadIdx.x, k = g.k;
  if (i >= g.na) return;  // no barrier below
  float* rd = ld + threadIdx.x * FS2_NN_MAX_K;
  int* ri = li + threadIdx.x * FS2_NN_MAX_K;
  for (int s = 0; s < k; ++s) rd[s] = INFINITY, ri[s] = -1;
  for (int p = 0; p < g.nsplit; ++p) {
    const int64_t po = ((int64_t)p * g.na + i) * k;
    for (int s = 0; s < k; ++s) {
      const int j = g.part_i[po + s];
      if (j < 0) break;  // the list's filled entries come first
      const float d = g.part_d[po + s];
      if (d < rd[k - 1]) nn_insert(rd, ri, k, d, j);
    }
  }
  for (int s = 0; s < k; ++s) {
    g.dist[(int64_t)i * k + s] = rd[s];
    g.index[(int64_t)i * k + s] = ri[s];
  }
}

static int nn_nsplit(int64_t nb) { return nb > NN_SPLIT ? (int)((nb + NN_SPLIT - 1) / NN_SPLIT) : 1; }

// ---------------------------------------------------------------- finite summary
// Order-preserving key of an fp32: finite values map into (key(-inf), key(+inf)), NaNs outside.
FS2_DEV uint32_t fs_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FS2_DEV float fs_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
constexpr uint32_t FS_DEAD = 0xffffffffu;  // the key written for inf and NaN (itself a NaN's key)

__global__ __launch_bounds__(256) void summary_keys_kernel(const float* __restrict__ x, int n,
                                                           uint32_t* __restrict__ keys) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float v = x[e];
  keys[e] = isfinite(v) ? fs_key(v) : FS_DEAD;
}

constexpr int FS_T = 1024, FS_W = FS_T / 64;

// integer block reductions (exact in any order); the same value in every thread
FS2_DEV uint32_t fs_block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int w = 0; w < FS_W; ++w) s += red[w];
  __syncthreads();
  return s;
}
FS2_DEV uint32_t fs_block_max(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int w = 0; w < FS_W; ++w) s = max(s, red[w]);
  __syncthreads();
  return s;
}

// One workgroup.  Count, min and max in one pass over the keys; the key of rank count / 2 by a
// binary search over the 32 key bits (one counting pass per bit); the rank below it, for an even
// count, is that key again when enough keys lie below it and their largest otherwise.  The mean
// is one thread's running fp64 sum, fed 1024 entries at a time through LDS.
__global__ __launch_bounds__(FS_T) void summary_kernel(const uint32_t* __restrict__ keys, int n,
                                                       double* __restrict__ out) {
  __shared__ uint32_t red[FS_W];
  __shared__ double chunk[FS_T];
  __shared__ double total;
  const int tid = threadIdx.x;
  uint32_t cnt = 0, kmin = FS_DEAD, kmax = 0;
  for (int e = tid; e < n; e += FS_T) {
    const uint32_t q = keys[e];
    if (q != FS_DEAD) ++cnt, kmin = min(kmin, q), kmax = max(kmax, q);
  }
  const uint32_t count = fs_block_sum(cnt, red);
  kmax = fs_block_max(kmax, red);
  kmin = ~fs_block_max(~kmin, red);
  if (count == 0) {
    if (tid == 0) {
      out[0] = 0.0;
      out[1] = out[2] = out[3] = out[4] = (double)NAN;
    }
    return;
  }
  // the key of 0-based rank `rank`: fix the bits from the top; with the prefix so far, `below`
  // keys are smaller than every key that shares it
  const uint32_t rank = count / 2;
  uint32_t prefix = 0, below = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t mask = ~((1u << bit) - 1u) << 1;  // the bits above `bit` (0 for bit 31)
    uint32_t zeros = 0;
    for (int e = tid; e < n; e += FS_T) {
      const uint32_t q = keys[e];
      zeros += q != FS_DEAD && (q & mask) == prefix && !((q >> bit) & 1u);
    }
    zeros = fs_block_sum(zeros, red);
    if (rank >= below + zeros) {
      below += zeros;
      prefix |= 1u << bit;
    }
  }
  const uint32_t k_hi = prefix;  // `below` keys are smaller than k_hi
  uint32_t k_lo = k_hi;
  if ((count & 1u) == 0 && below > rank - 1) {
    // rank - 1 lies among the smaller keys: it is their largest (below == rank then)
    uint32_t m = 0;
    for (int e = tid; e < n; e += FS_T) {
      const uint32_t q = keys[e];
      if (q != FS_DEAD && q < k_hi) m = max(m, q);
    }
    k_lo = fs_block_max(m, red);
  }
  // every thread converts its entry, a dead one to +0.0 (s + 0.0 == s for every s this sum can
  // hold: it starts at +0.0 and never becomes -0.0); thread 0 adds the 1024 in order
  if (tid == 0) total = 0.0;
  for (int c0 = 0; c0 < n; c0 += FS_T) {
    const uint32_t q = c0 + tid < n ? keys[c0 + tid] : FS_DEAD;
    chunk[tid] = q != FS_DEAD ? (double)fs_unkey(q) : 0.0;
    __syncthreads();
    if (tid == 0) {
      double s = total;
#pragma unroll 16
      for (int e = 0; e < FS_T; ++e) s += chunk[e];
      total = s;
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = (double)count;
    out[1] = (count & 1u) ? (double)fs_unkey(k_hi)
                          : ((double)fs_unkey(k_lo) + (double)fs_unkey(k_hi)) / 2.0;
    out[2] = total / (double)count;
    out[3] = (double)fs_unkey(kmin);
    out[4] = (double)fs_unkey(kmax);
  }
}

// ---------------------------------------------------------------- Gaussian moments
// Block i owns row i of the covariance, thread j its column: every block forms the whole mean
// (column j by thread j, rows in order), then its row of centred products, rows in order.
// The sums are chains of dependent adds over loads that do not depend on them: GM_U rows are
// loaded ahead of the adds (one load per row in flight measured 230 ns a row).
constexpr int GM_T = 64, GM_U = 16;
__global__ __launch_bounds__(GM_T) void gauss_moments_kernel(const float* __restrict__ x, int64_t n,
                                                             int D, double* __restrict__ mean,
                                                             double* __restrict__ cov) {
  __shared__ double mu[GM_T];
  const int i = blockIdx.x, j = threadIdx.x;
  if (j < D) {
    double s = 0.0;
    int64_t r = 0;
    for (; r + GM_U <= n; r += GM_U) {
      float v[GM_U];
#pragma unroll
      for (int u = 0; u < GM_U; ++u) v[u] = x[(r + u) * D + j];
#pragma unroll
      for (int u = 0; u < GM_U; ++u) s += (double)v[u];
    }
    for (; r < n; ++r) s += (double)x[r * D + j];
    mu[j] = s / (double)n;
    if (i == 0) mean[j] = mu[j];
  }
  __syncthreads();
  if (j >= D) return;
  const double mi = mu[i], mj = mu[j];
  double s = 0.0;
  int64_t r = 0;
  for (; r + GM_U <= n; r += GM_U) {
    float vi[GM_U], vj[GM_U];
#pragma unroll
    for (int u = 0; u < GM_U; ++u) vi[u] = x[(r + u) * D + i], vj[u] = x[(r + u) * D + j];
#pragma unroll
    for (int u = 0; u < GM_U; ++u) s = fma((double)vi[u] - mi, (double)vj[u] - mj, s);
  }
  for (; r < n; ++r) s = fma((double)x[r * D + i] - mi, (double)x[r * D + j] - mj, s);
  cov[(int64_t)i * D + j] = s / (double)(n - 1);
}

// ---------------------------------------------------------------- Frechet distance
constexpr int FR_T = 256;
constexpr int FR_D = FS2_FRECHET_MAX_DIM;
constexpr int FR_P = FR_D + 1;            // row pitch in doubles
constexpr int FR_E = FR_D * FR_D / FR_T;  // matrix entries per thread
constexpr int FR_SWEEPS = 30;

// Pair k (1 <= k < m / 2; pair 0 is (m - 1, r)) of round r of the round-robin over m players
// (m even): every pair of players meets once in the m - 1 rounds, and the pairs of a round are
// disjoint, so their rotations touch different rows and columns.
FS2_DEV void fr_pair(int m, int r, int k, int& p, int& q) {
  if (k == 0) {
    p = r, q = m - 1;
  } else {
    p = (r + k) % (m - 1), q = (r - k + m - 1) % (m - 1);
  }
  if (p > q) {
    const int t = p;
    p = q, q = t;
  }
}

// Cyclic Jacobi on the symmetric A (D x D in LDS, pitch FR_P), a sweep being the m - 1 rounds
// above.  Per round: the rotation of every pair from A's entries; then A J (and V J) by columns;
// then J^T A by rows.  A rotation is skipped once |a_pq| <= 1e-20 x the largest |a_ii| at entry,
// and the sweeps end after one without a rotation or after FR_SWEEPS: decided in the block from
// a flag in LDS, nothing goes to the host.  The eigenvalues are left on A's diagonal; with V
// non-null its columns are the eigenvectors.
FS2_DEV void fr_jacobi(double* A, double* V, int D, double* cs, double* sn, int* pp, int* qq,
                       int* flag, double* scale_s) {
  const int tid = threadIdx.x;
  const int m = D + (D & 1), half = m / 2;
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < D; ++i) s = fmax(s, fabs(A[i * FR_P + i]));
    *scale_s = s;
  }
  if (V)
    for (int e = tid; e < D * D; e += FR_T) V[(e / D) * FR_P + e % D] = e / D == e % D ? 1.0 : 0.0;
  __syncthreads();
  const double tiny = 1e-20 * *scale_s;
  for (int sweep = 0; sweep < FR_SWEEPS; ++sweep) {
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int r = 0; r < m - 1; ++r) {
      if (tid < half) {
        int p, q;
        fr_pair(m, r, tid, p, q);
        double c = 1.0, s = 0.0;
        if (q < D) {
          const double apq = A[p * FR_P + q];
          if (fabs(apq) > tiny) {
            const double theta = (A[q * FR_P + q] - A[p * FR_P + p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
            *flag = 1;  // every writer stores the same value
          }
        }
        cs[tid] = c, sn[tid] = s;  // s == 0: nothing to do for this pair
        pp[tid] = p, qq[tid] = q;
      }
      __syncthreads();
      // columns: (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q) in every row of A and of V;
      // lane k of each 32 takes pair k, the 8 groups of 32 share the rows
      {
        const int k = tid & 31;
        if (k < half && sn[k] != 0.0) {
          const int p = pp[k], q = qq[k];
          const double c = cs[k], s = sn[k];
          for (int i = tid >> 5; i < D; i += FR_T / 32) {
            double* row = A + i * FR_P;
            const double xp = row[p], xq = row[q];
            row[p] = c * xp - s * xq;
            row[q] = s * xp + c * xq;
            if (V) {
              double* vr = V + i * FR_P;
              const double vp = vr[p], vq = vr[q];
              vr[p] = c * vp - s * vq;
              vr[q] = s * vp + c * vq;
            }
          }
        }
      }
      __syncthreads();
      // rows: the same on (A[p][j], A[q][j]); lane j of each 64 takes column j, the 4 waves
      // share the pairs
      {
        const int j = tid & 63;
        if (j < D)
          for (int k = tid >> 6; k < half; k += FR_T / 64) {
            if (sn[k] == 0.0) continue;
            const int p = pp[k], q = qq[k];
            const double c = cs[k], s = sn[k];
            const double xp = A[p * FR_P + j], xq = A[q * FR_P + j];
            A[p * FR_P + j] = c * xp - s * xq;
            A[q * FR_P + j] = s * xp + c * xq;
          }
      }
      __syncthreads();
    }
    if (*flag == 0) break;  // read by every thread after the round's last barrier
    __syncthreads();        // ... and before thread 0 clears it
  }
}

__global__ __launch_bounds__(FR_T) void frechet_kernel(const double* __restrict__ mean_a,
                                                       const double* __restrict__ cov_a,
                                                       const double* __restrict__ mean_b,
                                                       const double* __restrict__ cov_b, int D,
                                                       double* __restrict__ out) {
  __shared__ double A[FR_D * FR_P];
  __shared__ double V[FR_D * FR_P];
  __shared__ double w[FR_D], cs[FR_D / 2], sn[FR_D / 2];
  __shared__ int pp[FR_D / 2], qq[FR_D / 2];
  __shared__ double scale_s;
  __shared__ int flag;
  const int tid = threadIdx.x, pr = blockIdx.x, DD = D * D;
  const double* ma = mean_a + (int64_t)pr * D;
  const double* mb = mean_b + (int64_t)pr * D;
  const double* ca = cov_a + (int64_t)pr * DD;
  const double* cb = cov_b + (int64_t)pr * DD;
  // Sigma_a, symmetrised, = V diag(lambda) V^T
  for (int e = tid; e < DD; e += FR_T) {
    const int i = e / D, j = e - i * D;
    A[i * FR_P + j] = 0.5 * (ca[i * D + j] + ca[j * D + i]);
  }
  __syncthreads();
  fr_jacobi(A, V, D, cs, sn, pp, qq, &flag, &scale_s);
  if (tid < D) w[tid] = sqrt(fmax(A[tid * FR_P + tid], 0.0));
  __syncthreads();
  // S = V diag(w) V^T into A
  for (int e = tid; e < DD; e += FR_T) {
    const int i = e / D, j = e - i * D;
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += V[i * FR_P + k] * w[k] * V[j * FR_P + k];
    A[i * FR_P + j] = s;
  }
  __syncthreads();
  // T = S Sigma_b into V
  for (int e = tid; e < DD; e += FR_T) {
    const int i = e / D, j = e - i * D;
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += A[i * FR_P + k] * cb[k * D + j];
    V[i * FR_P + j] = s;
  }
  __syncthreads();
  // M = T S, held in registers until every thread has read T, then over T
  double mreg[FR_E];
#pragma unroll
  for (int u = 0; u < FR_E; ++u) {
    const int e = tid + u * FR_T;
    double s = 0.0;
    if (e < DD) {
      const int i = e / D, j = e - i * D;
      for (int k = 0; k < D; ++k) s += V[i * FR_P + k] * A[k * FR_P + j];
    }
    mreg[u] = s;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < FR_E; ++u) {
    const int e = tid + u * FR_T;
    if (e < DD) V[(e / D) * FR_P + e % D] = mreg[u];
  }
  __syncthreads();
  for (int e = tid; e < DD; e += FR_T) {
    const int i = e / D, j = e - i * D;
    A[i * FR_P + j] = 0.5 * (V[i * FR_P + j] + V[j * FR_P + i]);
  }
  __syncthreads();
  fr_jacobi(A, nullptr, D, cs, sn, pp, qq, &flag, &scale_s);
  if (tid == 0) {
    double dm = 0.0, tr = 0.0, rt = 0.0;
    for (int i = 0; i < D; ++i) {
      const double t = ma[i] - mb[i];
      dm += t * t;
    }
    for (int i = 0; i < D; ++i) tr += ca[i * D + i];
    for (int i = 0; i < D; ++i) tr += cb[i * D + i];
    for (int i = 0; i < D; ++i) rt += sqrt(fmax(A[i * FR_P + i], 0.0));
    double* o = out + (int64_t)pr * 4;
    o[0] = dm + tr - 2.0 * rt;
    o[1] = dm;
    o[2] = tr;
    o[3] = rt;
  }
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int64_t fs2_cosine_nn_ws_bytes(int64_t na, int64_t nb, int64_t k) {
  if (na < 1 || nb < 1 || k < 1 || k > FS2_NN_MAX_K || nb >= (1ll << 31)) return 0;
  const int64_t ns = nn_nsplit(nb);
  return ns > 1 ? ns * na * k * 8 : 0;
}

int fs2_cosine_nn(const float* a, const float* b, int64_t na, int64_t nb, int64_t dim, int64_t k,
                  const int64_t* group_a, const int64_t* group_b, int mode, float* dist,
                  int64_t* index, void* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(dim >= 1 && dim <= FS2_NN_MAX_DIM, "fs2_cosine_nn: dim %lld (1..%d)",
                (long long)dim, FS2_NN_MAX_DIM);
  FS2_CHECK_ARG(k >= 1 && k <= FS2_NN_MAX_K, "fs2_cosine_nn: k %lld (1..%d)", (long long)k,
                FS2_NN_MAX_K);
  FS2_CHECK_ARG(na >= 0 && na < (1ll << 31) / FS2_NN_MAX_K && nb >= 0 && nb < (1ll << 31),
                "fs2_cosine_nn: na %lld (0..2^27 - 1), nb %lld (0..2^31 - 1)", (long long)na,
                (long long)nb);
  FS2_CHECK_ARG(mode == 0 || mode == 1, "fs2_cosine_nn: mode %d (0: skip the same group, 1: keep "
                "only the same group)", mode);
  FS2_CHECK_ARG((group_a == nullptr) == (group_b == nullptr),
                "fs2_cosine_nn: the groups come as a pair or not at all");
  if (na == 0) return FS2_OK;
  FS2_CHECK_ARG(a && dist && index && (b || nb == 0), "fs2_cosine_nn: missing operand");
  const int ns = nn_nsplit(nb);
  FS2_CHECK_ARG(ns <= 65535, "fs2_cosine_nn: nb %lld (at most %d)", (long long)nb, 65535 * NN_SPLIT);
  const int64_t need = fs2_cosine_nn_ws_bytes(na, nb, k);
  FS2_CHECK_ARG(need == 0 || (ws && ws_bytes >= need),
                "fs2_cosine_nn: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)need);
  hipStream_t st = as_stream(stream);
  NnArgs g;
  g.a = a, g.b = b, g.ga = group_a, g.gb = group_b;
  g.na = (int)na, g.nb = (int)nb, g.dim = (int)dim, g.k = (int)k, g.mode = mode, g.nsplit = ns;
  g.dist = dist, g.index = index;
  g.part_d = nullptr, g.part_i = nullptr;
  if (ns > 1) {
    poison(ws, ws_bytes, st);
    g.part_d = (float*)ws;
    g.part_i = (int*)(g.part_d + (int64_t)ns * na * k);
  }
  // nb = 0: one block column with an empty sweep writes the empty lists
  const dim3 grid((unsigned)((na + NN_TA - 1) / NN_TA), (unsigned)ns);
  cosine_nn_kernel<<<grid, NN_T, 0, st>>>(g);
  if (ns > 1)
    cosine_nn_merge_kernel<<<(unsigned)((na + NM_T - 1) / NM_T), NM_T, 0, st>>>(g);
  return launch_status("fs2_cosine_nn");
}

int64_t fs2_finite_summary_ws_bytes(int64_t n) {
  return n >= 1 && n <= FS2_SUMMARY_MAX_N ? n * 4 : 0;
}

int fs2_finite_summary(const float* x, int64_t n, double* out, void* ws, int64_t ws_bytes,
                       void* stream) {
  FS2_CHECK_ARG(n >= 0 && n <= FS2_SUMMARY_MAX_N, "fs2_finite_summary: n %lld (0..%d)",
                (long long)n, FS2_SUMMARY_MAX_N);
  FS2_CHECK_ARG(out, "fs2_finite_summary: missing operand");
  FS2_CHECK_ARG(n == 0 || (x && ws && ws_bytes >= n * 4),
                "fs2_finite_summary: missing operand, or workspace %lld bytes, %lld needed",
                (long long)ws_bytes, (long long)n * 4);
  hipStream_t st = as_stream(stream);
  if (n > 0) {
    poison(ws, ws_bytes, st);
    summary_keys_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(x, (int)n, (uint32_t*)ws);
  }
  // n = 0 still has a record to write: the one-block kernel sees no key
  summary_kernel<<<1, FS_T, 0, st>>>((const uint32_t*)ws, (int)n, out);
  return launch_status("fs2_finite_summary");
}

int fs2_gauss_moments(const float* x, int64_t n, int64_t dim, double* mean, double* cov,
                      void* stream) {
  FS2_CHECK_ARG(dim >= 1 && dim <= FS2_FRECHET_MAX_DIM, "fs2_gauss_moments: dim %lld (1..%d)",
                (long long)dim, FS2_FRECHET_MAX_DIM);
  FS2_CHECK_ARG(n >= 2 && n < (1ll << 40), "fs2_gauss_moments: n %lld (at least 2 rows)",
                (long long)n);
  FS2_CHECK_ARG(x && mean && cov, "fs2_gauss_moments: missing operand");
  gauss_moments_kernel<<<(unsigned)dim, GM_T, 0, as_stream(stream)>>>(x, n, (int)dim, mean, cov);
  return launch_status("fs2_gauss_moments");
}

int fs2_frechet(const double* mean_a, const double* cov_a, const double* mean_b,
                const double* cov_b, int64_t pairs, int64_t dim, double* out, void* stream) {
  FS2_CHECK_ARG(dim >= 1 && dim <= FS2_FRECHET_MAX_DIM, "fs2_frechet: dim %lld (1..%d)",
                (long long)dim, FS2_FRECHET_MAX_DIM);
  FS2_CHECK_ARG(pairs >= 0 && pairs < (1 << 20), "fs2_frechet: pairs %lld", (long long)pairs);
  if (pairs == 0) return FS2_OK;
  FS2_CHECK_ARG(mean_a && cov_a && mean_b && cov_b && out, "fs2_frechet: missing operand");
  frechet_kernel<<<(unsigned)pairs, FR_T, 0, as_stream(stream)>>>(mean_a, cov_a, mean_b, cov_b,
                                                                  (int)dim, out);
  return launch_status("fs2_frechet");
}

}  // extern "C"
