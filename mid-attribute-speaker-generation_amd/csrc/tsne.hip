// Exact t-SNE of speaker embeddings (train_speech_embedder.py:311-385, visualize_embeddings):
// the per-speaker mean points, the PCA initialisation, the perplexity search and the joint
// probabilities, and the gradient descent of scikit-learn's TSNE(method='exact') with its gains,
// momentum, two stages and stopping rules kept in a device record.  fp32 storage; the
// perplexity search, the eigenvectors and every sum over a row or over the rows run in fp64.
// No atomics: every accumulation has a fixed order (a lane takes j = lane, lane + 64, ... in
// order, then the xor tree over the wave, then the waves in order), so a run is bitwise
// repeatable.  The descent is two plain launches per iteration; the kernel boundary is the only
// grid-wide synchronisation.
#include <float.h>
#include <math.h>

#include "common.hpp"

namespace fs2 {

constexpr int TS_NMAX = 4096, TS_DMAX = 1024, TS_T = 256, TS_W = TS_T / 64;
constexpr double TS_EPS = DBL_EPSILON;      // sklearn's MACHINE_EPSILON
constexpr int TS_CHECK = 50;                // _N_ITER_CHECK
constexpr int TS_PCA_ITERS = 1000;          // cap of the subspace iteration

// the device state record (doubles; integers are exact in them)
enum {
  TS_ITER = 0,      // last iteration the control saw
  TS_STAGE,         // 1: early exaggeration, 2: final
  TS_BEST,          // best error of the stage
  TS_BEST_ITER,
  TS_DONE,          // 1: the descent has ended; phases A and B return at once
  TS_N_ITER,        // n_iter_: the last iteration that ran
  TS_ERROR,         // kl_divergence_: the last evaluated error
  TS_START,         // first iteration of the current stage
  TS_GRAD_NORM,     // norm at the last check
  TS_MAX_ITER,
  TS_EXPLORE,
  TS_WINDOW,        // n_iter_without_progress of stage 2
  TS_EXAG,
  TS_LR,
  TS_MIN_GRAD,
  TS_STATE_LEN = 16
};

FS2_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
FS2_DEV double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// Sum over a block of TS_T threads, the same value in every thread: wave trees, then the waves
// in order.  `red` holds TS_W doubles; two barriers, so it can be reused at once.
FS2_DEV double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < TS_W; ++w) s += red[w];
  __syncthreads();
  return s;
}

// sum of n doubles by a block of TS_T threads: thread t adds t, t + TS_T, ... in order
FS2_DEV double block_reduce_array(const double* __restrict__ a, int n, double* red) {
  double s = 0.0;
  for (int k = threadIdx.x; k < n; k += TS_T) s += a[k];
  return block_sum_f64(s, red);
}

// ---------------------------------------------------------------- points
// out[s] = mean of the first min(count, cap) rows of segment s; thread d adds in row order.
__global__ __launch_bounds__(TS_T) void tsne_points_kernel(const float* __restrict__ x,
                                                           const int64_t* __restrict__ seg_start,
                                                           int dim, int64_t cap,
                                                           float* __restrict__ out) {
  const int64_t s = blockIdx.x, r0 = seg_start[s];
  int64_t cnt = seg_start[s + 1] - r0;
  if (cnt > cap) cnt = cap;
  for (int d = threadIdx.x; d < dim; d += TS_T) {
    float a = 0.f;
    for (int64_t r = r0; r < r0 + cnt; ++r) a += x[r * dim + d];
    out[s * dim + d] = a / (float)cnt;
  }
}

// ---------------------------------------------------------------- PCA initialisation
// ws (doubles): mean[D] | V[2 D] | Yd[2 N] | cov[D D]
__global__ __launch_bounds__(TS_T) void tsne_pca_mean_kernel(const float* __restrict__ X, int n,
                                                             int dim, double* __restrict__ mean) {
  const int d = blockIdx.x * TS_T + threadIdx.x;
  if (d >= dim) return;
  double a = 0.0;
  for (int r = 0; r < n; ++r) a += (double)X[(int64_t)r * dim + d];
  mean[d] = a / (double)n;
}

// cov[a][b] = sum_r (x[r][a] - mean[a]) (x[r][b] - mean[b]) / n, rows in order; a block owns a
// 16 x 16 tile and stages 16 rows of its two column bands at a time
__global__ __launch_bounds__(256) void tsne_pca_cov_kernel(const float* __restrict__ X, int n,
                                                           int dim, const double* __restrict__ mean,
                                                           double* __restrict__ cov) {
  __shared__ double xa[16][17], xb[16][17];
  const int ta = threadIdx.x >> 4, tb = threadIdx.x & 15;
  const int a0 = blockIdx.y * 16, b0 = blockIdx.x * 16;
  double acc = 0.0;
  for (int r0 = 0; r0 < n; r0 += 16) {
    const int r = r0 + ta;
    const bool in = r < n;
    xa[ta][tb] = in && a0 + tb < dim ? (double)X[(int64_t)r * dim + a0 + tb] - mean[a0 + tb] : 0.0;
    xb[ta][tb] = in && b0 + tb < dim ? (double)X[(int64_t)r * dim + b0 + tb] - mean[b0 + tb] : 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = fma(xa[k][ta], xb[k][tb], acc);
    __syncthreads();
  }
  if (a0 + ta < dim && b0 + tb < dim) cov[(int64_t)(a0 + ta) * dim + b0 + tb] = acc / (double)n;
}

// The two leading eigenvectors of cov by subspace iteration with a Rayleigh-Ritz rotation, one
// block: W = C V, H = V^T W (2 x 2), the Jacobi rotation R that diagonalises H (larger value
// first), V <- Gram-Schmidt(W R).  The Ritz vectors converge at the rate lambda_3 / lambda_k;
// the loop stops when neither vector moved by more than 1e-14 or at TS_PCA_ITERS, whichever
// comes first (all threads see the same sums, so the decision is uniform).  Then the sign rule
// of svd_flip (V-based): each component's first largest-magnitude loading is positive.
__global__ __launch_bounds__(TS_T) void tsne_pca_eig_kernel(const double* __restrict__ cov, int dim,
                                                            double* __restrict__ V) {
  __shared__ double v0[TS_DMAX], v1[TS_DMAX];
  __shared__ double red[TS_W];
  __shared__ int arg[2];
  const int tid = threadIdx.x;
  constexpr int PER = TS_DMAX / TS_T;
  // a fixed start that is orthogonal to nothing in particular
  {
    double s0 = 0.0, s1 = 0.0;
    for (int d = tid; d < dim; d += TS_T) {
      uint32_t h = (uint32_t)d * 2654435761u + 12345u;
      h ^= h >> 15;
      h *= 2246822519u;
      h ^= h >> 13;
      v0[d] = 1.0 + (double)(h & 0xffffu) / 65536.0;
      v1[d] = ((d & 1) ? -1.0 : 1.0) * (0.5 + (double)(h >> 16) / 65536.0);
      s0 += v0[d] * v0[d];
      s1 += v1[d] * v1[d];
    }
    s0 = block_sum_f64(s0, red);
    s1 = block_sum_f64(s1, red);
    for (int d = tid; d < dim; d += TS_T) {
      v0[d] /= sqrt(s0);
      v1[d] /= sqrt(s1);
    }
    __syncthreads();
  }
  for (int it = 0; it < TS_PCA_ITERS; ++it) {
    double w0[PER], w1[PER];
    double h00 = 0.0, h01 = 0.0, h11 = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int d = tid + k * TS_T;
      w0[k] = w1[k] = 0.0;
      if (d < dim) {
        double a = 0.0, b = 0.0;
        // cov is symmetric: column d read down the rows, coalesced across the threads
        for (int e = 0; e < dim; ++e) {
          const double c = cov[(int64_t)e * dim + d];
          a = fma(c, v0[e], a);
          b = fma(c, v1[e], b);
        }
        w0[k] = a;
        w1[k] = b;
        h00 = fma(v0[d], a, h00);
        h01 = fma(v0[d], b, h01);
        h11 = fma(v1[d], b, h11);
      }
    }
    h00 = block_sum_f64(h00, red);
    h01 = block_sum_f64(h01, red);
    h11 = block_sum_f64(h11, red);
    // Jacobi rotation of the symmetric 2 x 2 H, |theta| <= pi / 4
    double c = 1.0, s = 0.0;
    if (h01 != 0.0) {
      const double tau = (h11 - h00) / (2.0 * h01);
      const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
      c = 1.0 / sqrt(1.0 + t * t);
      s = t * c;
    }
    const double l0 = c * c * h00 - 2.0 * s * c * h01 + s * s * h11;
    const double l1 = s * s * h00 + 2.0 * s * c * h01 + c * c * h11;
    const bool swap = l1 > l0;
    double n0 = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const double a = c * w0[k] - s * w1[k], b = s * w0[k] + c * w1[k];
      w0[k] = swap ? b : a;
      w1[k] = swap ? a : b;
      n0 = fma(w0[k], w0[k], n0);
    }
    n0 = block_sum_f64(n0, red);
    const double i0 = n0 > 0.0 ? 1.0 / sqrt(n0) : 0.0;
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      w0[k] *= i0;
      dot = fma(w0[k], w1[k], dot);
    }
    dot = block_sum_f64(dot, red);
    double n1 = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      w1[k] -= dot * w0[k];
      n1 = fma(w1[k], w1[k], n1);
    }
    n1 = block_sum_f64(n1, red);
    const double i1 = n1 > 0.0 ? 1.0 / sqrt(n1) : 0.0;
    double moved = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int d = tid + k * TS_T;
      if (d < dim) {
        w1[k] *= i1;
        moved = fmax(moved, fmax(fabs(w0[k] - v0[d]), fabs(w1[k] - v1[d])));
      }
    }
    moved = wave_max_f64(moved);
    if ((tid & 63) == 0) red[tid >> 6] = moved;
    __syncthreads();  // every thread has read v0, v1 of this round by now
    moved = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int d = tid + k * TS_T;
      if (d < dim) {
        v0[d] = w0[k];
        v1[d] = w1[k];
      }
    }
    __syncthreads();
    if (moved <= 1e-14) break;
  }
  if (tid < 2) {
    const double* v = tid ? v1 : v0;
    int best = 0;
    double m = -1.0;
    for (int d = 0; d < dim; ++d)
      if (fabs(v[d]) > m) m = fabs(v[d]), best = d;
    arg[tid] = best;
  }
  __syncthreads();
  const double s0 = v0[arg[0]] < 0.0 ? -1.0 : 1.0, s1 = v1[arg[1]] < 0.0 ? -1.0 : 1.0;
  for (int d = tid; d < dim; d += TS_T) {
    V[d] = s0 * v0[d];
    V[dim + d] = s1 * v1[d];
  }
}

// Yd[r] = (x[r] - mean) . V, one wave per row
__global__ __launch_bounds__(TS_T) void tsne_pca_project_kernel(const float* __restrict__ X, int n,
                                                                int dim,
                                                                const double* __restrict__ mean,
                                                                const double* __restrict__ V,
                                                                double* __restrict__ Yd) {
  const int r = blockIdx.x * TS_W + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= n) return;
  double a = 0.0, b = 0.0;
  for (int d = lane; d < dim; d += 64) {
    const double xc = (double)X[(int64_t)r * dim + d] - mean[d];
    a = fma(xc, V[d], a);
    b = fma(xc, V[dim + d], b);
  }
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  if (lane == 0) Yd[2 * r] = a, Yd[2 * r + 1] = b;
}

// Y0 = Yd * 1e-4 / std(Yd[:, 0]) (population), one block
__global__ __launch_bounds__(TS_T) void tsne_pca_scale_kernel(const double* __restrict__ Yd, int n,
                                                              float* __restrict__ Y0) {
  __shared__ double red[TS_W];
  double s = 0.0;
  for (int r = threadIdx.x; r < n; r += TS_T) s += Yd[2 * r];
  const double mean = block_sum_f64(s, red) / (double)n;
  double q = 0.0;
  for (int r = threadIdx.x; r < n; r += TS_T) {
    const double d = Yd[2 * r] - mean;
    q = fma(d, d, q);
  }
  const double sd = sqrt(block_sum_f64(q, red) / (double)n);
  for (int k = threadIdx.x; k < 2 * n; k += TS_T) Y0[k] = (float)(Yd[k] / sd * 1e-4);
}

// ---------------------------------------------------------------- affinities
// One block per row i: the row of squared distances goes to LDS as fp32 (fp64 sums of the
// direct (x_i - x_j)^2 form, one wave per j), then sklearn's binary search on beta in fp64.
// Every thread holds the same sums, so the search's branches are uniform.  Writes the
// conditional row C[i, :] (fp64, zero diagonal) and beta[i].
__global__ __launch_bounds__(TS_T) void tsne_cond_kernel(const float* __restrict__ X, int n, int dim,
                                                         double target, double* __restrict__ C,
                                                         double* __restrict__ beta_out) {
  __shared__ float xi[TS_DMAX];
  __shared__ float dist[TS_NMAX];
  __shared__ double red[TS_W];
  const int i = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int d = tid; d < dim; d += TS_T) xi[d] = X[(int64_t)i * dim + d];
  __syncthreads();
  for (int j = wave; j < n; j += TS_W) {
    const float* xj = X + (int64_t)j * dim;
    double a = 0.0;
    for (int d = lane; d < dim; d += 64) {
      const double t = (double)xi[d] - (double)xj[d];
      a = fma(t, t, a);
    }
    a = wave_sum_f64(a);
    if (lane == 0) dist[j] = (float)a;
  }
  __syncthreads();

  const double tol = (double)1e-5f, zero_sum = (double)1e-8f;  // floats in _utils.pyx
  double beta = 1.0, beta_row = 1.0, lo = -INFINITY, hi = INFINITY, sum = 1.0;
  for (int l = 0; l < 100; ++l) {
    double s = 0.0, sd = 0.0;
    beta_row = beta;
    for (int j = tid; j < n; j += TS_T)
      if (j != i) {
        const double d = (double)dist[j], p = exp(-d * beta);
        s += p;
        sd = fma(d, p, sd);
      }
    s = block_sum_f64(s, red);
    sd = block_sum_f64(sd, red);
    sum = s == 0.0 ? zero_sum : s;
    const double diff = log(sum) + beta * (sd / sum) - target;
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  // the row is that of the beta evaluated last; a search that runs out of steps reports the
  // next beta, as sklearn does
  for (int j = tid; j < n; j += TS_T)
    C[(int64_t)i * n + j] = j == i ? 0.0 : exp(-(double)dist[j] * beta_row) / sum;
  if (tid == 0 && beta_out) beta_out[i] = beta;
}

// rs[i] = sum_j (C[i, j] + C[j, i]), one wave per row
__global__ __launch_bounds__(TS_T) void tsne_sym_rowsum_kernel(const double* __restrict__ C, int n,
                                                               double* __restrict__ rs) {
  const int i = blockIdx.x * TS_W + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += C[(int64_t)i * n + j] + C[(int64_t)j * n + i];
  s = wave_sum_f64(s);
  if (lane == 0) rs[i] = s;
}

// P = max((C + C^T) / max(sum, eps), eps), zero diagonal; every block adds the row sums in the
// same order
__global__ __launch_bounds__(TS_T) void tsne_joint_kernel(const double* __restrict__ C, int n,
                                                          const double* __restrict__ rs,
                                                          float* __restrict__ P,
                                                          double* __restrict__ P64) {
  __shared__ double red[TS_W];
  const double total = fmax(block_reduce_array(rs, n, red), TS_EPS);
  const int i = blockIdx.x;
  for (int j = threadIdx.x; j < n; j += TS_T) {
    const int64_t e = (int64_t)i * n + j;
    const double p = j == i ? 0.0 : fmax((C[e] + C[(int64_t)j * n + i]) / total, TS_EPS);
    P[e] = (float)p;
    if (P64) P64[e] = p;
  }
}

// ---------------------------------------------------------------- descent
__global__ void tsne_state_init_kernel(double* st, double max_iter, double explore, double window,
                                       double exag, double lr, double min_grad) {
  if (threadIdx.x != 0) return;
  st[TS_ITER] = -1.0;
  st[TS_STAGE] = 1.0;
  st[TS_BEST] = DBL_MAX;
  st[TS_BEST_ITER] = 0.0;
  st[TS_DONE] = 0.0;
  st[TS_N_ITER] = -1.0;
  st[TS_ERROR] = NAN;
  st[TS_START] = 0.0;
  st[TS_GRAD_NORM] = NAN;
  st[TS_MAX_ITER] = max_iter;
  st[TS_EXPLORE] = explore;
  st[TS_WINDOW] = window;
  st[TS_EXAG] = exag;
  st[TS_LR] = lr;
  st[TS_MIN_GRAD] = min_grad;
  st[15] = 0.0;
}

// the student-t kernel of a pair, fp32; phases A and B form it with the same operations
FS2_DEV float pair_w(float2 yi, float2 yj, float& d0, float& d1) {
  d0 = yi.x - yj.x;
  d1 = yi.y - yj.y;
  return 1.0f / (1.0f + fmaf(d1, d1, d0 * d0));
}

// Phase A: rowsum[i] = sum_{j != i} w_ij, one wave per row.
__global__ __launch_bounds__(TS_T) void tsne_rowsum_kernel(const float2* __restrict__ Y, int n,
                                                           const double* __restrict__ st,
                                                           double* __restrict__ rowsum) {
  if (st && st[TS_DONE] != 0.0) return;
  const int i = blockIdx.x * TS_W + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const float2 yi = Y[i];
  double s = 0.0;
  for (int j = lane; j < n; j += 64)
    if (j != i) {
      float d0, d1;
      s += (double)pair_w(yi, Y[j], d0, d1);
    }
  s = wave_sum_f64(s);
  if (lane == 0) rowsum[i] = s;
}

struct TsneStep {
  const float* P;
  const float2* Y;
  float2* Y_out;
  float2* update;
  float2* gains;
  const double* st;      // null: the explicit scalars below (one step on explicit state)
  const double* rowsum;
  double* kl_rows;       // nullable
  double* gn_rows;       // nullable
  int n, iter;
  int evaluate, reset, no_update;
  float exag, momentum, lr;
};

FS2_DEV void gain_update(float g, float& gain, float& upd, float momentum, float lr, float& y,
                         double& gn) {
  gain = upd * g < 0.0f ? gain + 0.2f : gain * 0.8f;
  gain = fmaxf(gain, 0.01f);
  g *= gain;
  upd = momentum * upd - lr * g;
  y += upd;
  gn = fma((double)g, (double)g, gn);
}

// Phase B: one wave per row.  Z = the row sums added in the same order by every block; the
// gradient and, on an evaluating iteration, the row's share of the error from the pair terms.
__global__ __launch_bounds__(TS_T) void tsne_update_kernel(TsneStep a) {
  __shared__ double red[TS_W];
  const double* st = a.st;
  if (st && st[TS_DONE] != 0.0) return;
  const int n = a.n;
  float exag = a.exag, momentum = a.momentum, lr = a.lr;
  bool evaluate = a.evaluate != 0, reset = a.reset != 0;
  if (st) {
    const bool first = st[TS_STAGE] == 1.0;
    const int last = (int)(first ? st[TS_EXPLORE] : st[TS_MAX_ITER]) - 1;
    exag = first ? (float)st[TS_EXAG] : 1.0f;
    momentum = first ? 0.5f : 0.8f;
    lr = (float)st[TS_LR];
    evaluate = (a.iter + 1) % TS_CHECK == 0 || a.iter == last;
    reset = !first && a.iter == (int)st[TS_START];
  }
  const double Z = block_reduce_array(a.rowsum, n, red);
  const double inv_z = 1.0 / Z;
  const float eps = (float)TS_EPS;
  const int i = blockIdx.x * TS_W + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const float2 yi = a.Y[i];
  const float* prow = a.P + (int64_t)i * n;
  double g0 = 0.0, g1 = 0.0, kl = 0.0;
  for (int j = lane; j < n; j += 64)
    if (j != i) {
      float d0, d1;
      const float w = pair_w(yi, a.Y[j], d0, d1);
      const double qd = fmax((double)w * inv_z, TS_EPS);  // one rounding of w / Z
      const float q = (float)qd;
      const float p = exag * prow[j];
      const float t = (p - q) * w;
      g0 += (double)(t * d0);
      g1 += (double)(t * d1);
      if (evaluate) kl += (double)p * log((double)fmaxf(p, eps) / qd);
    }
  g0 = wave_sum_f64(g0);
  g1 = wave_sum_f64(g1);
  if (evaluate) kl = wave_sum_f64(kl);
  if (lane != 0) return;
  if (evaluate && a.kl_rows) a.kl_rows[i] = kl;
  if (a.no_update) return;
  float2 upd = reset ? make_float2(0.f, 0.f) : a.update[i];
  float2 gain = reset ? make_float2(1.f, 1.f) : a.gains[i];
  float2 y = yi;
  double gn = 0.0;
  gain_update((float)(4.0 * g0), gain.x, upd.x, momentum, lr, y.x, gn);
  gain_update((float)(4.0 * g1), gain.y, upd.y, momentum, lr, y.y, gn);
  a.update[i] = upd;
  a.gains[i] = gain;
  a.Y_out[i] = y;
  if (a.gn_rows) a.gn_rows[i] = gn;
}

// The rules of sklearn's _gradient_descent and of the two stages of TSNE._tsne for iteration
// `iter`, one block: error = sum of kl_rows, grad_norm = sqrt(sum of gn_rows).  Stage 1 may run
// to exploration_iter whatever max_iter is, as sklearn's does; when it ends at or past
// max_iter - 1 there is no stage 2 and the descent is done.
__global__ __launch_bounds__(TS_T) void tsne_control_kernel(double* st, int n, int iter,
                                                            const double* __restrict__ kl_rows,
                                                            const double* __restrict__ gn_rows) {
  __shared__ double red[TS_W];
  if (st[TS_DONE] != 0.0) return;
  const double error = block_reduce_array(kl_rows, n, red);
  const double grad_norm = sqrt(block_reduce_array(gn_rows, n, red));
  if (threadIdx.x != 0) return;
  const bool first = st[TS_STAGE] == 1.0;
  const int last = (int)(first ? st[TS_EXPLORE] : st[TS_MAX_ITER]) - 1;
  const bool check = (iter + 1) % TS_CHECK == 0;
  st[TS_ITER] = (double)iter;
  if (check || iter == last) st[TS_ERROR] = error;  // kl_rows is current only then
  bool stop = false;
  if (check) {
    st[TS_GRAD_NORM] = grad_norm;
    const double window = first ? st[TS_EXPLORE] : st[TS_WINDOW];
    if (error < st[TS_BEST]) {
      st[TS_BEST] = error;
      st[TS_BEST_ITER] = (double)iter;
    } else if ((double)iter - st[TS_BEST_ITER] > window) {
      stop = true;
    }
    if (!stop && grad_norm <= st[TS_MIN_GRAD]) stop = true;
  }
  if (stop || iter == last) {
    if (first && (double)(iter + 1) < st[TS_MAX_ITER]) {
      st[TS_STAGE] = 2.0;
      st[TS_START] = (double)(iter + 1);
      st[TS_BEST] = DBL_MAX;
      st[TS_BEST_ITER] = (double)(iter + 1);
    } else {
      st[TS_DONE] = 1.0;
      st[TS_N_ITER] = (double)iter;
    }
  }
}

// error[0] = sum of kl_rows (TSNE.kl)
__global__ __launch_bounds__(TS_T) void tsne_sum_kernel(const double* __restrict__ rows, int n,
                                                        double* __restrict__ out) {
  __shared__ double red[TS_W];
  const double s = block_reduce_array(rows, n, red);
  if (threadIdx.x == 0) out[0] = s;
}

// out = (Y - min) / (max - min) per column, one block; a constant column gives 0 / 0 = NaN
__global__ __launch_bounds__(TS_T) void tsne_finish_kernel(const float2* __restrict__ Y, int n,
                                                           float2* __restrict__ out) {
  __shared__ float red[4][TS_W];
  float lo0 = INFINITY, hi0 = -INFINITY, lo1 = INFINITY, hi1 = -INFINITY;
  for (int r = threadIdx.x; r < n; r += TS_T) {
    const float2 y = Y[r];
    lo0 = fminf(lo0, y.x), hi0 = fmaxf(hi0, y.x);
    lo1 = fminf(lo1, y.y), hi1 = fmaxf(hi1, y.y);
  }
  lo0 = -wave_max(-lo0), hi0 = wave_max(hi0), lo1 = -wave_max(-lo1), hi1 = wave_max(hi1);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = lo0, red[1][w] = hi0, red[2][w] = lo1, red[3][w] = hi1;
  }
  __syncthreads();
  lo0 = red[0][0], hi0 = red[1][0], lo1 = red[2][0], hi1 = red[3][0];
#pragma unroll
  for (int w = 1; w < TS_W; ++w) {
    lo0 = fminf(lo0, red[0][w]), hi0 = fmaxf(hi0, red[1][w]);
    lo1 = fminf(lo1, red[2][w]), hi1 = fmaxf(hi1, red[3][w]);
  }
  for (int r = threadIdx.x; r < n; r += TS_T) {
    const float2 y = Y[r];
    out[r] = make_float2((y.x - lo0) / (hi0 - lo0), (y.y - lo1) / (hi1 - lo1));
  }
}

static bool tsne_n_ok(int64_t n) { return n >= 0 && n <= TS_NMAX; }

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_tsne_points(const float* x, const int64_t* seg_start, int64_t n, int64_t dim, int64_t cap,
                    float* out, void* stream) {
  FS2_CHECK_ARG(dim >= 1 && dim <= TS_DMAX, "fs2_tsne_points: dim %lld (1..%d)", (long long)dim,
                TS_DMAX);
  FS2_CHECK_ARG(n >= 0 && n < (1ll << 31), "fs2_tsne_points: n %lld", (long long)n);
  FS2_CHECK_ARG(cap >= 1, "fs2_tsne_points: cap %lld (>= 1)", (long long)cap);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(x && seg_start && out, "fs2_tsne_points: missing operand");
  tsne_points_kernel<<<(unsigned)n, TS_T, 0, as_stream(stream)>>>(x, seg_start, (int)dim, cap, out);
  return launch_status("fs2_tsne_points");
}

int64_t fs2_tsne_pca_ws_bytes(int64_t n, int64_t dim) {
  if (n < 1 || dim < 1) return 0;
  return (dim + 2 * dim + 2 * n + dim * dim) * 8;
}

int fs2_tsne_pca_init(const float* X, int64_t n, int64_t dim, float* Y0, void* ws,
                      int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(tsne_n_ok(n), "fs2_tsne_pca_init: n %lld (0..%d)", (long long)n, TS_NMAX);
  FS2_CHECK_ARG(dim >= 1 && dim <= TS_DMAX, "fs2_tsne_pca_init: dim %lld (1..%d)", (long long)dim,
                TS_DMAX);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(X && Y0 && ws, "fs2_tsne_pca_init: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_tsne_pca_ws_bytes(n, dim), "fs2_tsne_pca_init: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const int N = (int)n, D = (int)dim;
  double* mean = (double*)ws;
  double* V = mean + D;
  double* Yd = V + 2 * D;
  double* cov = Yd + 2 * N;
  tsne_pca_mean_kernel<<<(D + TS_T - 1) / TS_T, TS_T, 0, st>>>(X, N, D, mean);
  const unsigned tiles = (unsigned)((D + 15) / 16);
  tsne_pca_cov_kernel<<<dim3(tiles, tiles), 256, 0, st>>>(X, N, D, mean, cov);
  tsne_pca_eig_kernel<<<1, TS_T, 0, st>>>(cov, D, V);
  tsne_pca_project_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, st>>>(X, N, D, mean, V, Yd);
  tsne_pca_scale_kernel<<<1, TS_T, 0, st>>>(Yd, N, Y0);
  return launch_status("fs2_tsne_pca_init");
}

int64_t fs2_tsne_affinities_ws_bytes(int64_t n) {
  if (n < 1) return 0;
  return (n * n + n) * 8;
}

int fs2_tsne_affinities(const float* X, int64_t n, int64_t dim, double perplexity, float* P,
                        double* beta, double* P64, void* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(tsne_n_ok(n), "fs2_tsne_affinities: n %lld (0..%d)", (long long)n, TS_NMAX);
  FS2_CHECK_ARG(dim >= 1 && dim <= TS_DMAX, "fs2_tsne_affinities: dim %lld (1..%d)",
                (long long)dim, TS_DMAX);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(perplexity > 0.0 && perplexity < (double)n,
                "fs2_tsne_affinities: perplexity %g must be positive and below n = %lld",
                perplexity, (long long)n);
  FS2_CHECK_ARG(X && P && ws, "fs2_tsne_affinities: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_tsne_affinities_ws_bytes(n),
                "fs2_tsne_affinities: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const int N = (int)n;
  double* C = (double*)ws;
  double* rs = C + n * n;
  const double target = log((double)(float)perplexity);  // sklearn passes the perplexity as a float
  tsne_cond_kernel<<<N, TS_T, 0, st>>>(X, N, (int)dim, target, C, beta);
  tsne_sym_rowsum_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, st>>>(C, N, rs);
  tsne_joint_kernel<<<N, TS_T, 0, st>>>(C, N, rs, P, P64);
  return launch_status("fs2_tsne_affinities");
}

int fs2_tsne_state_init(double* state, int64_t n, double perplexity, int64_t max_iter,
                        int64_t exploration_iter, int64_t n_iter_without_progress,
                        double early_exaggeration, double learning_rate, double min_grad_norm,
                        void* stream) {
  FS2_CHECK_ARG(n >= 1 && n <= TS_NMAX, "fs2_tsne_state_init: n %lld (1..%d)", (long long)n,
                TS_NMAX);
  FS2_CHECK_ARG(perplexity > 0.0 && perplexity < (double)n,
                "fs2_tsne_state_init: perplexity %g must be positive and below n = %lld",
                perplexity, (long long)n);
  FS2_CHECK_ARG(exploration_iter >= 1 && exploration_iter < (1 << 24) && max_iter >= 1 &&
                    max_iter < (1 << 24),
                "fs2_tsne_state_init: exploration_iter %lld, max_iter %lld (1 .. 2^24 - 1)",
                (long long)exploration_iter, (long long)max_iter);
  FS2_CHECK_ARG(n_iter_without_progress >= 0 && early_exaggeration >= 1.0 && learning_rate > 0.0 &&
                    min_grad_norm >= 0.0,
                "fs2_tsne_state_init: n_iter_without_progress %lld, early_exaggeration %g, "
                "learning_rate %g, min_grad_norm %g",
                (long long)n_iter_without_progress, early_exaggeration, learning_rate,
                min_grad_norm);
  FS2_CHECK_ARG(state, "fs2_tsne_state_init: missing state");
  tsne_state_init_kernel<<<1, 64, 0, as_stream(stream)>>>(
      state, (double)max_iter, (double)exploration_iter, (double)n_iter_without_progress,
      early_exaggeration, learning_rate, min_grad_norm);
  return launch_status("fs2_tsne_state_init");
}

int fs2_tsne_rowsum(const float* Y, int64_t n, const double* state, double* rowsum, void* stream) {
  FS2_CHECK_ARG(tsne_n_ok(n), "fs2_tsne_rowsum: n %lld (0..%d)", (long long)n, TS_NMAX);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(Y && rowsum, "fs2_tsne_rowsum: missing operand");
  const int N = (int)n;
  tsne_rowsum_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, as_stream(stream)>>>((const float2*)Y, N,
                                                                           state, rowsum);
  return launch_status("fs2_tsne_rowsum");
}

int fs2_tsne_update(const float* P, const float* Y, float* Y_out, float* update, float* gains,
                    int64_t n, int64_t iter, const double* state, const double* rowsum,
                    double* kl_rows, double* gn_rows, void* stream) {
  FS2_CHECK_ARG(tsne_n_ok(n), "fs2_tsne_update: n %lld (0..%d)", (long long)n, TS_NMAX);
  FS2_CHECK_ARG(iter >= 0 && iter < (1 << 24), "fs2_tsne_update: iter %lld", (long long)iter);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(P && Y && Y_out && update && gains && state && rowsum && kl_rows && gn_rows,
                "fs2_tsne_update: missing operand");
  FS2_CHECK_ARG(Y != Y_out, "fs2_tsne_update: Y_out must not be Y (other rows still read it)");
  const int N = (int)n;
  TsneStep a{P, (const float2*)Y, (float2*)Y_out, (float2*)update, (float2*)gains, state, rowsum,
             kl_rows, gn_rows, N, (int)iter, 0, 0, 0, 1.f, 0.f, 0.f};
  tsne_update_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, as_stream(stream)>>>(a);
  return launch_status("fs2_tsne_update");
}

int fs2_tsne_step(const float* P, const float* Y, float* Y_out, float* update, float* gains,
                  int64_t n, double exaggeration, double momentum, double learning_rate,
                  double* rowsum, double* kl_rows, double* gn_rows, void* stream) {
  FS2_CHECK_ARG(tsne_n_ok(n), "fs2_tsne_step: n %lld (0..%d)", (long long)n, TS_NMAX);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(P && Y && Y_out && update && gains && rowsum && kl_rows && gn_rows,
                "fs2_tsne_step: missing operand");
  FS2_CHECK_ARG(Y != Y_out, "fs2_tsne_step: Y_out must not be Y (other rows still read it)");
  const int N = (int)n;
  hipStream_t st = as_stream(stream);
  tsne_rowsum_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, st>>>((const float2*)Y, N, nullptr, rowsum);
  TsneStep a{P, (const float2*)Y, (float2*)Y_out, (float2*)update, (float2*)gains, nullptr, rowsum,
             kl_rows, gn_rows, N, 0, 1, 0, 0, (float)exaggeration, (float)momentum,
             (float)learning_rate};
  tsne_update_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, st>>>(a);
  return launch_status("fs2_tsne_step");
}

int fs2_tsne_kl(const float* P, const float* Y, int64_t n, double exaggeration, double* rowsum,
                double* kl_rows, double* kl, void* stream) {
  FS2_CHECK_ARG(tsne_n_ok(n), "fs2_tsne_kl: n %lld (0..%d)", (long long)n, TS_NMAX);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(P && Y && rowsum && kl_rows && kl, "fs2_tsne_kl: missing operand");
  const int N = (int)n;
  hipStream_t st = as_stream(stream);
  tsne_rowsum_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, st>>>((const float2*)Y, N, nullptr, rowsum);
  TsneStep a{P, (const float2*)Y, nullptr, nullptr, nullptr, nullptr, rowsum, kl_rows, nullptr,
             N, 0, 1, 0, 1, (float)exaggeration, 0.f, 0.f};
  tsne_update_kernel<<<(N + TS_W - 1) / TS_W, TS_T, 0, st>>>(a);
  tsne_sum_kernel<<<1, TS_T, 0, st>>>(kl_rows, N, kl);
  return launch_status("fs2_tsne_kl");
}

int fs2_tsne_control(double* state, int64_t n, int64_t iter, const double* kl_rows,
                     const double* gn_rows, void* stream) {
  FS2_CHECK_ARG(n >= 1 && n <= TS_NMAX, "fs2_tsne_control: n %lld (1..%d)", (long long)n, TS_NMAX);
  FS2_CHECK_ARG(iter >= 0 && iter < (1 << 24), "fs2_tsne_control: iter %lld", (long long)iter);
  FS2_CHECK_ARG(state && kl_rows && gn_rows, "fs2_tsne_control: missing operand");
  tsne_control_kernel<<<1, TS_T, 0, as_stream(stream)>>>(state, (int)n, (int)iter, kl_rows, gn_rows);
  return launch_status("fs2_tsne_control");
}

int fs2_tsne_finish(const float* Y, int64_t n, float* out, void* stream) {
  FS2_CHECK_ARG(tsne_n_ok(n), "fs2_tsne_finish: n %lld (0..%d)", (long long)n, TS_NMAX);
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(Y && out, "fs2_tsne_finish: missing operand");
  tsne_finish_kernel<<<1, TS_T, 0, as_stream(stream)>>>((const float2*)Y, (int)n, (float2*)out);
  return launch_status("fs2_tsne_finish");
}

}  // extern "C"
