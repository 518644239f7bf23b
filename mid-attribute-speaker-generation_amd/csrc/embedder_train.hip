// Training the GE2E speaker encoder (train_speech_embedder.py): what the --use_clf path of
// train.py never needs -- the head's weight gradients, the GE2E softmax loss for M > 1
// utterances per speaker (utils.py:77-90, 126-135, speech_embedder_net.py:173-181) and its
// 'contrast' alternative (utils.py:106-124), and Adam with torch.optim.Adam's coupled L2 weight
// decay.  The LSTM weight gradients are in lstm_wgrad.hip.  fp32 throughout; every reduction
// runs in a fixed order (no atomics).
#include <math.h>

#include "common.hpp"

namespace fs2 {

// ---------------------------------------------------------------- head weight gradients
// Phase 1 (one wave per row) repeats clf_head_kernel's forward and backward (lstm.hip; same
// arithmetic, same regenerated dropout masks) and leaves the row's vectors in the workspace:
//   [dp | e | dz0 | a0 | dz1 | a1 | dlogit], HW_ROW floats per row.
// Phase 2 gives every output element one thread that adds the rows in row order.
constexpr int HW_D = 256, HW_P = 64, HW_ROW = 6 * HW_P + 4;

struct HeadWgrad {
  const float* x;
  int64_t ldx;
  const float* wpt;
  const float* bp;
  const float* w0;
  const float* w0t;
  const float* b0;
  const float* w1;
  const float* w1t;
  const float* b1;
  const float* w2;
  const float* b2;
  int N;
  float p_drop;
  const uint64_t* seed;
  uint64_t site;
  const float* demb;
  const float* dlogit;
  float* ws;  // (N, HW_ROW)
};

__global__ __launch_bounds__(256) void head_wgrad_rows(HeadWgrad a) {
  __shared__ float xs[4][HW_D];
  __shared__ float vs[4][HW_P];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= a.N) return;  // whole wave
  const uint64_t seed = a.seed ? *a.seed : 0ull;
  for (int k = lane; k < HW_D; k += 64) xs[wave][k] = a.x[(int64_t)n * a.ldx + k];
  __builtin_amdgcn_wave_barrier();
  float p = a.bp[lane];
  for (int k = 0; k < HW_D; ++k) p = fmaf(a.wpt[k * HW_P + lane], xs[wave][k], p);
  const float nrm = sqrtf(wave_sum(p * p));
  const float e = p / nrm;
  const uint64_t el = (uint64_t)n * (2 * HW_P);
  const float m0 = a.p_drop > 0.f ? dropout1(seed, a.site, el + lane, a.p_drop) : 1.f;
  const float m1 = a.p_drop > 0.f ? dropout1(seed, a.site, el + HW_P + lane, a.p_drop) : 1.f;
  vs[wave][lane] = e;
  __builtin_amdgcn_wave_barrier();
  float z0 = a.b0[lane];
  for (int k = 0; k < HW_P; ++k) z0 = fmaf(a.w0t[k * HW_P + lane], vs[wave][k], z0);
  const float a0 = fmaxf(z0 * m0, 0.f);
  __builtin_amdgcn_wave_barrier();
  vs[wave][lane] = a0;
  __builtin_amdgcn_wave_barrier();
  float z1 = a.b1[lane];
  for (int k = 0; k < HW_P; ++k) z1 = fmaf(a.w1t[k * HW_P + lane], vs[wave][k], z1);
  const float a1 = fmaxf(z1 * m1, 0.f);
  // ---- backward
  const float dl = a.dlogit ? a.dlogit[n] : 0.f;
  const float dz1 = (a1 > 0.f ? dl * a.w2[lane] : 0.f) * m1;
  __builtin_amdgcn_wave_barrier();
  vs[wave][lane] = dz1;
  __builtin_amdgcn_wave_barrier();
  float da0 = 0.f;
  for (int o = 0; o < HW_P; ++o) da0 = fmaf(a.w1[o * HW_P + lane], vs[wave][o], da0);
  const float dz0 = (a0 > 0.f ? da0 : 0.f) * m0;
  __builtin_amdgcn_wave_barrier();
  vs[wave][lane] = dz0;
  __builtin_amdgcn_wave_barrier();
  float de = a.demb ? a.demb[(int64_t)n * HW_P + lane] : 0.f;
  for (int o = 0; o < HW_P; ++o) de = fmaf(a.w0[o * HW_P + lane], vs[wave][o], de);
  const float ed = wave_sum(e * de);
  const float dp = (de - e * ed) / nrm;
  float* r = a.ws + (int64_t)n * HW_ROW;
  r[lane] = dp;
  r[HW_P + lane] = e;
  r[2 * HW_P + lane] = dz0;
  r[3 * HW_P + lane] = a0;
  r[4 * HW_P + lane] = dz1;
  r[5 * HW_P + lane] = a1;
  if (lane == 0) r[6 * HW_P] = dl;
}

struct HeadWgradOut {
  const float* x;
  int64_t ldx;
  const float* ws;
  int N, beta;
  float* dwp;  // (P, D)
  float* dbp;  // (P)
  float* dw0;  // (P, P)
  float* db0;
  float* dw1;
  float* db1;
  float* dw2;  // (1, P)
  float* db2;  // (1)
};

constexpr int HW_OUTS = HW_P * HW_D + HW_P + 2 * (HW_P * HW_P + HW_P) + HW_P + 1;

__global__ __launch_bounds__(256) void head_wgrad_sum(HeadWgradOut a) {
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= HW_OUTS) return;
  // left factor at ws column ca (stride HW_ROW); right factor: x, a ws column, or 1
  float* out;
  int ca, cb = -1;
  const float* xr = nullptr;
  if (idx < HW_P * HW_D) {
    out = a.dwp + idx, ca = idx / HW_D, xr = a.x + idx % HW_D;
  } else if ((idx -= HW_P * HW_D) < HW_P) {
    out = a.dbp + idx, ca = idx;
  } else if ((idx -= HW_P) < HW_P * HW_P) {
    out = a.dw0 + idx, ca = 2 * HW_P + idx / HW_P, cb = HW_P + idx % HW_P;
  } else if ((idx -= HW_P * HW_P) < HW_P) {
    out = a.db0 + idx, ca = 2 * HW_P + idx;
  } else if ((idx -= HW_P) < HW_P * HW_P) {
    out = a.dw1 + idx, ca = 4 * HW_P + idx / HW_P, cb = 3 * HW_P + idx % HW_P;
  } else if ((idx -= HW_P * HW_P) < HW_P) {
    out = a.db1 + idx, ca = 4 * HW_P + idx;
  } else if ((idx -= HW_P) < HW_P) {
    out = a.dw2 + idx, ca = 6 * HW_P, cb = 5 * HW_P + idx;
  } else {
    out = a.db2, ca = 6 * HW_P;
  }
  float s = 0.f;
  for (int n = 0; n < a.N; ++n) {
    const float* r = a.ws + (int64_t)n * HW_ROW;
    const float rhs = xr ? xr[(int64_t)n * a.ldx] : cb >= 0 ? r[cb] : 1.f;
    s = fmaf(r[ca], rhs, s);
  }
  *out = a.beta ? *out + s : s;
}

// ---------------------------------------------------------------- GE2E softmax loss
// One block, 16 waves.  e (N speakers, M utterances, D), S_jik = w cos(e_ji, c_k) + b with
// c_k the mean over M, and for k = j the exclude-self centroid (sum_j - e_ji) / (M - 1);
// cos clamps each norm at 1e-8 (F.cosine_similarity);
//   loss = sum_ji log(sum_k exp S_jik + 1e-6) - S_jij.
// Phases (block barriers between them; the workspace is global memory):
//   A  centroid sums, means and norms;
//   B  one wave per utterance row, rows dealt round-robin: the row's loss, its direct gradient,
//      the coefficients of its gradient into every centroid, and the gradient into its
//      exclude-self centroid; per-wave loss / dw / db partials, added in wave order;
//   C  each centroid's gradient (rows in row order), then each embedding's total gradient.
// db's row term sum_k p_k - 1 is -1e-6 / (sum_k exp S + 1e-6) in closed form; it is taken in
// that form (the subtraction would leave only fp32 rounding of 1).
constexpr int GE_WAVES = 16, GE_DMAX = 256, GE_DS = GE_DMAX / 64;

struct Ge2e {
  const float* e;
  int N, M, D;
  const float* w;
  const float* b;
  const float* g;  // upstream gradient of the loss (NULL = 1)
  float* loss;
  float* demb;
  float* dw;
  float* db;
  float* ws;
};

FS2_DEV float ge_clamp(float n) { return fmaxf(n, 1e-8f); }

__global__ __launch_bounds__(64 * GE_WAVES) void ge2e_softmax_kernel(Ge2e a) {
  __shared__ float red[GE_WAVES][3];
  const int N = a.N, M = a.M, D = a.D, NM = N * M;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* csum = a.ws;            // (N, D)
  float* cmean = csum + N * D;   // (N, D)
  float* cnrm = cmean + N * D;   // (N)
  float* coefA = cnrm + N;       // (NM, N)
  float* coefB = coefA + NM * N; // (NM, N)
  float* dcx = coefB + NM * N;   // (NM, D)
  float* dc = dcx + NM * D;      // (N, D)
  const bool grads = a.demb != nullptr;
  const float w = a.w[0], b = a.b[0], g = a.g ? a.g[0] : 1.f;
  const float inv_m1 = 1.f / (float)(M - 1);

  for (int idx = tid; idx < N * D; idx += blockDim.x) {
    const int k = idx / D, d = idx % D;
    float s = 0.f;
    for (int i = 0; i < M; ++i) s += a.e[((int64_t)k * M + i) * D + d];
    csum[idx] = s;
    cmean[idx] = s / (float)M;
  }
  __threadfence_block();
  __syncthreads();
  for (int k = tid; k < N; k += blockDim.x) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(cmean[k * D + d], cmean[k * D + d], s);
    cnrm[k] = sqrtf(s);
  }
  __threadfence_block();
  __syncthreads();

  float w_loss = 0.f, w_dw = 0.f, w_db = 0.f;  // this wave's partials (same in every lane)
  for (int row = wave; row < NM; row += GE_WAVES) {
    const int j = row / M;
    float ev[GE_DS], cx[GE_DS], gd[GE_DS];
    float na2 = 0.f, nx2 = 0.f;
#pragma unroll
    for (int s = 0; s < GE_DS; ++s) {
      const int d = lane + 64 * s;
      ev[s] = d < D ? a.e[(int64_t)row * D + d] : 0.f;
      cx[s] = d < D ? (csum[j * D + d] - ev[s]) * inv_m1 : 0.f;
      gd[s] = 0.f;
      na2 = fmaf(ev[s], ev[s], na2);
      nx2 = fmaf(cx[s], cx[s], nx2);
    }
    const float na_raw = sqrtf(wave_sum(na2)), nx_raw = sqrtf(wave_sum(nx2));
    const float na = ge_clamp(na_raw);
    // pass 1: the row's denominator; pass 2: its loss and gradients
    float den = 0.f, s_own = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
      const float rden = 1.f / (den + 1e-6f);
      for (int k = 0; k < N; ++k) {
        const bool own = k == j;
        float dot = 0.f;
#pragma unroll
        for (int s = 0; s < GE_DS; ++s) {
          const int d = lane + 64 * s;
          const float bv = own ? cx[s] : d < D ? cmean[k * D + d] : 0.f;
          dot = fmaf(ev[s], bv, dot);
        }
        dot = wave_sum(dot);
        const float nb_raw = own ? nx_raw : cnrm[k], nb = ge_clamp(nb_raw);
        const float sim = dot / (na * nb);
        const float S = w * sim + b, ex = expf(S);
        if (pass == 0) {
          den += ex;
          if (own) s_own = S;
          continue;
        }
        const float dS = ex * rden - (own ? 1.f : 0.f);
        w_dw = fmaf(dS, sim, w_dw);
        if (!grads) continue;
        const float dsim = g * w * dS;
        const float cA = dsim / (na * nb);
        const float cBa = na_raw > 1e-8f ? dsim * dot / (na * na * na * nb) : 0.f;
        const float cBb = nb_raw > 1e-8f ? dsim * dot / (na * nb * nb * nb) : 0.f;
#pragma unroll
        for (int s = 0; s < GE_DS; ++s) {
          const int d = lane + 64 * s;
          const float bv = own ? cx[s] : d < D ? cmean[k * D + d] : 0.f;
          gd[s] += cA * bv - cBa * ev[s];
          if (own && d < D) dcx[(int64_t)row * D + d] = cA * ev[s] - cBb * cx[s];
        }
        if (lane == 0) {
          coefA[row * N + k] = own ? 0.f : cA;
          coefB[row * N + k] = own ? 0.f : cBb;
        }
      }
    }
    w_loss += logf(den + 1e-6f) - s_own;
    w_db -= 1e-6f / (den + 1e-6f);
    if (grads) {
#pragma unroll
      for (int s = 0; s < GE_DS; ++s) {
        const int d = lane + 64 * s;
        if (d < D) a.demb[(int64_t)row * D + d] = gd[s];
      }
    }
  }
  if (lane == 0) red[wave][0] = w_loss, red[wave][1] = w_dw, red[wave][2] = w_db;
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    float l = 0.f, dw = 0.f, db = 0.f;
    for (int v = 0; v < GE_WAVES; ++v) l += red[v][0], dw += red[v][1], db += red[v][2];
    if (a.loss) a.loss[0] = l;
    if (a.dw) a.dw[0] = g * dw;
    if (a.db) a.db[0] = g * db;
  }
  if (!grads) return;
  // c_k = csum_k / M: every embedding of speaker k receives dc_k / M
  for (int idx = tid; idx < N * D; idx += blockDim.x) {
    const int k = idx / D, d = idx % D;
    float sa = 0.f, sb = 0.f;
    for (int row = 0; row < NM; ++row) {
      sa = fmaf(coefA[row * N + k], a.e[(int64_t)row * D + d], sa);
      sb += coefB[row * N + k];
    }
    dc[idx] = (sa - sb * cmean[idx]) / (float)M;
  }
  __threadfence_block();
  __syncthreads();
  for (int idx = tid; idx < NM * D; idx += blockDim.x) {
    const int row = idx / D, d = idx % D, j = row / M, i = row % M;
    float sx = 0.f;
    for (int i2 = 0; i2 < M; ++i2)
      if (i2 != i) sx += dcx[((int64_t)j * M + i2) * D + d];
    a.demb[idx] += dc[j * D + d] + sx * inv_m1;
  }
}

// ---------------------------------------------------------------- GE2E contrast loss
// hp.model.loss == 'contrast' (utils.py:106-124) on the S of the softmax kernel above:
//   sig = 1 / (1 + exp(-S)),   loss = sum_ji (1 - sig(S_jij)) + max_k sig~_jik,
// sig~_jik = sig(S_jik) for k != j and sig~_jij = 0 -- the reference zeroes the own-speaker entry
// in place, so it takes part in the maximum with value 0 and carries no gradient.  The scan over
// k keeps the first strict maximum: on equal values the lowest k wins, as torch.max(dim=2).
//   dL/dS_jij = -sig (1 - sig),  dL/dS_jik* = +sig (1 - sig) at the winner k*,  nothing else.
// 1 - sig is formed as 1 / (1 + exp(S)): the subtraction would keep 6e-8 absolute of a value
// that is 7e-3 at S = 5.
// Same block shape and phases as ge2e_softmax_kernel; a row has at most two centroid terms, so
// phase B leaves per row the winner's index and its two coefficients (no (NM, N) tables) and
// the gradient into its exclude-self centroid; phase C gathers each centroid's rows in row order.
__global__ __launch_bounds__(64 * GE_WAVES) void ge2e_contrast_kernel(Ge2e a) {
  __shared__ float red[GE_WAVES][3];
  const int N = a.N, M = a.M, D = a.D, NM = N * M;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* csum = a.ws;                             // (N, D)
  float* cmean = csum + N * D;                    // (N, D)
  float* cnrm = cmean + N * D;                    // (N)
  int* kwin = reinterpret_cast<int*>(cnrm + N);   // (NM) winning k, -1: no gradient
  float* coefA = cnrm + N + NM;                   // (NM)
  float* coefB = coefA + NM;                      // (NM)
  float* dcx = coefB + NM;                        // (NM, D)
  float* dc = dcx + NM * D;                       // (N, D)
  const bool grads = a.demb != nullptr;
  const float w = a.w[0], b = a.b[0], g = a.g ? a.g[0] : 1.f;
  const float inv_m1 = 1.f / (float)(M - 1);

  for (int idx = tid; idx < N * D; idx += blockDim.x) {
    const int k = idx / D, d = idx % D;
    float s = 0.f;
    for (int i = 0; i < M; ++i) s += a.e[((int64_t)k * M + i) * D + d];
    csum[idx] = s;
    cmean[idx] = s / (float)M;
  }
  __threadfence_block();
  __syncthreads();
  for (int k = tid; k < N; k += blockDim.x) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(cmean[k * D + d], cmean[k * D + d], s);
    cnrm[k] = sqrtf(s);
  }
  __threadfence_block();
  __syncthreads();

  float w_loss = 0.f, w_dw = 0.f, w_db = 0.f;  // this wave's partials (same in every lane)
  for (int row = wave; row < NM; row += GE_WAVES) {
    const int j = row / M;
    float ev[GE_DS], cx[GE_DS];
    float na2 = 0.f, nx2 = 0.f, dot_own = 0.f;
#pragma unroll
    for (int s = 0; s < GE_DS; ++s) {
      const int d = lane + 64 * s;
      ev[s] = d < D ? a.e[(int64_t)row * D + d] : 0.f;
      cx[s] = d < D ? (csum[j * D + d] - ev[s]) * inv_m1 : 0.f;
      na2 = fmaf(ev[s], ev[s], na2);
      nx2 = fmaf(cx[s], cx[s], nx2);
      dot_own = fmaf(ev[s], cx[s], dot_own);
    }
    const float na_raw = sqrtf(wave_sum(na2)), nx_raw = sqrtf(wave_sum(nx2));
    const float na = ge_clamp(na_raw), nx = ge_clamp(nx_raw);
    dot_own = wave_sum(dot_own);
    const float sim_own = dot_own / (na * nx), s_own = w * sim_own + b;
    // the hardest negative: first strict maximum of sig~ over k, the own entry standing as 0
    float best = -1.f, best_dot = 0.f, best_sim = 0.f, best_s = 0.f;
    int kb = -1;
    for (int k = 0; k < N; ++k) {
      float val = 0.f, dot = 0.f, sim = 0.f, S = 0.f;
      if (k != j) {
#pragma unroll
        for (int s = 0; s < GE_DS; ++s) {
          const int d = lane + 64 * s;
          dot = fmaf(ev[s], d < D ? cmean[k * D + d] : 0.f, dot);
        }
        dot = wave_sum(dot);
        sim = dot / (na * ge_clamp(cnrm[k]));
        S = w * sim + b;
        val = 1.f / (1.f + expf(-S));
      }
      // a NaN candidate wins and then stays (the first one), as in torch.max
      if (val > best || (val != val && best == best))
        best = val, kb = k, best_dot = dot, best_sim = sim, best_s = S;
    }
    const bool neg = kb >= 0 && kb != j;  // a negative won: it carries the second term's gradient
    const float oms_own = 1.f / (1.f + expf(s_own));
    const float dS_own = -(1.f - oms_own) * oms_own;
    const float dS_neg = neg ? best / (1.f + expf(best_s)) : 0.f;
    w_loss += oms_own + best;
    w_dw = fmaf(dS_own, sim_own, w_dw);
    w_dw = fmaf(dS_neg, best_sim, w_dw);
    w_db += dS_own + dS_neg;
    if (!grads) continue;
    // own term: cos(e, x) into e and into the exclude-self centroid x
    const float ds_o = g * w * dS_own;
    const float oA = ds_o / (na * nx);
    const float oBa = na_raw > 1e-8f ? ds_o * dot_own / (na * na * na * nx) : 0.f;
    const float oBb = nx_raw > 1e-8f ? ds_o * dot_own / (na * nx * nx * nx) : 0.f;
    // winner's term: cos(e, c_k*) into e; its coefficients into c_k* are left for phase C
    const int kc = neg ? kb : 0;
    const float nb_raw = cnrm[kc], nb = ge_clamp(nb_raw);
    const float ds_n = g * w * dS_neg;
    const float nA = ds_n / (na * nb);
    const float nBa = na_raw > 1e-8f ? ds_n * best_dot / (na * na * na * nb) : 0.f;
    const float nBb = nb_raw > 1e-8f ? ds_n * best_dot / (na * nb * nb * nb) : 0.f;
#pragma unroll
    for (int s = 0; s < GE_DS; ++s) {
      const int d = lane + 64 * s;
      if (d < D) {
        float gd = oA * cx[s] - oBa * ev[s];
        if (neg) gd += nA * cmean[kc * D + d] - nBa * ev[s];
        a.demb[(int64_t)row * D + d] = gd;
        dcx[(int64_t)row * D + d] = oA * ev[s] - oBb * cx[s];
      }
    }
    if (lane == 0) {
      kwin[row] = neg ? kb : -1;
      coefA[row] = nA;
      coefB[row] = nBb;
    }
  }
  if (lane == 0) red[wave][0] = w_loss, red[wave][1] = w_dw, red[wave][2] = w_db;
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    float l = 0.f, dw = 0.f, db = 0.f;
    for (int v = 0; v < GE_WAVES; ++v) l += red[v][0], dw += red[v][1], db += red[v][2];
    if (a.loss) a.loss[0] = l;
    if (a.dw) a.dw[0] = g * dw;
    if (a.db) a.db[0] = g * db;
  }
  if (!grads) return;
  // c_k = csum_k / M: every embedding of speaker k receives dc_k / M
  for (int idx = tid; idx < N * D; idx += blockDim.x) {
    const int k = idx / D, d = idx % D;
    float sa = 0.f, sb = 0.f;
    for (int row = 0; row < NM; ++row) {
      if (kwin[row] != k) continue;
      sa = fmaf(coefA[row], a.e[(int64_t)row * D + d], sa);
      sb += coefB[row];
    }
    dc[idx] = (sa - sb * cmean[idx]) / (float)M;
  }
  __threadfence_block();
  __syncthreads();
  for (int idx = tid; idx < NM * D; idx += blockDim.x) {
    const int row = idx / D, d = idx % D, j = row / M, i = row % M;
    float sx = 0.f;
    for (int i2 = 0; i2 < M; ++i2)
      if (i2 != i) sx += dcx[((int64_t)j * M + i2) * D + d];
    a.demb[idx] += dc[j * D + d] + sx * inv_m1;
  }
}

// ---------------------------------------------------------------- Adam, coupled L2 decay
// torch.optim.Adam(weight_decay = wd): g <- clip_coef g + wd p, then Adam.  The step counter
// lives on the device; with a gate (device float) of 0 the call is torch's "no parameter has a
// gradient": nothing moves, the counter included.  hyper = [1 - b1^t, sqrt(1 - b2^t), on].
// omb1 / omb2 are 1 - beta formed in double on the host and rounded once, as torch rounds its
// scalars: 1.f - 0.999f is 0.00099998713, 1.3e-5 short of 0.001f, and v would carry that.
__global__ void adam_l2_tick(int64_t* step, float* hyper, double b1, double b2, const float* gate) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool on = !gate || gate[0] != 0.f;
  const int64_t t = on ? ++step[0] : step[0];
  hyper[0] = (float)(1.0 - pow(b1, (double)t));
  hyper[1] = (float)sqrt(1.0 - pow(b2, (double)t));
  hyper[2] = on ? 1.f : 0.f;
}

__global__ void adam_l2_kernel(float* __restrict__ p, const float* __restrict__ g,
                               float* __restrict__ m, float* __restrict__ v, int64_t n,
                               const float* __restrict__ norm_coef, float lr, float omb1,
                               float b2, float omb2, float eps, float wd,
                               const float* __restrict__ hyper) {
  if (hyper[2] == 0.f) return;
  const float coef = norm_coef ? norm_coef[1] : 1.f;
  const float step = lr / hyper[0], bc2s = hyper[1];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float pv = p[i], gv = fmaf(wd, pv, g[i] * coef);
    const float mv = m[i] + (gv - m[i]) * omb1;
    const float vv = b2 * v[i] + omb2 * gv * gv;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv - step * mv / (sqrtf(vv) / bc2s + eps);
  }
}

__global__ void gate_lt_kernel(const float* x, float thr, float* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = x[0] < thr ? 1.f : 0.f;
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int64_t fs2_clf_head_wgrad_ws_bytes(int64_t n) { return (n < 1 ? 1 : n) * HW_ROW * 4; }

int fs2_clf_head_wgrad(const float* x, int64_t ldx, int64_t n, const float* wp, const float* wpt,
                       const float* bp, const float* w0, const float* w0t, const float* b0,
                       const float* w1, const float* w1t, const float* b1, const float* w2,
                       const float* b2, float p_drop, const uint64_t* seed, uint64_t site,
                       const float* demb, const float* dlogit, float* dwp, float* dbp, float* dw0,
                       float* db0, float* dw1, float* db1, float* dw2, float* db2, int beta,
                       float* ws, int64_t ws_bytes, void* stream) {
  (void)wp;
  FS2_CHECK_ARG(x && wpt && bp && w0 && w0t && b0 && w1 && w1t && b1 && w2 && b2,
                "fs2_clf_head_wgrad: missing weight operand");
  FS2_CHECK_ARG(dwp && dbp && dw0 && db0 && dw1 && db1 && dw2 && db2 && ws,
                "fs2_clf_head_wgrad: missing output");
  FS2_CHECK_ARG(p_drop <= 0.f || seed, "fs2_clf_head_wgrad: dropout needs a seed");
  FS2_CHECK_ARG(beta == 0 || beta == 1, "fs2_clf_head_wgrad: beta %d (0 or 1)", beta);
  FS2_CHECK_ARG(n >= 0 && n < (1ll << 24), "fs2_clf_head_wgrad: n %lld", (long long)n);
  FS2_CHECK_ARG(ws_bytes >= fs2_clf_head_wgrad_ws_bytes(n),
                "fs2_clf_head_wgrad: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  if (n > 0) {
    HeadWgrad a{x, ldx, wpt, bp, w0, w0t, b0, w1, w1t, b1, w2, b2, (int)n, p_drop, seed, site,
                demb, dlogit, ws};
    head_wgrad_rows<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(a);
  }
  HeadWgradOut o{x, ldx, ws, (int)n, beta, dwp, dbp, dw0, db0, dw1, db1, dw2, db2};
  head_wgrad_sum<<<(HW_OUTS + 255) / 256, 256, 0, st>>>(o);
  return launch_status("fs2_clf_head_wgrad");
}

int64_t fs2_ge2e_softmax_ws_bytes(int64_t n_spk, int64_t m_utt, int64_t dim) {
  if (n_spk < 1 || m_utt < 1 || dim < 1) return 0;
  const int64_t nm = n_spk * m_utt;
  return (3 * n_spk * dim + n_spk + 2 * nm * n_spk + nm * dim) * 4;
}

int fs2_ge2e_softmax(const float* emb, int64_t n_spk, int64_t m_utt, int64_t dim, const float* w,
                     const float* b, const float* g, float* loss, float* demb, float* dw,
                     float* db, float* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(n_spk >= 1 && m_utt >= 2 && dim >= 1 && dim <= GE_DMAX &&
                    n_spk * m_utt * (n_spk > dim ? n_spk : dim) < (1ll << 28),
                "fs2_ge2e_softmax: n_spk %lld (>= 1), m_utt %lld (>= 2), dim %lld (1..%d)",
                (long long)n_spk, (long long)m_utt, (long long)dim, GE_DMAX);
  FS2_CHECK_ARG(emb && w && b && ws, "fs2_ge2e_softmax: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_ge2e_softmax_ws_bytes(n_spk, m_utt, dim),
                "fs2_ge2e_softmax: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  Ge2e a{emb, (int)n_spk, (int)m_utt, (int)dim, w, b, g, loss, demb, dw, db, ws};
  ge2e_softmax_kernel<<<1, 64 * GE_WAVES, 0, st>>>(a);
  return launch_status("fs2_ge2e_softmax");
}

// fs2_ge2e_softmax's limits, the products taken one at a time (no int64 overflow on any input)
static bool ge2e_contrast_shape_ok(int64_t n_spk, int64_t m_utt, int64_t dim) {
  const int64_t lim = 1ll << 28;
  if (n_spk < 1 || n_spk >= lim || m_utt < 2 || m_utt >= lim || dim < 1 || dim > GE_DMAX)
    return false;
  const int64_t nm = n_spk * m_utt;
  return nm < lim && nm * (n_spk > dim ? n_spk : dim) < lim;
}

// centroid sums, means and gradients (3 N D), centroid norms (N), per row the winner's index and
// two coefficients (3 NM) and the gradient into its exclude-self centroid (NM D); 0 for a shape
// the entry rejects
int64_t fs2_ge2e_contrast_ws_bytes(int64_t n_spk, int64_t m_utt, int64_t dim) {
  if (!ge2e_contrast_shape_ok(n_spk, m_utt, dim)) return 0;
  const int64_t nm = n_spk * m_utt;
  return (3 * n_spk * dim + n_spk + 3 * nm + nm * dim) * 4;
}

int fs2_ge2e_contrast(const float* emb, int64_t n_spk, int64_t m_utt, int64_t dim, const float* w,
                      const float* b, const float* g, float* loss, float* demb, float* dw,
                      float* db, float* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(ge2e_contrast_shape_ok(n_spk, m_utt, dim),
                "fs2_ge2e_contrast: n_spk %lld (>= 1), m_utt %lld (>= 2), dim %lld (1..%d)",
                (long long)n_spk, (long long)m_utt, (long long)dim, GE_DMAX);
  FS2_CHECK_ARG(emb && w && b && ws, "fs2_ge2e_contrast: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_ge2e_contrast_ws_bytes(n_spk, m_utt, dim),
                "fs2_ge2e_contrast: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  Ge2e a{emb, (int)n_spk, (int)m_utt, (int)dim, w, b, g, loss, demb, dw, db, ws};
  ge2e_contrast_kernel<<<1, 64 * GE_WAVES, 0, st>>>(a);
  return launch_status("fs2_ge2e_contrast");
}

int fs2_adam_l2_step(float* p, const float* g, float* m, float* v, int64_t n,
                     const float* norm_coef, float lr, double beta1, double beta2, float eps,
                     float weight_decay, int64_t* step, float* hyper, const float* gate,
                     void* stream) {
  FS2_CHECK_ARG(p && g && m && v && step && hyper, "fs2_adam_l2_step: missing operand");
  FS2_CHECK_ARG(n >= 0 && weight_decay >= 0.f, "fs2_adam_l2_step: n %lld, weight_decay %g",
                (long long)n, (double)weight_decay);
  hipStream_t st = as_stream(stream);
  adam_l2_tick<<<1, 64, 0, st>>>(step, hyper, beta1, beta2, gate);
  if (n > 0) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    adam_l2_kernel<<<(unsigned)blocks, 256, 0, st>>>(p, g, m, v, n, norm_coef, lr,
                                                     (float)(1.0 - beta1), (float)beta2,
                                                     (float)(1.0 - beta2), eps, weight_decay,
                                                     hyper);
  }
  return launch_status("fs2_adam_l2_step");
}

int fs2_gate_lt(const float* x, float threshold, float* out, void* stream) {
  FS2_CHECK_ARG(x && out, "fs2_gate_lt: missing operand");
  gate_lt_kernel<<<1, 64, 0, as_stream(stream)>>>(x, threshold, out);
  return launch_status("fs2_gate_lt");
}

}  // extern "C"
