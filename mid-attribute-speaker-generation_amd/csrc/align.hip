// Durations without an outside aligner: the alignment learning framework's hot
// path.  Four exports over a batch of (mel, phoneme) pairs with device lengths M = mel_lens[b],
// N = src_lens[b] that are never read back:
//
//   align_logprob       logp[t, s] = log_softmax_s(-temperature |q_t - k_s|^2) + prior(t, s)
//   align_logprob_bwd   dq, dk from dL/dlogp, the softmax recomputed
//   forward_sum         the CTC forward-sum loss over the target 1..N and its gradient
//   mas                 monotonic alignment search: the best monotonic path as durations
// and forward_sum_opt / mas_opt, the last two over a source sequence whose marked positions (the
// optional silences) may take no frame.
//
// The distance-softmax kernels own a tile of AL_TT frames with the tile's whole score rows in LDS
// (AL_TT x T_s floats), so a row is written once, normalised.  The two dynamic programmes run one
// workgroup per utterance and sweep the frames with the previous row in LDS, one barrier per
// frame; the next frame's operands are loaded before the barrier so that the global latency is
// not on the chain.  A batch runs side by side, nothing launches per frame, there are no atomics
// and every reduction has a fixed order: a row has the same bits wherever it sits in a batch.
#include <math.h>

#include "common.hpp"

namespace fs2 {

constexpr int AL_T = 256, AL_W = AL_T / 64;
constexpr int AL_TT = 8;                                           // frames per logprob tile
constexpr int AL_KC = 256;                                         // frames per dk partial
constexpr int AL_SI = (FS2_ALIGN_MAX_SRC + 1 + AL_T - 1) / AL_T;   // states per thread (0..N)
constexpr int AL_MI = FS2_ALIGN_MAX_SRC / AL_T;                    // MAS cells per thread

// a length outside 1..hi is clamped into it, as fs2_dtw does
FS2_DEV int al_len(int64_t v, int hi) { return (int)(v < 1 ? 1 : v > hi ? hi : v); }

// log of the beta-binomial pmf of s with n = N - 1, a = omega (t + 1), b = omega (M - t), in
// three parts: what depends on s alone, on t alone, and on both
FS2_DEV double bb_s(int s, int n) { return lgamma(n + 1.0) - lgamma(s + 1.0) - lgamma(n - s + 1.0); }
FS2_DEV double bb_t(double a, double b, int n) {
  return lgamma(a + b) - lgamma(a) - lgamma(b) - lgamma(n + a + b);
}
FS2_DEV double bb_ts(int s, int n, double a, double b) { return lgamma(s + a) + lgamma(n - s + b); }

FS2_DEV float al_dist(const float* __restrict__ qrow, const float* __restrict__ krow, int A) {
  float acc = 0.f;
  for (int a = 0; a < A; a += 4) {
    const f32x4 kv = ld4(krow + a), qv = ld4(qrow + a);
    const float d0 = qv.x - kv.x, d1 = qv.y - kv.y, d2 = qv.z - kv.z, d3 = qv.w - kv.w;
    acc = fmaf(d0, d0, acc);
    acc = fmaf(d1, d1, acc);
    acc = fmaf(d2, d2, acc);
    acc = fmaf(d3, d3, acc);
  }
  return acc;
}

// The tile's raw scores z[f][s] = -temperature |q_f - k_s|^2 into LDS (s < N), after its q rows.
FS2_DEV void al_scores(const float* __restrict__ q, const float* __restrict__ k, int t0, int nf,
                       int N, int A, float temperature, float* qs, float* z, int zp) {
  const int tid = threadIdx.x;
  for (int e = tid; e < nf * A; e += AL_T) qs[e] = q[(int64_t)t0 * A + e];
  __syncthreads();
  for (int s = tid; s < N; s += AL_T) {
    const float* krow = k + (int64_t)s * A;
    for (int f = 0; f < nf; ++f) z[f * zp + s] = -temperature * al_dist(qs + f * A, krow, A);
  }
  __syncthreads();
}

// max and log-sum-exp of z[0..N) over the wave (every lane gets both)
FS2_DEV void al_row_lse(const float* z, int N, float& mx, float& lse) {
  const int lane = threadIdx.x & 63;
  float m = -INFINITY;
  for (int s = lane; s < N; s += 64) m = fmaxf(m, z[s]);
  m = wave_max(m);
  float sum = 0.f;
  for (int s = lane; s < N; s += 64) sum += expf(z[s] - m);
  sum = wave_sum(sum);
  mx = m;
  lse = m + logf(sum);
}

// ---------------------------------------------------------------- align_logprob
// grid (ceil(T_m / AL_TT), B).  LDS: AL_TT x A floats of q, AL_TT x T_s of scores.
__global__ __launch_bounds__(AL_T) void align_logprob_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const int64_t* __restrict__ src_lens,
    const int64_t* __restrict__ mel_lens, int T_m, int T_s, int A, float temperature, float omega,
    float* __restrict__ logp) {
  extern __shared__ float al_lds[];
  __shared__ double ct[AL_TT];
  const int b = blockIdx.y, t0 = blockIdx.x * AL_TT, tid = threadIdx.x;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  const int nt = min(AL_TT, T_m - t0);        // frames of this tile
  const int nf = max(0, min(nt, M - t0));     // ... that are live
  float* out = logp + ((int64_t)b * T_m + t0) * T_s;
  if (nf == 0 || N == 0) {
    for (int e = tid; e < nt * T_s; e += AL_T) out[e] = 0.f;
    return;
  }
  float* qs = al_lds;
  float* z = al_lds + AL_TT * A;
  al_scores(q + (int64_t)b * T_m * A, k + (int64_t)b * T_s * A, t0, nf, N, A, temperature, qs, z,
            T_s);
  const bool prior = omega > 0.f;
  if (prior && tid < nf) {
    const double a = (double)omega * (t0 + tid + 1), bb = (double)omega * (M - t0 - tid);
    ct[tid] = bb_t(a, bb, N - 1);
  }
  // one wave per frame: the row's normaliser into lane registers, then the row in place
  const int wave = tid >> 6, lane = tid & 63;
  for (int f = wave; f < nf; f += AL_W) {
    float mx, lse;
    al_row_lse(z + f * T_s, N, mx, lse);
    for (int s = lane; s < N; s += 64) z[f * T_s + s] -= lse;
  }
  __syncthreads();
  // thread <-> column s, so that the s-only part of the prior is formed once per column
  for (int s = tid; s < T_s; s += AL_T) {
    const bool live = s < N;
    const double cs = prior && live ? bb_s(s, N - 1) : 0.0;
    for (int f = 0; f < nt; ++f) {
      float v = 0.f;
      if (live && f < nf) {
        v = z[f * T_s + s];
        if (prior) {
          const double a = (double)omega * (t0 + f + 1), bb = (double)omega * (M - t0 - f);
          v += (float)(cs + ct[f] + bb_ts(s, N - 1, a, bb));
        }
      }
      out[(int64_t)f * T_s + s] = v;
    }
  }
}

// ---------------------------------------------------------------- align_logprob_bwd
// Same tiles.  dz[t, s] = g[t, s] - softmax[t, s] sum_s g[t, s] goes to the workspace (live cells
// only) for the dk kernels; dq_t = -2 temperature sum_s dz[t, s] (q_t - k_s) is finished here.
__global__ __launch_bounds__(AL_T) void align_dq_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ g,
    const int64_t* __restrict__ src_lens, const int64_t* __restrict__ mel_lens, int T_m, int T_s,
    int A, float temperature, float* __restrict__ dz_ws, float* __restrict__ dq) {
  extern __shared__ float al_lds[];
  const int b = blockIdx.y, t0 = blockIdx.x * AL_TT, tid = threadIdx.x;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  const int nt = min(AL_TT, T_m - t0);
  const int nf = max(0, min(nt, M - t0));
  float* dq_out = dq + ((int64_t)b * T_m + t0) * A;
  if (nf == 0 || N == 0) {
    for (int e = tid; e < nt * A; e += AL_T) dq_out[e] = 0.f;
    return;
  }
  float* qs = al_lds;
  float* z = al_lds + AL_TT * A;
  const float* kb = k + (int64_t)b * T_s * A;
  al_scores(q + (int64_t)b * T_m * A, kb, t0, nf, N, A, temperature, qs, z, T_s);
  const float* gt = g + ((int64_t)b * T_m + t0) * T_s;
  float* dzt = dz_ws + ((int64_t)b * T_m + t0) * T_s;
  const int wave = tid >> 6, lane = tid & 63;
  for (int f = wave; f < nf; f += AL_W) {
    float mx, lse;
    al_row_lse(z + f * T_s, N, mx, lse);
    float G = 0.f;
    for (int s = lane; s < N; s += 64) G += gt[(int64_t)f * T_s + s];
    G = wave_sum(G);
    for (int s = lane; s < N; s += 64) {
      const float d = gt[(int64_t)f * T_s + s] - expf(z[f * T_s + s] - lse) * G;
      z[f * T_s + s] = d;
      dzt[(int64_t)f * T_s + s] = d;
    }
  }
  __syncthreads();
  for (int e = tid; e < nt * A; e += AL_T) {
    const int f = e / A, a = e % A;
    float acc = 0.f;
    if (f < nf) {
      const float qa = qs[e];
      for (int s = 0; s < N; ++s) acc = fmaf(z[f * T_s + s], qa - kb[(int64_t)s * A + a], acc);
      acc *= -2.f * temperature;
    }
    dq_out[e] = acc;
  }
}

// grid (ceil(T_s A / AL_T), ceil(T_m / AL_KC), B): the partial of dk[s, a] over the frames of
// chunk c, summed in frame order.  Chunks that start at or past M and columns s >= N write nothing.
__global__ __launch_bounds__(AL_T) void align_dk_partial_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ dz_ws,
    const int64_t* __restrict__ src_lens, const int64_t* __restrict__ mel_lens, int T_m, int T_s,
    int A, int chunks, float* __restrict__ part) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int e = blockIdx.x * AL_T + threadIdx.x;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  const int t0 = c * AL_KC, t1 = min(M, t0 + AL_KC);
  if (e >= N * A || t0 >= t1) return;
  const int s = e / A, a = e % A;
  const float ka = k[((int64_t)b * T_s + s) * A + a];
  const float* qb = q + (int64_t)b * T_m * A + a;
  const float* dz = dz_ws + (int64_t)b * T_m * T_s + s;
  float acc = 0.f;
#pragma unroll 4
  for (int t = t0; t < t1; ++t) acc = fmaf(dz[(int64_t)t * T_s], qb[(int64_t)t * A] - ka, acc);
  part[((int64_t)b * chunks + c) * T_s * A + e] = acc;
}

// dk[b, s, a] = 2 temperature x the live chunks' partials in chunk order; 0 at s >= N
__global__ __launch_bounds__(AL_T) void align_dk_final_kernel(
    const float* __restrict__ part, const int64_t* __restrict__ src_lens,
    const int64_t* __restrict__ mel_lens, int T_m, int T_s, int A, int chunks, float temperature,
    float* __restrict__ dk) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * AL_T + threadIdx.x;
  if (e >= T_s * A) return;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  float acc = 0.f;
  if (e < N * A) {
    const int live = (M + AL_KC - 1) / AL_KC;
    for (int c = 0; c < live; ++c) acc += part[((int64_t)b * chunks + c) * T_s * A + e];
    acc *= 2.f * temperature;
  }
  dk[(int64_t)b * T_s * A + e] = acc;
}

// ---------------------------------------------------------------- forward_sum
FS2_DEV double lse2(double a, double b) {
  const double m = fmax(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m));
}
FS2_DEV double lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// One workgroup per utterance.  The 2N + 1 CTC states are held as pairs: index s in 0..N owns the
// blank before label s (bl[s]; bl[N] is the last blank) and, for s < N, label s (la[s]).
//   alpha_t(bl s) = e_blank + lse(alpha_{t-1}(bl s), alpha_{t-1}(la s-1))
//   alpha_t(la s) = e_s     + lse(alpha_{t-1}(la s), alpha_{t-1}(bl s), alpha_{t-1}(la s-1))
// (distinct labels: the skip la s-1 -> la s is always open), beta the mirror image.  Only the
// label states' alpha goes to the workspace: the gradient needs no other.
__global__ __launch_bounds__(AL_T) void forward_sum_kernel(
    const float* __restrict__ logp, const int64_t* __restrict__ src_lens,
    const int64_t* __restrict__ mel_lens, const float* __restrict__ w, int T_m, int T_s,
    float* __restrict__ nll, float* __restrict__ grad, double* __restrict__ alpha_ws) {
  extern __shared__ double fs_lds[];
  __shared__ double ll_s;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  const float* lp = logp + (int64_t)b * T_m * T_s;
  float* gr = grad + (int64_t)b * T_m * T_s;
  double* aw = alpha_ws + (int64_t)b * T_m * T_s;
  const int P = T_s + 1;                  // pitch of a state row
  double* norm = fs_lds;                  // T_m: the log-sum-exp of frame t's N + 1 scores
  double* rows = fs_lds + T_m;            // 2 buffers x {la, bl} x P
  if (M < N) {  // no valid path
    for (int64_t e = tid; e < (int64_t)T_m * T_s; e += AL_T) gr[e] = 0.f;
    if (tid == 0) nll[b] = INFINITY;
    return;
  }
  // the frames' normalisers, a wave per frame
  for (int t = wave; t < M; t += AL_W) {
    const float* row = lp + (int64_t)t * T_s;
    float m = -1.f;  // the blank's score
    for (int s = lane; s < N; s += 64) m = fmaxf(m, row[s]);
    m = wave_max(m);
    double sum = 0.0;
    for (int s = lane; s < N; s += 64) sum += exp((double)row[s] - (double)m);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    sum += exp(-1.0 - (double)m);
    if (lane == 0) norm[t] = (double)m + log(sum);
  }
  __syncthreads();
  const double ninf = -INFINITY;
  float el[AL_SI], el_next[AL_SI];
  // ---- alpha, forward
#pragma unroll
  for (int i = 0; i < AL_SI; ++i) {
    const int s = tid + i * AL_T;
    el_next[i] = s < N ? lp[s] : 0.f;
  }
  for (int t = 0; t < M; ++t) {
    double* cur = rows + (t & 1) * 2 * P;
    const double* prv = rows + ((t + 1) & 1) * 2 * P;
    const double nt = norm[t], eb = -1.0 - nt;
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      el[i] = el_next[i];
      const int s = tid + i * AL_T;
      if (t + 1 < M && s < N) el_next[i] = lp[(int64_t)(t + 1) * T_s + s];
    }
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      const int s = tid + i * AL_T;
      if (s > N) continue;
      double ab, al = ninf;
      if (t == 0) {
        ab = s == 0 ? eb : ninf;
        if (s == 0) al = (double)el[i] - nt;
      } else {
        const double pl1 = s > 0 ? prv[s - 1] : ninf;  // la s-1
        const double pb = prv[P + s];
        ab = eb + lse2(pb, pl1);
        if (s < N) al = (double)el[i] - nt + lse3(prv[s], pb, pl1);
      }
      cur[P + s] = ab;
      if (s < N) {
        cur[s] = al;
        aw[(int64_t)t * T_s + s] = al;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double* last = rows + ((M - 1) & 1) * 2 * P;
    ll_s = lse2(last[P + N], last[N - 1]);
    nll[b] = (float)-ll_s;
  }
  __syncthreads();
  const double ll = ll_s;
  const double wb = (double)w[b];
  // ---- beta, backward, combined with alpha on the fly
  double a_next[AL_SI], a_cur[AL_SI];
#pragma unroll
  for (int i = 0; i < AL_SI; ++i) {
    const int s = tid + i * AL_T;
    el_next[i] = s < N ? lp[(int64_t)(M - 1) * T_s + s] : 0.f;
    a_next[i] = s < N ? aw[(int64_t)(M - 1) * T_s + s] : 0.0;
  }
  for (int t = M - 1; t >= 0; --t) {
    double* cur = rows + (t & 1) * 2 * P;
    const double* nxt = rows + ((t + 1) & 1) * 2 * P;
    const double nt = norm[t], eb = -1.0 - nt;
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      el[i] = el_next[i];
      a_cur[i] = a_next[i];
      const int s = tid + i * AL_T;
      if (t > 0 && s < N) {
        el_next[i] = lp[(int64_t)(t - 1) * T_s + s];
        a_next[i] = aw[(int64_t)(t - 1) * T_s + s];
      }
    }
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      const int s = tid + i * AL_T;
      if (s > N) continue;
      const double e = (double)el[i] - nt;
      double bb, bl = ninf;
      if (t == M - 1) {
        bb = s == N ? eb : ninf;
        if (s == N - 1) bl = e;
      } else {
        const double nb = nxt[P + s];
        bb = eb + (s < N ? lse2(nb, nxt[s]) : nb);
        if (s < N) bl = e + lse3(nxt[s], nxt[P + s + 1], s + 1 < N ? nxt[s + 1] : ninf);
      }
      cur[P + s] = bb;
      if (s < N) {
        cur[s] = bl;
        // d nll / d logp[t, s] = softmax_t(s) - occupancy_t(label s)
        const double occ = exp(a_cur[i] + bl - e - ll);
        gr[(int64_t)t * T_s + s] = (float)(wb * (exp(e) - occ));
      }
    }
    __syncthreads();
  }
  // dead cells
  for (int64_t e = tid; e < (int64_t)T_m * T_s; e += AL_T) {
    const int t = (int)(e / T_s), s = (int)(e % T_s);
    if (t >= M || s >= N) gr[e] = 0.f;
  }
}

// ---------------------------------------------------------------- mas
// One workgroup per utterance: V[t, s] = logp[t, s] + max(V[t-1, s-1], V[t-1, s]) in fp32 with
// two LDS rows, the diagonal on a tie; one step byte per cell (1 = diagonal) to the workspace; then
// one lane walks back from (M-1, N-1) counting frames per phoneme into LDS.
__global__ __launch_bounds__(AL_T) void mas_kernel(
    const float* __restrict__ logp, const int64_t* __restrict__ src_lens,
    const int64_t* __restrict__ mel_lens, int T_m, int T_s, int64_t* __restrict__ durations,
    unsigned char* __restrict__ steps_ws) {
  __shared__ float V[2][FS2_ALIGN_MAX_SRC];
  __shared__ int dur[FS2_ALIGN_MAX_SRC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  int64_t* out = durations + (int64_t)b * T_s;
  if (M < N) {  // no monotonic path covers every phoneme
    for (int s = tid; s < T_s; s += AL_T) out[s] = 0;
    return;
  }
  const float* lp = logp + (int64_t)b * T_m * T_s;
  unsigned char* st = steps_ws + (int64_t)b * T_m * T_s;
  float x[AL_MI], x_next[AL_MI];
#pragma unroll
  for (int i = 0; i < AL_MI; ++i) {
    const int s = tid + i * AL_T;
    x_next[i] = s < N ? lp[s] : 0.f;
    if (s < T_s) dur[s] = 0;
  }
  for (int t = 0; t < M; ++t) {
    float* cur = V[t & 1];
    const float* prv = V[(t + 1) & 1];
#pragma unroll
    for (int i = 0; i < AL_MI; ++i) {
      x[i] = x_next[i];
      const int s = tid + i * AL_T;
      if (t + 1 < M && s < N) x_next[i] = lp[(int64_t)(t + 1) * T_s + s];
    }
#pragma unroll
    for (int i = 0; i < AL_MI; ++i) {
      const int s = tid + i * AL_T;
      if (s >= N) continue;
      if (t == 0) {
        cur[s] = s == 0 ? x[i] : -INFINITY;
      } else {
        const float dg = s > 0 ? prv[s - 1] : -INFINITY, up = prv[s];
        const bool diag = dg >= up;
        cur[s] = __fadd_rn(x[i], diag ? dg : up);
        st[(int64_t)t * T_s + s] = diag ? 1 : 0;
      }
    }
    __syncthreads();  // row t complete (and, in global memory, its step bytes for this block)
  }
  if (tid == 0) {
    int s = N - 1;
    for (int t = M - 1; t >= 0; --t) {
      ++dur[s];
      if (t > 0 && s > 0 && st[(int64_t)t * T_s + s]) --s;
    }
  }
  __syncthreads();
  for (int s = tid; s < T_s; s += AL_T) out[s] = s < N ? (int64_t)dur[s] : 0;
}

// ---------------------------------------------------------------- optional positions
// A position s < N with optional[s] != 0 may take no frame (an optional silence).  The row's mask
// is staged once into LDS as bytes, 0 at s >= N, so that the sweeps read it beside the state rows.
FS2_DEV void al_stage_mask(const unsigned char* __restrict__ optional, int N, int T_s,
                           unsigned char* op) {
  for (int s = threadIdx.x; s < T_s; s += AL_T) op[s] = s < N && optional[s] ? 1 : 0;
  __syncthreads();
}

// the extra terms come last: an exp of -inf adds an exact 0, so with none of them open these are
// the bits of lse2 / lse3
FS2_DEV double lse4(double a, double b, double c, double d) {
  const double m = fmax(fmax(a, fmax(b, c)), d);
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m) + exp(d - m));
}
FS2_DEV double lse5(double a, double b, double c, double d, double e) {
  const double m = fmax(fmax(fmax(a, fmax(b, c)), d), e);
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m) + exp(d - m) + exp(e - m));
}
FS2_DEV double lse2x(double a, double b, double c) {  // lse2 and one extra term
  const double m = fmax(fmax(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// forward_sum_kernel with skippable labels.  Omitting a marked label u omits the pair (la[u],
// bl[u+1]), so a labelling keeps exactly one state path.  Beside the edges of forward_sum_kernel:
//   into la[s], optional[s-1]:  from bl[s-1] and, s >= 2, from la[s-2]
//   optional[0], N >= 2:        la[1] is an initial state too
//   optional[N-1], N >= 2:      la[N-2] and bl[N-1] are final states too
// beta the mirror image: bl[s] -> la[s+1] when optional[s], la[s] -> la[s+2] when optional[s+1].
// Whether a path exists is known after the alpha pass (ll = -inf: nll = +inf, gradient 0).
__global__ __launch_bounds__(AL_T) void forward_sum_opt_kernel(
    const float* __restrict__ logp, const int64_t* __restrict__ src_lens,
    const int64_t* __restrict__ mel_lens, const unsigned char* __restrict__ optional,
    const float* __restrict__ w, int T_m, int T_s, float* __restrict__ nll,
    float* __restrict__ grad, double* __restrict__ alpha_ws) {
  extern __shared__ double fs_lds[];
  __shared__ double ll_s;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  const float* lp = logp + (int64_t)b * T_m * T_s;
  float* gr = grad + (int64_t)b * T_m * T_s;
  double* aw = alpha_ws + (int64_t)b * T_m * T_s;
  const int P = T_s + 1;                  // pitch of a state row
  double* norm = fs_lds;                  // T_m: the log-sum-exp of frame t's N + 1 scores
  double* rows = fs_lds + T_m;            // 2 buffers x {la, bl} x P
  unsigned char* op = (unsigned char*)(rows + 4 * P);  // T_s: the row's mask
  al_stage_mask(optional + (int64_t)b * T_s, N, T_s, op);
  // the frames' normalisers, a wave per frame
  for (int t = wave; t < M; t += AL_W) {
    const float* row = lp + (int64_t)t * T_s;
    float m = -1.f;  // the blank's score
    for (int s = lane; s < N; s += 64) m = fmaxf(m, row[s]);
    m = wave_max(m);
    double sum = 0.0;
    for (int s = lane; s < N; s += 64) sum += exp((double)row[s] - (double)m);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    sum += exp(-1.0 - (double)m);
    if (lane == 0) norm[t] = (double)m + log(sum);
  }
  __syncthreads();
  const double ninf = -INFINITY;
  const bool head = N >= 2 && op[0], tail = N >= 2 && op[N - 1];
  float el[AL_SI], el_next[AL_SI];
  bool o_prev[AL_SI], o_self[AL_SI], o_next[AL_SI];  // optional[s-1], [s], [s+1]
#pragma unroll
  for (int i = 0; i < AL_SI; ++i) {
    const int s = tid + i * AL_T;
    o_prev[i] = s >= 1 && s <= N && op[s - 1];
    o_self[i] = s < N && op[s];
    o_next[i] = s + 1 < N && op[s + 1];
  }
  // ---- alpha, forward
#pragma unroll
  for (int i = 0; i < AL_SI; ++i) {
    const int s = tid + i * AL_T;
    el_next[i] = s < N ? lp[s] : 0.f;
  }
  for (int t = 0; t < M; ++t) {
    double* cur = rows + (t & 1) * 2 * P;
    const double* prv = rows + ((t + 1) & 1) * 2 * P;
    const double nt = norm[t], eb = -1.0 - nt;
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      el[i] = el_next[i];
      const int s = tid + i * AL_T;
      if (t + 1 < M && s < N) el_next[i] = lp[(int64_t)(t + 1) * T_s + s];
    }
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      const int s = tid + i * AL_T;
      if (s > N) continue;
      double ab, al = ninf;
      if (t == 0) {
        ab = s == 0 ? eb : ninf;
        if (s == 0 || (s == 1 && head)) al = (double)el[i] - nt;
      } else {
        const double pl1 = s > 0 ? prv[s - 1] : ninf;  // la s-1
        const double pb = prv[P + s];
        ab = eb + lse2(pb, pl1);
        if (s < N) {
          if (o_prev[i]) {
            const double pb1 = prv[P + s - 1];               // bl s-1
            const double pl2 = s >= 2 ? prv[s - 2] : ninf;   // la s-2
            al = (double)el[i] - nt + lse5(prv[s], pb, pl1, pb1, pl2);
          } else {
            al = (double)el[i] - nt + lse3(prv[s], pb, pl1);
          }
        }
      }
      cur[P + s] = ab;
      if (s < N) {
        cur[s] = al;
        aw[(int64_t)t * T_s + s] = al;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double* last = rows + ((M - 1) & 1) * 2 * P;
    ll_s = tail ? lse4(last[P + N], last[N - 1], last[N - 2], last[P + N - 1])
                : lse2(last[P + N], last[N - 1]);
    nll[b] = (float)-ll_s;
  }
  __syncthreads();
  const double ll = ll_s;
  if (ll == ninf) {  // no valid path
    for (int64_t e = tid; e < (int64_t)T_m * T_s; e += AL_T) gr[e] = 0.f;
    return;
  }
  const double wb = (double)w[b];
  // ---- beta, backward, combined with alpha on the fly
  double a_next[AL_SI], a_cur[AL_SI];
#pragma unroll
  for (int i = 0; i < AL_SI; ++i) {
    const int s = tid + i * AL_T;
    el_next[i] = s < N ? lp[(int64_t)(M - 1) * T_s + s] : 0.f;
    a_next[i] = s < N ? aw[(int64_t)(M - 1) * T_s + s] : 0.0;
  }
  for (int t = M - 1; t >= 0; --t) {
    double* cur = rows + (t & 1) * 2 * P;
    const double* nxt = rows + ((t + 1) & 1) * 2 * P;
    const double nt = norm[t], eb = -1.0 - nt;
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      el[i] = el_next[i];
      a_cur[i] = a_next[i];
      const int s = tid + i * AL_T;
      if (t > 0 && s < N) {
        el_next[i] = lp[(int64_t)(t - 1) * T_s + s];
        a_next[i] = aw[(int64_t)(t - 1) * T_s + s];
      }
    }
#pragma unroll
    for (int i = 0; i < AL_SI; ++i) {
      const int s = tid + i * AL_T;
      if (s > N) continue;
      const double e = (double)el[i] - nt;
      double bb, bl = ninf;
      if (t == M - 1) {
        bb = s == N || (s == N - 1 && tail) ? eb : ninf;
        if (s == N - 1 || (s == N - 2 && tail)) bl = e;
      } else {
        const double nb = nxt[P + s];
        if (s < N) {
          // bl s -> la s+1 over an omitted label s
          bb = eb + (o_self[i] && s + 1 < N ? lse2x(nb, nxt[s], nxt[s + 1]) : lse2(nb, nxt[s]));
          const double nl1 = s + 1 < N ? nxt[s + 1] : ninf;
          // la s -> la s+2 over an omitted label s+1
          bl = e + (o_next[i] && s + 2 < N ? lse4(nxt[s], nxt[P + s + 1], nl1, nxt[s + 2])
                                            : lse3(nxt[s], nxt[P + s + 1], nl1));
        } else {
          bb = eb + nb;
        }
      }
      cur[P + s] = bb;
      if (s < N) {
        cur[s] = bl;
        // d nll / d logp[t, s] = softmax_t(s) - occupancy_t(label s)
        const double occ = exp(a_cur[i] + bl - e - ll);
        gr[(int64_t)t * T_s + s] = (float)(wb * (exp(e) - occ));
      }
    }
    __syncthreads();
  }
  // dead cells
  for (int64_t e = tid; e < (int64_t)T_m * T_s; e += AL_T) {
    const int t = (int)(e / T_s), s = (int)(e % T_s);
    if (t >= M || s >= N) gr[e] = 0.f;
  }
}

// mas_kernel with skippable positions: V[t-1, s-2] is a third candidate where optional[s-1], taken
// only when strictly greater than the winner of the other two; V[0, 1] is a start where
// optional[0], and (M-1, N-2) the end where optional[N-1] and it is strictly greater.  The step
// byte is what the trace-back subtracts from s: 0 stay, 1 diagonal, 2 skip.  A row whose end cell
// is -inf has no path: all zeros.
__global__ __launch_bounds__(AL_T) void mas_opt_kernel(
    const float* __restrict__ logp, const int64_t* __restrict__ src_lens,
    const int64_t* __restrict__ mel_lens, const unsigned char* __restrict__ optional, int T_m,
    int T_s, int64_t* __restrict__ durations, unsigned char* __restrict__ steps_ws) {
  __shared__ float V[2][FS2_ALIGN_MAX_SRC];
  __shared__ int dur[FS2_ALIGN_MAX_SRC];
  __shared__ unsigned char op[FS2_ALIGN_MAX_SRC];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = al_len(src_lens[b], T_s), M = al_len(mel_lens[b], T_m);
  int64_t* out = durations + (int64_t)b * T_s;
  const float* lp = logp + (int64_t)b * T_m * T_s;
  unsigned char* st = steps_ws + (int64_t)b * T_m * T_s;
  al_stage_mask(optional + (int64_t)b * T_s, N, T_s, op);
  const bool head = N >= 2 && op[0], tail = N >= 2 && op[N - 1];
  float x[AL_MI], x_next[AL_MI];
  bool o_prev[AL_MI];  // optional[s-1], s >= 2
#pragma unroll
  for (int i = 0; i < AL_MI; ++i) {
    const int s = tid + i * AL_T;
    x_next[i] = s < N ? lp[s] : 0.f;
    o_prev[i] = s >= 2 && s < N && op[s - 1];
    if (s < T_s) dur[s] = 0;
  }
  for (int t = 0; t < M; ++t) {
    float* cur = V[t & 1];
    const float* prv = V[(t + 1) & 1];
#pragma unroll
    for (int i = 0; i < AL_MI; ++i) {
      x[i] = x_next[i];
      const int s = tid + i * AL_T;
      if (t + 1 < M && s < N) x_next[i] = lp[(int64_t)(t + 1) * T_s + s];
    }
#pragma unroll
    for (int i = 0; i < AL_MI; ++i) {
      const int s = tid + i * AL_T;
      if (s >= N) continue;
      if (t == 0) {
        cur[s] = s == 0 || (s == 1 && head) ? x[i] : -INFINITY;
      } else {
        const float dg = s > 0 ? prv[s - 1] : -INFINITY, up = prv[s];
        const bool diag = dg >= up;
        float best = diag ? dg : up;
        int step = diag ? 1 : 0;
        if (o_prev[i]) {
          const float sk = prv[s - 2];
          if (sk > best) {
            best = sk;
            step = 2;
          }
        }
        cur[s] = __fadd_rn(x[i], best);
        st[(int64_t)t * T_s + s] = (unsigned char)step;
      }
    }
    __syncthreads();  // row t complete (and, in global memory, its step bytes for this block)
  }
  if (tid == 0) {
    const float* last = V[(M - 1) & 1];
    int s = N - 1;
    if (tail && last[N - 2] > last[N - 1]) s = N - 2;
    if (last[s] != -INFINITY) {
      for (int t = M - 1; t >= 0; --t) {
        ++dur[s];
        if (t > 0) s = max(0, s - (int)st[(int64_t)t * T_s + s]);
      }
    }
  }
  __syncthreads();
  for (int s = tid; s < T_s; s += AL_T) out[s] = s < N ? (int64_t)dur[s] : 0;
}

static bool al_dims_ok(int64_t t_m, int64_t t_s) {
  return t_m >= 1 && t_m <= FS2_ALIGN_MAX_MEL && t_s >= 1 && t_s <= FS2_ALIGN_MAX_SRC;
}
static bool al_width_ok(int64_t a) { return a >= 8 && a <= FS2_ALIGN_MAX_WIDTH && a % 8 == 0; }
static bool al_batch_ok(int64_t b) { return b >= 0 && b <= 65535; }
static int64_t al_chunks(int64_t t_m) { return (t_m + AL_KC - 1) / AL_KC; }
static size_t al_tile_lds(int64_t t_s, int64_t a) { return (size_t)AL_TT * (a + t_s) * sizeof(float); }

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_align_logprob(const float* q, const float* k, const int64_t* src_lens,
                      const int64_t* mel_lens, int64_t batch, int64_t t_m, int64_t t_s, int64_t a,
                      float temperature, float omega, float* logp, void* stream) {
  FS2_CHECK_ARG(al_dims_ok(t_m, t_s), "fs2_align_logprob: T_m %lld (1..%d), T_s %lld (1..%d)",
                (long long)t_m, FS2_ALIGN_MAX_MEL, (long long)t_s, FS2_ALIGN_MAX_SRC);
  FS2_CHECK_ARG(al_width_ok(a), "fs2_align_logprob: width %lld (8..%d, a multiple of 8)",
                (long long)a, FS2_ALIGN_MAX_WIDTH);
  FS2_CHECK_ARG(al_batch_ok(batch), "fs2_align_logprob: batch %lld (0..65535)", (long long)batch);
  FS2_CHECK_ARG(temperature > 0.f && temperature < INFINITY,
                "fs2_align_logprob: temperature %g", (double)temperature);
  FS2_CHECK_ARG(omega == omega && omega < INFINITY, "fs2_align_logprob: omega %g", (double)omega);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(q && k && src_lens && mel_lens && logp, "fs2_align_logprob: missing operand");
  const dim3 grid((unsigned)((t_m + AL_TT - 1) / AL_TT), (unsigned)batch);
  align_logprob_kernel<<<grid, AL_T, al_tile_lds(t_s, a), as_stream(stream)>>>(
      q, k, src_lens, mel_lens, (int)t_m, (int)t_s, (int)a, temperature, omega, logp);
  return launch_status("fs2_align_logprob");
}

int64_t fs2_align_logprob_bwd_ws_bytes(int64_t batch, int64_t t_m, int64_t t_s, int64_t a) {
  if (batch < 1 || !al_batch_ok(batch) || !al_dims_ok(t_m, t_s) || !al_width_ok(a)) return 0;
  return batch * (t_m * t_s + al_chunks(t_m) * t_s * a) * 4;
}

int fs2_align_logprob_bwd(const float* q, const float* k, const float* g, const int64_t* src_lens,
                          const int64_t* mel_lens, int64_t batch, int64_t t_m, int64_t t_s,
                          int64_t a, float temperature, float* dq, float* dk, void* ws,
                          int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(al_dims_ok(t_m, t_s), "fs2_align_logprob_bwd: T_m %lld (1..%d), T_s %lld (1..%d)",
                (long long)t_m, FS2_ALIGN_MAX_MEL, (long long)t_s, FS2_ALIGN_MAX_SRC);
  FS2_CHECK_ARG(al_width_ok(a), "fs2_align_logprob_bwd: width %lld (8..%d, a multiple of 8)",
                (long long)a, FS2_ALIGN_MAX_WIDTH);
  FS2_CHECK_ARG(al_batch_ok(batch), "fs2_align_logprob_bwd: batch %lld (0..65535)",
                (long long)batch);
  FS2_CHECK_ARG(temperature > 0.f && temperature < INFINITY,
                "fs2_align_logprob_bwd: temperature %g", (double)temperature);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(q && k && g && src_lens && mel_lens && dq && dk && ws,
                "fs2_align_logprob_bwd: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_align_logprob_bwd_ws_bytes(batch, t_m, t_s, a),
                "fs2_align_logprob_bwd: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_align_logprob_bwd_ws_bytes(batch, t_m, t_s, a));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  float* dz = (float*)ws;
  float* part = dz + batch * t_m * t_s;
  const int chunks = (int)al_chunks(t_m);
  const dim3 grid((unsigned)((t_m + AL_TT - 1) / AL_TT), (unsigned)batch);
  align_dq_kernel<<<grid, AL_T, al_tile_lds(t_s, a), st>>>(
      q, k, g, src_lens, mel_lens, (int)t_m, (int)t_s, (int)a, temperature, dz, dq);
  int rc = launch_status("fs2_align_logprob_bwd (dq)");
  if (rc != FS2_OK) return rc;
  const unsigned cols = (unsigned)((t_s * a + AL_T - 1) / AL_T);
  align_dk_partial_kernel<<<dim3(cols, (unsigned)chunks, (unsigned)batch), AL_T, 0, st>>>(
      q, k, dz, src_lens, mel_lens, (int)t_m, (int)t_s, (int)a, chunks, part);
  rc = launch_status("fs2_align_logprob_bwd (dk partials)");
  if (rc != FS2_OK) return rc;
  align_dk_final_kernel<<<dim3(cols, (unsigned)batch), AL_T, 0, st>>>(
      part, src_lens, mel_lens, (int)t_m, (int)t_s, (int)a, chunks, temperature, dk);
  return launch_status("fs2_align_logprob_bwd (dk)");
}

int64_t fs2_forward_sum_ws_bytes(int64_t batch, int64_t t_m, int64_t t_s) {
  if (batch < 1 || !al_batch_ok(batch) || !al_dims_ok(t_m, t_s)) return 0;
  return batch * t_m * t_s * 8;
}

int fs2_forward_sum(const float* logp, const int64_t* src_lens, const int64_t* mel_lens,
                    const float* w, int64_t batch, int64_t t_m, int64_t t_s, float* nll,
                    float* grad, void* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(al_dims_ok(t_m, t_s), "fs2_forward_sum: T_m %lld (1..%d), T_s %lld (1..%d)",
                (long long)t_m, FS2_ALIGN_MAX_MEL, (long long)t_s, FS2_ALIGN_MAX_SRC);
  FS2_CHECK_ARG(al_batch_ok(batch), "fs2_forward_sum: batch %lld (0..65535)", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(logp && src_lens && mel_lens && w && nll && grad && ws,
                "fs2_forward_sum: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_forward_sum_ws_bytes(batch, t_m, t_s),
                "fs2_forward_sum: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_forward_sum_ws_bytes(batch, t_m, t_s));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const size_t lds = (size_t)(t_m + 4 * (t_s + 1)) * sizeof(double);
  forward_sum_kernel<<<(unsigned)batch, AL_T, lds, st>>>(logp, src_lens, mel_lens, w, (int)t_m,
                                                         (int)t_s, nll, grad, (double*)ws);
  return launch_status("fs2_forward_sum");
}

int64_t fs2_mas_ws_bytes(int64_t batch, int64_t t_m, int64_t t_s) {
  if (batch < 1 || !al_batch_ok(batch) || !al_dims_ok(t_m, t_s)) return 0;
  return batch * t_m * t_s;
}

int fs2_mas(const float* logp, const int64_t* src_lens, const int64_t* mel_lens, int64_t batch,
            int64_t t_m, int64_t t_s, int64_t* durations, void* ws, int64_t ws_bytes,
            void* stream) {
  FS2_CHECK_ARG(al_dims_ok(t_m, t_s), "fs2_mas: T_m %lld (1..%d), T_s %lld (1..%d)",
                (long long)t_m, FS2_ALIGN_MAX_MEL, (long long)t_s, FS2_ALIGN_MAX_SRC);
  FS2_CHECK_ARG(al_batch_ok(batch), "fs2_mas: batch %lld (0..65535)", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(logp && src_lens && mel_lens && durations && ws, "fs2_mas: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_mas_ws_bytes(batch, t_m, t_s),
                "fs2_mas: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_mas_ws_bytes(batch, t_m, t_s));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  mas_kernel<<<(unsigned)batch, AL_T, 0, st>>>(logp, src_lens, mel_lens, (int)t_m, (int)t_s,
                                               durations, (unsigned char*)ws);
  return launch_status("fs2_mas");
}

int fs2_forward_sum_opt(const float* logp, const int64_t* src_lens, const int64_t* mel_lens,
                        const unsigned char* optional, const float* w, int64_t batch, int64_t t_m,
                        int64_t t_s, float* nll, float* grad, void* ws, int64_t ws_bytes,
                        void* stream) {
  FS2_CHECK_ARG(al_dims_ok(t_m, t_s), "fs2_forward_sum_opt: T_m %lld (1..%d), T_s %lld (1..%d)",
                (long long)t_m, FS2_ALIGN_MAX_MEL, (long long)t_s, FS2_ALIGN_MAX_SRC);
  FS2_CHECK_ARG(al_batch_ok(batch), "fs2_forward_sum_opt: batch %lld (0..65535)",
                (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(logp && src_lens && mel_lens && optional && w && nll && grad && ws,
                "fs2_forward_sum_opt: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_forward_sum_ws_bytes(batch, t_m, t_s),
                "fs2_forward_sum_opt: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_forward_sum_ws_bytes(batch, t_m, t_s));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const size_t lds = (size_t)(t_m + 4 * (t_s + 1)) * sizeof(double) + (size_t)t_s;
  forward_sum_opt_kernel<<<(unsigned)batch, AL_T, lds, st>>>(
      logp, src_lens, mel_lens, optional, w, (int)t_m, (int)t_s, nll, grad, (double*)ws);
  return launch_status("fs2_forward_sum_opt");
}

int fs2_mas_opt(const float* logp, const int64_t* src_lens, const int64_t* mel_lens,
                const unsigned char* optional, int64_t batch, int64_t t_m, int64_t t_s,
                int64_t* durations, void* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(al_dims_ok(t_m, t_s), "fs2_mas_opt: T_m %lld (1..%d), T_s %lld (1..%d)",
                (long long)t_m, FS2_ALIGN_MAX_MEL, (long long)t_s, FS2_ALIGN_MAX_SRC);
  FS2_CHECK_ARG(al_batch_ok(batch), "fs2_mas_opt: batch %lld (0..65535)", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(logp && src_lens && mel_lens && optional && durations && ws,
                "fs2_mas_opt: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_mas_ws_bytes(batch, t_m, t_s),
                "fs2_mas_opt: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_mas_ws_bytes(batch, t_m, t_s));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  mas_opt_kernel<<<(unsigned)batch, AL_T, 0, st>>>(logp, src_lens, mel_lens, optional, (int)t_m,
                                                   (int)t_s, durations, (unsigned char*)ws);
  return launch_status("fs2_mas_opt");
}

}  // extern "C"
