// Objective synthesis metrics: MFCCs of the natural-log mel, batched dynamic time
// warping with its path, and per-pair records along the path (MCD, F0 error, voicing error).
//
// DTW is a wavefront recurrence: cell (i, j) needs (i-1, j-1), (i-1, j) and (i, j-1), so the
// cells of one anti-diagonal d = i + j are independent and need only the diagonals d - 1 and
// d - 2.  One workgroup owns a pair and sweeps the diagonals with those three in LDS, indexed
// by the position along the SHORTER of the two padded sequences (3 x min(T1max, T2max) x 8 B,
// 48 KiB at 2048); the fp64 matrix is never stored.  What the backtrack needs is which
// predecessor won: one byte per cell, laid out diagonal-major so that a wave's 64 bytes are
// contiguous.  The features are (T, K) row-major, which along a diagonal is a stride of K floats
// between lanes (measured: the sweep then runs at the rate of its uncoalesced loads), so the
// block first copies its pair into the workspace feature-major (K, T): lane u then reads
// x[k][u] and y[k][d - u], consecutive addresses across the wave.  All arithmetic is fp64 with
// one add per cell, no atomics and a fixed order, so a run is bitwise repeatable and a CPU
// oracle can match it exactly.
#include <math.h>

#include "common.hpp"

namespace fs2 {

constexpr int MT_T = 256, MT_W = MT_T / 64;
constexpr int MF_TILE = 64;  // frames per MFCC block

// ---------------------------------------------------------------- MFCC
// One block per (64-frame tile, utterance): the tile goes to LDS (frame-major, pitch n_mels + 1),
// thread t then forms outputs (frame, k) = t, t + 256, ... with k fastest, so the table reads
// (dct[m][k], k consecutive) and the stores are coalesced and the tile reads are broadcasts.
__global__ __launch_bounds__(MT_T) void mfcc_kernel(const float* __restrict__ x,
                                                    const int64_t* __restrict__ n_frames,
                                                    int n_mels, int F, int rows,
                                                    const float* __restrict__ dct, int n_coef,
                                                    float* __restrict__ out) {
  __shared__ float xs[MF_TILE * (FS2_MFCC_MAX_MELS + 1)];
  const int b = blockIdx.y, f0 = blockIdx.x * MF_TILE, tid = threadIdx.x;
  const int pitch = n_mels + 1;
  int live = n_frames ? (int)(n_frames[b] < 0 ? 0 : n_frames[b] > F ? F : n_frames[b]) : F;
  const int nt = min(MF_TILE, F - f0);            // frames of this tile
  const int nl = max(0, min(nt, live - f0));      // ... that are live
  if (rows) {  // (B * F, n_mels): m fastest
    const float* src = x + ((int64_t)b * F + f0) * n_mels;
    for (int e = tid; e < nl * n_mels; e += MT_T) xs[(e / n_mels) * pitch + e % n_mels] = src[e];
  } else {     // (B, n_mels, F): frames fastest
    const float* src = x + (int64_t)b * n_mels * F + f0;
    for (int e = tid; e < nl * n_mels; e += MT_T) {
      const int m = e / nl, f = e % nl;
      xs[f * pitch + m] = src[(int64_t)m * F + f];
    }
  }
  __syncthreads();
  float* dst = out + ((int64_t)b * F + f0) * n_coef;
  for (int e = tid; e < nt * n_coef; e += MT_T) {
    const int f = e / n_coef, k = e % n_coef;
    float acc = 0.f;
    if (f < nl) {
      const float* row = xs + f * pitch;
      for (int m = 0; m < n_mels; ++m) acc = fmaf(row[m], dct[m * n_coef + k], acc);
    }
    dst[e] = acc;
  }
}

// ---------------------------------------------------------------- DTW
struct DtwArgs {
  const float* a;
  const float* b;
  const int64_t* la;
  const int64_t* lb;
  int t1_max, t2_max, k;
  double* cost;
  int* path;
  int* path_len;
  unsigned char* steps;  // per pair: (t1_max + t2_max - 1) diagonals x inner bytes
  int2* rev;             // per pair: t1_max + t2_max - 1 entries, the path from its end
  float* feat;           // per pair: (k, t1_max) then (k, t2_max), the features transposed
  int64_t steps_pair;    // bytes of one pair's step codes
};

FS2_DEV int clamp_len(int64_t v, int hi) { return (int)(v < 1 ? 1 : v > hi ? hi : v); }

// Trace the path of pair p from (la-1, lb-1) back to (0, 0) (one lane, a chain of dependent
// byte reads), then every thread of the block copies it out front to back.
FS2_DEV void dtw_backtrack(const DtwArgs& g, int p, int la, int lb, bool swap, int inner,
                           int* n_shared) {
  const int L = g.t1_max + g.t2_max - 1;
  const unsigned char* steps = g.steps + (int64_t)p * g.steps_pair;
  int2* rev = g.rev + (int64_t)p * L;
  if (threadIdx.x == 0) {
    int i = la - 1, j = lb - 1, n = 0;
    while (true) {
      rev[n++] = make_int2(i, j);
      if (i == 0 && j == 0) break;
      const int s = steps[(int64_t)(i + j) * inner + (swap ? j : i)];
      // the first row and column have one way back whatever the byte says
      if (i == 0) --j;
      else if (j == 0) --i;
      else if (s == 0) --i, --j;
      else if (s == 1) --i;
      else --j;
    }
    *n_shared = n;
    g.path_len[p] = n;
  }
  __syncthreads();  // rev was written by this block: visible after the barrier
  const int n = *n_shared;
  int2* path = reinterpret_cast<int2*>(g.path) + (int64_t)p * L;
  for (int e = threadIdx.x; e < n; e += blockDim.x) path[e] = rev[n - 1 - e];
}

// SWAP = false: lanes run along a (u = i, v = j); true: along b (u = j, v = i).  The host picks
// the shorter padded length for u.  The path is traced in the same launch: a second launch for
// it measured the same (3.416 against 3.415 ms for 16 pairs of 800 x 800).
template <bool SWAP>
__global__ __launch_bounds__(MT_T) void dtw_kernel(DtwArgs g) {
  extern __shared__ double diag[];  // 3 x inner
  __shared__ int n_shared;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int la = clamp_len(g.la[p], g.t1_max), lb = clamp_len(g.lb[p], g.t2_max);
  const int inner = SWAP ? g.t2_max : g.t1_max;
  const int lx = SWAP ? lb : la, ly = SWAP ? la : lb, K = g.k;
  const int outer = SWAP ? g.t1_max : g.t2_max;
  const float* X = (SWAP ? g.b : g.a) + (int64_t)p * inner * K;
  const float* Y = (SWAP ? g.a : g.b) + (int64_t)p * outer * K;
  unsigned char* steps = g.steps + (int64_t)p * g.steps_pair;
  const double inf = INFINITY;
  // the live rows, feature-major (padding rows are not read, their columns stay unwritten)
  float* Xt = g.feat + (int64_t)p * (g.t1_max + g.t2_max) * K;
  float* Yt = Xt + (int64_t)inner * K;
  for (int e = tid; e < lx * K; e += MT_T) Xt[(int64_t)(e % K) * inner + e / K] = X[e];
  for (int e = tid; e < ly * K; e += MT_T) Yt[(int64_t)(e % K) * outer + e / K] = Y[e];
  __syncthreads();  // written by this block: visible to it after the barrier
  for (int d = 0; d <= lx + ly - 2; ++d) {
    double* cur = diag + (d % 3) * inner;
    const double* p1 = diag + ((d + 2) % 3) * inner;  // diagonal d - 1
    const double* p2 = diag + ((d + 1) % 3) * inner;  // diagonal d - 2
    const int lo = max(0, d - (ly - 1)), hi = min(d, lx - 1);
    for (int u = lo + tid; u <= hi; u += MT_T) {
      const int v = d - u;
      const float* xc = Xt + u;
      const float* yc = Yt + v;
      double s = 0.0;
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const double t = (double)xc[(int64_t)k * inner] - (double)yc[(int64_t)k * outer];
        s = fma(t, t, s);
      }
      const double c = sqrt(s);
      // predecessors in (i, j) terms: diagonal, (i-1, j), (i, j-1); the first minimum wins
      const double dg = u > 0 && v > 0 ? p2[u - 1] : inf;
      const double um = u > 0 ? p1[u - 1] : inf;  // (u-1, v)
      const double vm = v > 0 ? p1[u] : inf;      // (u, v-1)
      const double up = SWAP ? vm : um, left = SWAP ? um : vm;
      double m = dg;
      int step = 0;
      if (up < m) m = up, step = 1;
      if (left < m) m = left, step = 2;
      const double D = d == 0 ? c : c + m;
      cur[u] = D;
      steps[(int64_t)d * inner + u] = (unsigned char)step;
      if (d == lx + ly - 2) g.cost[p] = D;  // the one cell of the last diagonal
    }
    __syncthreads();  // diagonal d complete; its readers (d + 1) come before the writer of d + 3
  }
  dtw_backtrack(g, p, la, lb, SWAP, inner, &n_shared);
}

// ---------------------------------------------------------------- path metrics
FS2_DEV double mt_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the same value in every thread: wave trees, then the waves in order
FS2_DEV double mt_block_sum(double v, double* red) {
  v = mt_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < MT_W; ++w) s += red[w];
  __syncthreads();
  return s;
}

// One block per pair; thread t takes the path entries t, t + 256, ... in order.
__global__ __launch_bounds__(MT_T) void path_metrics_kernel(
    const double* __restrict__ cost, const int2* __restrict__ path,
    const int* __restrict__ path_len, const int64_t* __restrict__ la,
    const int64_t* __restrict__ lb, int t1_max, int t2_max, const float* __restrict__ fa,
    const float* __restrict__ fb, double* __restrict__ rec) {
  __shared__ double red[MT_W];
  const int p = blockIdx.x, L = t1_max + t2_max - 1;
  const int n = min(max(path_len[p], 1), L);
  double vv = 0.0, sq = 0.0, vuv = 0.0;
  if (fa && fb) {
    const int2* pp = path + (int64_t)p * L;
    const float* ra = fa + (int64_t)p * t1_max;
    const float* rb = fb + (int64_t)p * t2_max;
    for (int e = threadIdx.x; e < n; e += MT_T) {
      const int2 ij = pp[e];
      const int i = min(max(ij.x, 0), t1_max - 1), j = min(max(ij.y, 0), t2_max - 1);
      const float x = ra[i], y = rb[j];
      const bool va = x > 0.f, vb = y > 0.f;
      if (va && vb) {
        const double c = 1200.0 * log2((double)x / (double)y);
        vv += 1.0;
        sq = fma(c, c, sq);
      } else if (va != vb) {
        vuv += 1.0;
      }
    }
    vv = mt_block_sum(vv, red);
    sq = mt_block_sum(sq, red);
    vuv = mt_block_sum(vuv, red);
  }
  if (threadIdx.x != 0) return;
  const double frames_a = (double)clamp_len(la[p], t1_max), frames_b = (double)clamp_len(lb[p], t2_max);
  double* r = rec + (int64_t)p * FS2_METRIC_FIELDS;
  r[0] = (double)n;
  r[1] = 10.0 / log(10.0) * sqrt(2.0) * cost[p] / (double)n;
  r[2] = frames_a;
  r[3] = frames_b;
  r[4] = vv;
  r[5] = sq;
  r[6] = vuv;
  r[7] = (frames_a - frames_b) / frames_b;
}

static bool dtw_len_ok(int64_t t) { return t >= 1 && t <= FS2_DTW_MAX_LEN; }
static int64_t dtw_steps_pair(int64_t t1, int64_t t2) {
  const int64_t inner = t1 < t2 ? t1 : t2;
  return ((t1 + t2 - 1) * inner + 7) / 8 * 8;  // the reversed path after it stays 8-B aligned
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_mfcc(const float* logmel, const int64_t* n_frames, int64_t batch, int64_t n_mels,
             int64_t frames, int rows, const float* dct, int64_t n_coef, float* out, void* stream) {
  FS2_CHECK_ARG(n_mels >= 2 && n_mels <= FS2_MFCC_MAX_MELS, "fs2_mfcc: n_mels %lld (2..%d)",
                (long long)n_mels, FS2_MFCC_MAX_MELS);
  FS2_CHECK_ARG(n_coef >= 1 && n_coef < n_mels, "fs2_mfcc: n_coef %lld (1..n_mels - 1 = %lld)",
                (long long)n_coef, (long long)n_mels - 1);
  FS2_CHECK_ARG(batch >= 0 && batch <= 65535 && frames >= 0 && frames < (1ll << 24),
                "fs2_mfcc: batch %lld (0..65535), frames %lld (0..2^24 - 1)", (long long)batch,
                (long long)frames);
  FS2_CHECK_ARG(rows == 0 || rows == 1, "fs2_mfcc: rows %d (0: (B, n_mels, F), 1: (B F, n_mels))",
                rows);
  if (batch == 0 || frames == 0) return FS2_OK;
  FS2_CHECK_ARG(logmel && dct && out, "fs2_mfcc: missing operand");
  const dim3 grid((unsigned)((frames + MF_TILE - 1) / MF_TILE), (unsigned)batch);
  mfcc_kernel<<<grid, MT_T, 0, as_stream(stream)>>>(logmel, n_frames, (int)n_mels, (int)frames,
                                                    rows, dct, (int)n_coef, out);
  return launch_status("fs2_mfcc");
}

int64_t fs2_dtw_ws_bytes(int64_t batch, int64_t t1_max, int64_t t2_max, int64_t k) {
  if (batch < 1 || !dtw_len_ok(t1_max) || !dtw_len_ok(t2_max) || k < 1 || k >= (1 << 16)) return 0;
  return batch * (dtw_steps_pair(t1_max, t2_max) + (t1_max + t2_max - 1) * 8 +
                  (t1_max + t2_max) * k * 4);
}

int fs2_dtw(const float* a, const float* b, const int64_t* la, const int64_t* lb, int64_t batch,
            int64_t t1_max, int64_t t2_max, int64_t k, double* cost, int* path, int* path_len,
            void* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(dtw_len_ok(t1_max) && dtw_len_ok(t2_max),
                "fs2_dtw: padded lengths %lld x %lld (1..%d each)", (long long)t1_max,
                (long long)t2_max, FS2_DTW_MAX_LEN);
  FS2_CHECK_ARG(k >= 1 && k < (1 << 16), "fs2_dtw: K %lld (1..65535)", (long long)k);
  FS2_CHECK_ARG(batch >= 0 && batch < (1 << 20), "fs2_dtw: batch %lld", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(a && b && la && lb && cost && path && path_len && ws, "fs2_dtw: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_dtw_ws_bytes(batch, t1_max, t2_max, k),
                "fs2_dtw: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_dtw_ws_bytes(batch, t1_max, t2_max, k));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  DtwArgs g;
  g.a = a, g.b = b, g.la = la, g.lb = lb;
  g.t1_max = (int)t1_max, g.t2_max = (int)t2_max, g.k = (int)k;
  g.cost = cost, g.path = path, g.path_len = path_len;
  g.steps_pair = dtw_steps_pair(t1_max, t2_max);
  g.steps = (unsigned char*)ws;
  g.rev = (int2*)((unsigned char*)ws + batch * g.steps_pair);
  g.feat = (float*)(g.rev + batch * (t1_max + t2_max - 1));
  const bool swap = t2_max < t1_max;
  const size_t lds = 3 * (size_t)(swap ? t2_max : t1_max) * sizeof(double);
  if (swap) dtw_kernel<true><<<(unsigned)batch, MT_T, lds, st>>>(g);
  else dtw_kernel<false><<<(unsigned)batch, MT_T, lds, st>>>(g);
  return launch_status("fs2_dtw");
}

int fs2_path_metrics(const double* cost, const int* path, const int* path_len, const int64_t* la,
                     const int64_t* lb, int64_t batch, int64_t t1_max, int64_t t2_max,
                     const float* fa, const float* fb, double* rec, void* stream) {
  FS2_CHECK_ARG(dtw_len_ok(t1_max) && dtw_len_ok(t2_max),
                "fs2_path_metrics: padded lengths %lld x %lld (1..%d each)", (long long)t1_max,
                (long long)t2_max, FS2_DTW_MAX_LEN);
  FS2_CHECK_ARG(batch >= 0 && batch < (1 << 20), "fs2_path_metrics: batch %lld", (long long)batch);
  FS2_CHECK_ARG((fa == nullptr) == (fb == nullptr),
                "fs2_path_metrics: the F0 contours come as a pair or not at all");
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(cost && path && path_len && la && lb && rec, "fs2_path_metrics: missing operand");
  path_metrics_kernel<<<(unsigned)batch, MT_T, 0, as_stream(stream)>>>(
      cost, reinterpret_cast<const int2*>(path), path_len, la, lb, (int)t1_max, (int)t2_max, fa, fb,
      rec);
  return launch_status("fs2_path_metrics");
}

}  // extern "C"
