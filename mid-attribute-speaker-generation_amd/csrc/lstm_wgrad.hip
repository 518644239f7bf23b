// Weight gradients of the GE2E LSTM stack (train_speech_embedder.py steps the embedder; the
// --use_clf path of train.py only needs dx, see lstm.hip).  For layer l, fp32:
//   dW_ih[l] (4H, c_in_l) = sum_rows dgates[l][row]^T (x) in_l[row]      in_0 = x, in_l = h[l-1]
//   dW_hh[l] (4H, H)      = sum_rows dgates[l][row]^T (x) h[l][row - 1]  (0 at t = 0)
//   db[l]    (4H)         = sum_rows dgates[l][row]
// i.e. one GEMM per layer with the rows as the reduction dimension, M = 4H gate rows and
// N = the concatenated panel [in_l(row) | h_l(row - 1)] (c_in_l + H columns), so dW_ih and
// dW_hh leave one pass over dgates.
//
// Tiling: a block owns a 256 x 256 output tile and one slice of the rows; 8 waves as 4 x 2,
// each 64 x 128 = 4 x 8 tiles of v_mfma_f32_16x16x4_f32 (exact f32).  (A 128 x 128 tile moves
// 1 byte per 32 FLOP through L2 -- 4.8 TB/s at the MFMA peak -- and measured 27% of peak; the
// 256 x 256 tile halves that.)  Per stage 16 rows of both panels go through registers into LDS
// (row stride 272 floats: the 4 rows a wave reads at once land 16 banks apart, its 16 columns
// are consecutive); the loads of stage s + 1 are in flight while stage s is multiplied.  The
// h(row - 1) columns are zeroed where row is the first frame of its sequence, whichever stage
// or slice it falls into; waves whose 128 columns lie past layer 0's narrower panel skip the
// MFMAs.  The blocks of column tile 0 also add their dgates panel down the rows from the same
// LDS stage (one thread per gate column, rows in order): the bias sums.
//
// The stack has 24 such tiles, far fewer than the CUs, so the rows are split into as many
// slices as fill the CUs once (10 on 256 CUs, each of at least 128 rows); every slice writes
// its partial tile to the workspace and a second kernel adds the slices in slice order (no
// atomics: bitwise repeatable on a device) into the outputs, with beta in {0, 1}.
#include "common.hpp"

namespace fs2 {

using f32x4w = __attribute__((__vector_size__(4 * sizeof(float)))) float;

constexpr int WG_T = 256;         // output tile edge
constexpr int WG_RK = 16;         // rows per LDS stage
constexpr int WG_LD = WG_T + 16;  // LDS row stride (floats)
constexpr int WG_THREADS = 512;   // 8 waves as 4 (M) x 2 (N), each 64 x 128
constexpr int WG_MAX_SPLITS = 16;
constexpr int WG_SPLIT_ROWS = 128;  // at least this many rows per slice

struct LstmWgrad {
  const float* x;   // (rows, c_in)
  const float* h;   // (L, rows, H)
  const float* dg;  // (L, rows, 4H)
  float* part;      // (splits, L, 4H, ldp)
  float* partb;     // (splits, L, 4H)
  int N, T, H, L, c_in, splits, ldp;
  int64_t rows_per_split;
};

static int64_t wgrad_ldp(int64_t c_in, int64_t hidden) {
  const int64_t kw = hidden + (c_in > hidden ? c_in : hidden);
  return (kw + WG_T - 1) / WG_T * WG_T;
}
static int wgrad_cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      n = v;
    else
      n = 256;
  }
  return n;
}
// one block per CU (8 waves of ~250 VGPRs): as many slices as fill the CUs once, each of at
// least WG_SPLIT_ROWS rows
static int wgrad_splits(int64_t rows, int64_t c_in, int64_t hidden, int layers) {
  const int64_t tiles = 4 * hidden / WG_T * (wgrad_ldp(c_in, hidden) / WG_T) * layers;
  int64_t s = wgrad_cu_count() / tiles;
  const int64_t by_rows = (rows + WG_SPLIT_ROWS - 1) / WG_SPLIT_ROWS;
  if (s > by_rows) s = by_rows;
  return (int)(s < 1 ? 1 : s > WG_MAX_SPLITS ? WG_MAX_SPLITS : s);
}

__global__ __launch_bounds__(WG_THREADS) void lstm_wgrad_kernel(LstmWgrad a) {
  __shared__ __attribute__((aligned(16))) float As[WG_RK][WG_LD];
  __shared__ __attribute__((aligned(16))) float Bs[WG_RK][WG_LD];
  const int l = blockIdx.z / a.splits, sp = blockIdx.z % a.splits;
  const int H = a.H, G = 4 * H, T = a.T;
  const int cin = l == 0 ? a.c_in : H, kw = cin + H;
  const int n0 = blockIdx.x * WG_T, m0 = blockIdx.y * WG_T;
  if (n0 >= kw) return;  // block-uniform: layer 0's panel is narrower
  const int64_t rows = (int64_t)a.N * T;
  const int64_t r_begin = (int64_t)sp * a.rows_per_split;
  const int64_t r_end = r_begin + a.rows_per_split < rows ? r_begin + a.rows_per_split : rows;
  const float* dg_l = a.dg + (int64_t)l * rows * G;
  const float* in_l = l == 0 ? a.x : a.h + (int64_t)(l - 1) * rows * H;
  const float* h_l = a.h + (int64_t)l * rows * H;

  // loader: thread -> 4 columns (lc) of rows lr and lr + 8 of the stage
  const int lc = (threadIdx.x & 63) * 4, lr = threadIdx.x >> 6;
  const int kcol = n0 + lc;  // panel column of this thread's float4
  float4 ra[2], rb[2];
  auto fetch = [&](int64_t r0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t r = r0 + lr + 8 * j;
      ra[j] = rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r >= r_end) continue;
      ra[j] = *reinterpret_cast<const float4*>(dg_l + r * G + m0 + lc);
      if (kcol < cin) {
        rb[j] = *reinterpret_cast<const float4*>(in_l + r * cin + kcol);
      } else if (kcol < kw && r % T != 0) {  // h_{t-1}; 0 at the first frame of a sequence
        rb[j] = *reinterpret_cast<const float4*>(h_l + (r - 1) * H + (kcol - cin));
      }
    }
  };

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wave >> 1, wn = wave & 1, r16 = lane & 15, kq = lane >> 4;
  // the column tile n = 0 also sums its dgates panel down the rows (thread -> gate column)
  const bool bias = blockIdx.x == 0 && threadIdx.x < WG_T;  // wave-uniform
  float bsum = 0.f;
  const bool live = n0 + wn * 128 < kw;          // wave-uniform: columns inside the panel
  f32x4w acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4w{0.f, 0.f, 0.f, 0.f};
  }

  if (r_begin < r_end) fetch(r_begin);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += WG_RK) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<float4*>(&As[lr + 8 * j][lc]) = ra[j];
      *reinterpret_cast<float4*>(&Bs[lr + 8 * j][lc]) = rb[j];
    }
    __syncthreads();
    if (r0 + WG_RK < r_end) fetch(r0 + WG_RK);
    if (live) {
#pragma unroll
      for (int sub = 0; sub < WG_RK / 4; ++sub) {
        const int rr = sub * 4 + kq;
        float av[4], bv[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = As[rr][wm * 64 + 16 * i + r16];
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = Bs[rr][wn * 128 + 16 * j + r16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
      }
    }
    if (bias) {
#pragma unroll
      for (int rr = 0; rr < WG_RK; ++rr) bsum += As[rr][threadIdx.x];
    }
    __syncthreads();
  }

  // D of tile (i, j): register q is row 4 kq + q, column r16
  const int64_t slab = (int64_t)sp * a.L + l;
  float* pt = a.part + slab * G * a.ldp;
  if (bias) a.partb[slab * G + m0 + threadIdx.x] = bsum;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + wm * 64 + 16 * i + 4 * kq + q;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = n0 + wn * 128 + 16 * j + r16;
        if (n < kw) pt[(int64_t)m * a.ldp + n] = acc[i][j][q];
      }
    }
  }
}

struct LstmWgradOut {
  const float* part;
  const float* partb;
  float* dw_ih0;   // (4H, c_in)
  float* dw_ih_up; // (L-1, 4H, H)
  float* dw_hh;    // (L, 4H, H)
  float* db;       // (L, 4H)
  int H, L, c_in, splits, ldp, beta;
};

// out (+)= sum over the slices, in slice order.  grid (4H * ldp / 256 + 4H / 256, L)
__global__ __launch_bounds__(256) void lstm_wgrad_reduce(LstmWgradOut a) {
  const int l = blockIdx.y, H = a.H, G = 4 * H;
  const int cin = l == 0 ? a.c_in : H, kw = cin + H;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nw = (int64_t)G * a.ldp;
  float* out;
  const float* src;
  int64_t stride;
  if (idx < nw) {
    const int m = (int)(idx / a.ldp), n = (int)(idx % a.ldp);
    if (n >= kw) return;
    if (n < cin)
      out = (l == 0 ? a.dw_ih0 : a.dw_ih_up + (int64_t)(l - 1) * G * H) + (int64_t)m * cin + n;
    else
      out = a.dw_hh + ((int64_t)l * G + m) * H + (n - cin);
    src = a.part + (int64_t)l * nw + idx;
    stride = (int64_t)a.L * nw;
  } else {
    const int64_t m = idx - nw;
    if (m >= G) return;
    out = a.db + (int64_t)l * G + m;
    src = a.partb + (int64_t)l * G + m;
    stride = (int64_t)a.L * G;
  }
  float s = 0.f;
  for (int p = 0; p < a.splits; ++p) s += src[p * stride];
  *out = a.beta ? *out + s : s;
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int64_t fs2_lstm_stack_wgrad_ws_bytes(int64_t n_seq, int64_t steps, int64_t c_in, int64_t hidden,
                                      int layers) {
  if (n_seq < 1 || steps < 1 || c_in < 1 || hidden < 1 || layers < 1) return 0;
  const int64_t G = 4 * hidden;
  return (int64_t)wgrad_splits(n_seq * steps, c_in, hidden, layers) * layers * G * (wgrad_ldp(c_in, hidden) + 1) * 4;
}

int fs2_lstm_stack_wgrad(const float* x, const float* h_all, const float* dgates, int64_t n_seq,
                         int64_t steps, int64_t c_in, int64_t hidden, int layers, float* dw_ih0,
                         float* dw_ih_up, float* dw_hh, float* db, int beta, float* ws,
                         int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(hidden > 0 && hidden % 256 == 0 && c_in > 0 && c_in % 4 == 0 && layers >= 1,
                "fs2_lstm_stack_wgrad: hidden %lld (multiple of 256), c_in %lld (multiple of 4), "
                "layers %d >= 1", (long long)hidden, (long long)c_in, layers);
  FS2_CHECK_ARG(n_seq >= 1 && steps >= 1 && n_seq * steps < (1ll << 31) && n_seq < (1ll << 31) &&
                    steps < (1ll << 31),
                "fs2_lstm_stack_wgrad: n_seq %lld, steps %lld (>= 1, rows < 2^31)",
                (long long)n_seq, (long long)steps);
  FS2_CHECK_ARG(beta == 0 || beta == 1, "fs2_lstm_stack_wgrad: beta %d (0 or 1)", beta);
  FS2_CHECK_ARG(x && h_all && dgates && dw_ih0 && dw_hh && db && ws && (layers == 1 || dw_ih_up),
                "fs2_lstm_stack_wgrad: missing operand");
  FS2_CHECK_ARG((((uintptr_t)x | (uintptr_t)h_all | (uintptr_t)dgates | (uintptr_t)ws) & 15) == 0,
                "fs2_lstm_stack_wgrad: operands must be 16-B aligned");
  FS2_CHECK_ARG(ws_bytes >= fs2_lstm_stack_wgrad_ws_bytes(n_seq, steps, c_in, hidden, layers),
                "fs2_lstm_stack_wgrad: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const int64_t rows = n_seq * steps, G = 4 * hidden;
  const int splits = wgrad_splits(rows, c_in, hidden, layers), ldp = (int)wgrad_ldp(c_in, hidden);
  int64_t rps = (rows + splits - 1) / splits;
  rps = (rps + WG_RK - 1) / WG_RK * WG_RK;
  float* part = ws;
  float* partb = ws + (int64_t)splits * layers * G * ldp;
  LstmWgrad a{x, h_all, dgates, part, partb, (int)n_seq, (int)steps, (int)hidden, layers,
              (int)c_in, splits, ldp, rps};
  lstm_wgrad_kernel<<<dim3((unsigned)(ldp / WG_T), (unsigned)(G / WG_T),
                           (unsigned)(layers * splits)), WG_THREADS, 0, st>>>(a);
  LstmWgradOut o{part, partb, dw_ih0, dw_ih_up, dw_hh, db, (int)hidden, layers, (int)c_in, splits,
                 ldp, beta};
  lstm_wgrad_reduce<<<dim3((unsigned)((G * ldp + G + 255) / 256), (unsigned)layers), 256, 0, st>>>(o);
  return launch_status("fs2_lstm_stack_wgrad");
}

}  // extern "C"
