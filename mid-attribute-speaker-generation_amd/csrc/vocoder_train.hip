// The HiFi-GAN generator's backward (hifigan/models.py:155-171 under autograd) beyond the data
// gradients, which are fs2_conv_gemm_ex on dy with w_bwd:
//
// * fs2_conv_wgrad_dil: the weight gradient of a dilated Conv1d for any channel counts,
//   taps <= 11.  dw[o, kk] = sum_r dy[r, o] x~[r, kk] with x~[r, j*Cin + c] = x[r + j*dil - pad, c]
//   is a GEMM whose reduction runs over the rows, both operands row-major in memory.  A block of
//   4 waves owns a 64 (o) x 64 (kk) tile and one range of the rows.  Per 32 rows it stages both
//   operands TRANSPOSED into LDS ([column][row], so the 8 consecutive k of a bf16 16x16x32
//   fragment, or the single k of an f32 16x16x4 one, are a row read): thread (column tid & 63,
//   rows tid >> 6 + 4 i) loads along the channels (coalesced), the tap shift and the utterance
//   test ride on the load, and the next 32 rows are in registers while the current ones are
//   multiplied.  Wave w owns output rows 16 w .. 16 w + 15 of the tile for all 64 columns; the
//   bias gradient is one more MFMA of the same dy fragment against ones.  Slabs per row range,
//   then wgrad_dil_reduce adds them in a fixed order into the (c_out, c_in, taps) masters.
// * fs2_lrelu_bwd, fs2_vocoder_post_bwd, fs2_convT_wgrad_fold, fs2_mel_l1: vector-unit kernels
//   with fixed summation orders (see include/fs2hip.h for the contracts).
#include <math.h>

#include "common.hpp"

namespace fs2 {

typedef unsigned short vt_u16;
typedef __bf16 vt_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t vt_u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
FS2_DEV float vt_ld(const T* p);
template <>
FS2_DEV float vt_ld<float>(const float* p) { return *p; }
template <>
FS2_DEV float vt_ld<vt_u16>(const vt_u16* p) { return __uint_as_float(((uint32_t)*p) << 16); }

// ------------------------------------------------------------------ dilated weight gradient
constexpr int WD_BM = 64, WD_BN = 64, WD_BK = 32;
constexpr int WD_TAPS_MAX = 11;
constexpr int WD_FILL_TILES = 256;    // tiles that fill the device on their own: no row split
constexpr int WD_TARGET_BLOCKS = 1024;
constexpr int WD_MIN_SPLIT_ROWS = 128;

struct WgradDil {
  const void* dy;
  int64_t ldy;
  const void* x;
  int64_t ldx;
  float* slab;
  float* bslab;
  int64_t M, T;
  int Cin, Cout, taps, pad, dil, Kp;
  int64_t rows_per_split;
  int tiles_o, tiles_k, splits;
};

// the routing rule: tiles, row splits and rows per split
static void wgrad_dil_plan(int64_t rows, int64_t c_in, int64_t c_out, int taps, int* tiles_o,
                           int* tiles_k, int* splits, int64_t* rps) {
  *tiles_o = (int)((c_out + WD_BM - 1) / WD_BM);
  *tiles_k = (int)((taps * c_in + WD_BN - 1) / WD_BN);
  const int64_t tiles = (int64_t)*tiles_o * *tiles_k;
  int64_t s = 1;
  if (tiles < WD_FILL_TILES) {
    s = (WD_TARGET_BLOCKS + tiles - 1) / tiles;
    const int64_t cap = rows / WD_MIN_SPLIT_ROWS;
    s = s > cap ? cap : s;
    s = s < 1 ? 1 : s;
  }
  int64_t r = (rows + s - 1) / s;
  r = (r + WD_BK - 1) / WD_BK * WD_BK;
  r = r < WD_BK ? WD_BK : r;
  *rps = r;
  *splits = (int)((rows + r - 1) / r);
  if (*splits < 1) *splits = 1;
}

template <typename T>
struct WdLd;
template <>
struct WdLd<float> {
  static constexpr int LD = WD_BK + 1;  // odd dword stride: a row-of-columns store spreads banks
};
template <>
struct WdLd<vt_u16> {
  static constexpr int LD = WD_BK + 2;  // 17 dwords: odd, and every 8-k fragment is 4-B aligned
};

template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_dil_kernel(WgradDil a) {
  constexpr int LD = WdLd<T>::LD;
  constexpr bool BF = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) T As[WD_BM * LD];
  __shared__ __attribute__((aligned(16))) T Bs[WD_BN * LD];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;

  const int per_split = a.tiles_o * a.tiles_k;
  const int z = blockIdx.x / per_split, rem = blockIdx.x - z * per_split;
  const int to = rem / a.tiles_k, tk = rem - to * a.tiles_k;
  const int o0 = to * WD_BM, n0 = tk * WD_BN;
  const int64_t r_begin = (int64_t)z * a.rows_per_split;
  int64_t r_end = r_begin + a.rows_per_split;
  if (r_end > a.M) r_end = a.M;
  const int nk = r_end > r_begin ? (int)((r_end - r_begin + WD_BK - 1) / WD_BK) : 0;

  // staging: this thread owns one column of each operand tile and rows rq + 4 i of a k-tile
  const int col = tid & 63, rq = tid >> 6;
  const T* dyp = reinterpret_cast<const T*>(a.dy);
  const T* xp = reinterpret_cast<const T*>(a.x);
  const bool a_ok = o0 + col < a.Cout;
  const int kk = n0 + col;
  const bool b_ok = kk < a.Kp;
  const int bj = b_ok ? kk / a.Cin : 0;
  const int bc = b_ok ? kk - bj * a.Cin : 0;
  const int shift = bj * a.dil - a.pad;  // source row = row + shift, inside the same utterance
  T ra[8], rb[8];
  auto load = [&](int kt) {
    const int64_t m0 = r_begin + (int64_t)kt * WD_BK + rq;
    int64_t t = m0 % a.T;  // frame of the row within its utterance
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t m = m0 + 4 * i;
      const bool mok = m < r_end;
      ra[i] = (mok && a_ok) ? dyp[m * a.ldy + o0 + col] : (T)0;
      const int64_t tt = t + shift;
      rb[i] = (mok && b_ok && tt >= 0 && tt < a.T && m + shift < a.M)
                  ? xp[(m + shift) * a.ldx + bc] : (T)0;
      t += 4;
      while (t >= a.T) t -= a.T;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      As[col * LD + rq + 4 * i] = ra[i];
      Bs[col * LD + rq + 4 * i] = rb[i];
    }
  };

  f32x4 acc[4], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool wave_on = o0 + wave * 16 < a.Cout;             // wave-uniform
  const bool do_bias = a.bslab != nullptr && tk == 0 && wave_on;

  auto compute = [&]() {
    if (!wave_on) return;
    if constexpr (BF) {
      auto frag = [&](const T* img, int row) -> vt_bf16x8 {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(img + row * LD + 8 * g);
        return __builtin_bit_cast(vt_bf16x8, vt_u32x4{p[0], p[1], p[2], p[3]});
      };
      const vt_bf16x8 fa = frag(As, wave * 16 + r16);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, frag(Bs, j * 16 + r16), acc[j], 0, 0, 0);
      if (do_bias) {
        vt_bf16x8 ones;
#pragma unroll
        for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
        accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, ones, accb, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s = 0; s < WD_BK / 4; ++s) {
        const float fa = As[(wave * 16 + r16) * LD + 4 * s + g];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, Bs[(j * 16 + r16) * LD + 4 * s + g],
                                                        acc[j], 0, 0, 0);
        if (do_bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, 1.0f, accb, 0, 0, 0);
      }
    }
  };

  if (nk > 0) load(0);
  for (int kt = 0; kt < nk; ++kt) {
    store();
    __syncthreads();
    if (kt + 1 < nk) load(kt + 1);
    compute();
    __syncthreads();
  }

  // D[row = 4 g + r][col = r16] of each 16 x 16 subtile
  if (wave_on) {
    float* slab = a.slab + (int64_t)z * a.Cout * a.Kp;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + wave * 16 + 4 * g + r, k2 = n0 + j * 16 + r16;
        if (o < a.Cout && k2 < a.Kp) slab[(int64_t)o * a.Kp + k2] = acc[j][r];
      }
    if (do_bias && r16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + wave * 16 + 4 * g + r;
        if (o < a.Cout) a.bslab[(int64_t)z * a.Cout + o] = accb[r];
      }
    }
  }
}

// dw[o][c][j] += sum_z slab[z][o][j*Cin + c], db[o] += sum_z bslab[z][o].  A block owns
// WD_RED_N consecutive slab elements; lane group y sums the splits y, y + WD_RED_G, ... in
// ascending order (four loads in flight), then the WD_RED_G group sums are added in group order:
// a fixed order, with the deep splits' hundreds of slabs read in parallel instead of by one
// thread in a row.  The bias partials are one more row of WD_RED_N-element chunks after the
// weights'.
constexpr int WD_RED_N = 32, WD_RED_G = 8;

FS2_DEV float wd_group_sum(const float* __restrict__ p, int64_t stride, int splits, int y) {
  float s = 0.f;
  int zz = y;
  for (; zz + 3 * WD_RED_G < splits; zz += 4 * WD_RED_G) {
    const float v0 = p[zz * stride], v1 = p[(zz + WD_RED_G) * stride];
    const float v2 = p[(zz + 2 * WD_RED_G) * stride], v3 = p[(zz + 3 * WD_RED_G) * stride];
    s += v0;
    s += v1;
    s += v2;
    s += v3;
  }
  for (; zz < splits; zz += WD_RED_G) s += p[zz * stride];
  return s;
}

__global__ __launch_bounds__(WD_RED_N* WD_RED_G) void wgrad_dil_reduce(
    const float* __restrict__ slab, const float* __restrict__ bslab, int splits, int Cout, int Cin,
    int taps, int64_t w_blocks, float* dw, float* db) {
  __shared__ float red[WD_RED_G][WD_RED_N];
  const int x = threadIdx.x % WD_RED_N, y = threadIdx.x / WD_RED_N;
  const int64_t Kp = (int64_t)taps * Cin, total = (int64_t)Cout * Kp;
  const bool bias = (int64_t)blockIdx.x >= w_blocks;  // block-uniform
  const int64_t i = ((int64_t)blockIdx.x - (bias ? w_blocks : 0)) * WD_RED_N + x;
  const int64_t n = bias ? Cout : total;
  red[y][x] = i < n ? wd_group_sum((bias ? bslab : slab) + i, n, splits, y) : 0.f;
  __syncthreads();
  if (y != 0 || i >= n) return;
  float s = red[0][x];
#pragma unroll
  for (int g2 = 1; g2 < WD_RED_G; ++g2) s += red[g2][x];
  if (bias) {
    db[i] += s;
  } else {
    const int64_t o = i / Kp;
    const int k2 = (int)(i - o * Kp);
    const int j = k2 / Cin, c = k2 - j * Cin;
    dw[(o * Cin + c) * taps + j] += s;
  }
}

// ------------------------------------------------------------------ leaky ReLU backward
template <typename T>
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const T* v, const float* dy, float* dx,
                                                        int64_t n, float alpha, int acc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = dy[i] * (vt_ld<T>(v + i) > 0.f ? 1.f : alpha);
    dx[i] = acc ? dx[i] + d : d;
  }
}

// ------------------------------------------------------------------ output head backward
constexpr int PB_ROWS = 128, PB_TAPS = 7, PB_PAD = 3, PB_HALO = PB_ROWS + PB_TAPS - 1;

template <typename T>
__global__ __launch_bounds__(256) void vocoder_post_bwd_kernel(const T* x, const float* wav,
                                                               const float* d_wav, int64_t rows,
                                                               int64_t T_, int c_in, const float* w,
                                                               float* dx, float* part_w,
                                                               float* part_b) {
  extern __shared__ float sm[];
  float* xs = sm;                                   // (PB_HALO, c_in): rows r0 - 3 ..
  float* gs = xs + PB_HALO * c_in;                  // g of those rows (0 outside the matrix)
  int* ts = reinterpret_cast<int*>(gs + PB_HALO);   // their frame within the utterance
  float* wl = reinterpret_cast<float*>(ts + PB_HALO);  // (c_in, 7) as given
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * PB_ROWS;
  for (int i = tid; i < PB_TAPS * c_in; i += 256) wl[i] = w[i];
  for (int h = tid; h < PB_HALO; h += 256) {
    const int64_t r = r0 - PB_PAD + h;
    float gv = 0.f;
    int t = 0;
    if (r >= 0 && r < rows) {
      const float y = wav[r];
      gv = d_wav[r] * (1.f - y * y);
      t = (int)(r % T_);
    }
    gs[h] = gv;
    ts[h] = t;
  }
  for (int i = tid; i < PB_HALO * c_in; i += 256) {
    const int h = i / c_in, c = i - h * c_in;
    const int64_t r = r0 - PB_PAD + h;
    xs[i] = (r >= 0 && r < rows) ? vt_ld<T>(x + r * c_in + c) : 0.f;
  }
  __syncthreads();
  const int T32 = (int)T_;
  if (dx) {
    for (int i = tid; i < PB_ROWS * c_in; i += 256) {
      const int rl = i / c_in, c = i - rl * c_in;
      const int64_t r = r0 + rl;
      if (r >= rows) break;
      const int t = ts[rl + PB_PAD];
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < PB_TAPS; ++j) {
        const int tt = t - j + PB_PAD;  // the output row whose tap j reads row r
        if (tt >= 0 && tt < T32) s += gs[rl + 2 * PB_PAD - j] * wl[c * PB_TAPS + j];
      }
      dx[r * c_in + c] = s;
    }
  }
  const int nlive = rows - r0 < PB_ROWS ? (int)(rows - r0) : PB_ROWS;
  for (int e = tid; e < PB_TAPS * c_in; e += 256) {
    const int j = e / c_in, c = e - j * c_in;
    float s = 0.f;
    for (int rl = 0; rl < nlive; ++rl) {
      const int tt = ts[rl + PB_PAD] + j - PB_PAD;
      if (tt >= 0 && tt < T32) s += gs[rl + PB_PAD] * xs[(rl + j) * c_in + c];
    }
    part_w[(int64_t)blockIdx.x * PB_TAPS * c_in + c * PB_TAPS + j] = s;
  }
  if (tid == 0) {
    float s = 0.f;
    for (int rl = 0; rl < nlive; ++rl) s += gs[rl + PB_PAD];
    part_b[blockIdx.x] = s;
  }
}

// ------------------------------------------------------------------ transposed-conv fold
__global__ __launch_bounds__(256) void convT_fold_kernel(const float* dwc, const float* dbc,
                                                         int c_in, int c_out, int s, float* dw,
                                                         float* db) {
  const int64_t n = (int64_t)c_in * c_out * 2 * s;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int k = (int)(i % (2 * s));
    const int o = (int)((i / (2 * s)) % c_out);
    const int c = (int)(i / ((int64_t)2 * s * c_out));
    // k = ph + s/2 - s d with ph in [0, s), d in {-1, 0, 1}
    const int u = k - s / 2;  // = ph - s d
    const int d = u < 0 ? 1 : u >= s ? -1 : 0;
    const int ph = u + s * d;
    dw[i] += dwc[(((int64_t)ph * c_out + o) * c_in + c) * 3 + d + 1];
  }
  if (db && i < c_out) {
    float b = 0.f;
    for (int ph = 0; ph < s; ++ph) b += dbc[(int64_t)ph * c_out + i];
    db[i] += b;
  }
}

// ------------------------------------------------------------------ mel L1
constexpr int L1_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void mel_l1_partial(const float* a, const float* b, int64_t n,
                                                      float inv_n, float* d_a, double* part) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = a[i] - b[i];
    s += (double)fabsf(d);
    if (d_a) d_a[i] = d > 0.f ? inv_n : d < 0.f ? -inv_n : 0.f;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ void mel_l1_final(const double* part, int nparts, int64_t n, float* loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s += part[p];
    loss[0] = (float)(s / (double)n);
  }
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int64_t fs2_conv_wgrad_dil_ws_bytes(int64_t rows, int64_t c_in, int64_t c_out, int taps) {
  if (rows < 1 || c_in < 1 || c_out < 1 || taps < 1) return 0;
  int to, tk, splits;
  int64_t rps;
  wgrad_dil_plan(rows, c_in, c_out, taps, &to, &tk, &splits, &rps);
  return (int64_t)splits * (c_out * taps * c_in + c_out) * (int64_t)sizeof(float);
}

int fs2_conv_wgrad_dil(int dtype, const void* dy, int64_t ldy, const void* x, int64_t ldx,
                       float* dw, float* db, int64_t rows, int64_t seq_len, int64_t c_in,
                       int64_t c_out, int taps, int pad, int dilation, float* ws,
                       int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(rows >= 0 && seq_len > 0 && c_in >= 1 && c_out >= 1 && taps >= 1 &&
                    taps <= WD_TAPS_MAX && dilation >= 1 && pad >= 0 &&
                    (int64_t)pad <= (int64_t)(taps - 1) * dilation,
                "fs2_conv_wgrad_dil: bad geometry (c_in %lld, c_out %lld, taps %d <= %d, pad %d, "
                "dilation %d)", (long long)c_in, (long long)c_out, taps, WD_TAPS_MAX, pad, dilation);
  FS2_CHECK_ARG(c_in * taps < (1ll << 24) && c_out < (1ll << 24) &&
                    (int64_t)taps * dilation < (1ll << 24),
                "fs2_conv_wgrad_dil: channel counts / dilation too large");
  FS2_CHECK_ARG(ldy >= c_out && ldx >= c_in, "fs2_conv_wgrad_dil: ldy / ldx below the channel counts");
  FS2_CHECK_ARG(rows % seq_len == 0, "fs2_conv_wgrad_dil: rows %lld is not batch x seq_len %lld",
                (long long)rows, (long long)seq_len);
  if (dtype != FS2_F32 && dtype != FS2_BF16) {
    set_error("fs2_conv_wgrad_dil: dtype %d not built", dtype);
    return FS2_ERR_DTYPE;
  }
  if (rows == 0) return FS2_OK;
  FS2_CHECK_ARG(dy && x && dw && ws, "fs2_conv_wgrad_dil: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_conv_wgrad_dil_ws_bytes(rows, c_in, c_out, taps),
                "fs2_conv_wgrad_dil: workspace too small (%lld bytes needed)",
                (long long)fs2_conv_wgrad_dil_ws_bytes(rows, c_in, c_out, taps));
  int to, tk, splits;
  int64_t rps;
  wgrad_dil_plan(rows, c_in, c_out, taps, &to, &tk, &splits, &rps);
  const int64_t Kp = (int64_t)taps * c_in;
  const int64_t blocks = (int64_t)to * tk * splits;
  FS2_CHECK_ARG(blocks < (1ll << 31), "fs2_conv_wgrad_dil: grid too large");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  float* bslab = db ? ws + (int64_t)splits * c_out * Kp : nullptr;
  const WgradDil a{dy, ldy, x, ldx, ws, bslab, rows, seq_len, (int)c_in, (int)c_out, taps, pad,
                   dilation, (int)Kp, rps, to, tk, splits};
  if (dtype == FS2_BF16)
    conv_wgrad_dil_kernel<vt_u16><<<(unsigned)blocks, 256, 0, st>>>(a);
  else
    conv_wgrad_dil_kernel<float><<<(unsigned)blocks, 256, 0, st>>>(a);
  const int64_t w_blocks = (c_out * Kp + WD_RED_N - 1) / WD_RED_N;
  const int64_t b_blocks = db ? (c_out + WD_RED_N - 1) / WD_RED_N : 0;
  FS2_CHECK_ARG(w_blocks + b_blocks < (1ll << 31), "fs2_conv_wgrad_dil: weight too large");
  wgrad_dil_reduce<<<(unsigned)(w_blocks + b_blocks), WD_RED_N * WD_RED_G, 0, st>>>(
      ws, bslab, splits, (int)c_out, (int)c_in, taps, w_blocks, dw, db);
  return launch_status("fs2_conv_wgrad_dil");
}

int fs2_lrelu_bwd(int dtype, const void* v, const float* dy, float* dx, int64_t n, float alpha,
                  int accumulate, void* stream) {
  FS2_CHECK_ARG(n >= 0, "fs2_lrelu_bwd: n %lld", (long long)n);
  if (dtype != FS2_F32 && dtype != FS2_BF16) {
    set_error("fs2_lrelu_bwd: dtype %d not built", dtype);
    return FS2_ERR_DTYPE;
  }
  if (n == 0) return FS2_OK;
  FS2_CHECK_ARG(v && dy && dx, "fs2_lrelu_bwd: missing operand");
  int64_t blocks = (n + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  if (dtype == FS2_BF16)
    lrelu_bwd_kernel<vt_u16><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(
        (const vt_u16*)v, dy, dx, n, alpha, accumulate);
  else
    lrelu_bwd_kernel<float><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>((const float*)v, dy, dx,
                                                                            n, alpha, accumulate);
  return launch_status("fs2_lrelu_bwd");
}

int64_t fs2_vocoder_post_bwd_ws_bytes(int64_t rows, int64_t c_in) {
  if (rows < 1 || c_in < 1) return 0;
  const int64_t nb = (rows + PB_ROWS - 1) / PB_ROWS;
  return nb * (PB_TAPS * c_in + 1) * (int64_t)sizeof(float);
}

int fs2_vocoder_post_bwd(int dtype, const void* x, const float* wav, const float* d_wav,
                         int64_t rows, int64_t seq_len, int64_t c_in, const float* w, float* dx,
                         float* dw, float* db, float* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(rows >= 0 && seq_len > 0 && seq_len < (1ll << 31) && c_in >= 1 && c_in <= 64,
                "fs2_vocoder_post_bwd: bad arguments (1 <= c_in %lld <= 64)", (long long)c_in);
  if (dtype != FS2_F32 && dtype != FS2_BF16) {
    set_error("fs2_vocoder_post_bwd: dtype %d not built", dtype);
    return FS2_ERR_DTYPE;
  }
  if (rows == 0) return FS2_OK;
  FS2_CHECK_ARG(x && wav && d_wav && w && dw && db && ws, "fs2_vocoder_post_bwd: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_vocoder_post_bwd_ws_bytes(rows, c_in),
                "fs2_vocoder_post_bwd: workspace too small");
  const int64_t nb = (rows + PB_ROWS - 1) / PB_ROWS;
  FS2_CHECK_ARG(nb < (1ll << 31), "fs2_vocoder_post_bwd: too many rows");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  float* part_w = ws;
  float* part_b = ws + nb * PB_TAPS * c_in;
  const size_t smem = sizeof(float) * ((size_t)PB_HALO * c_in + 2 * PB_HALO + PB_TAPS * c_in);
  if (dtype == FS2_BF16)
    vocoder_post_bwd_kernel<vt_u16><<<(unsigned)nb, 256, smem, st>>>(
        (const vt_u16*)x, wav, d_wav, rows, seq_len, (int)c_in, w, dx, part_w, part_b);
  else
    vocoder_post_bwd_kernel<float><<<(unsigned)nb, 256, smem, st>>>(
        (const float*)x, wav, d_wav, rows, seq_len, (int)c_in, w, dx, part_w, part_b);
  if (const int rc = launch_status("fs2_vocoder_post_bwd")) return rc;
  if (const int rc = colsum_final_launch(part_w, nb, PB_TAPS * c_in, dw, 1, st)) return rc;
  return colsum_final_launch(part_b, nb, 1, db, 1, st);
}

int fs2_convT_wgrad_fold(const float* dwc, const float* dbc, int64_t c_in, int64_t c_out,
                         int stride, float* dw, float* db, void* stream) {
  FS2_CHECK_ARG(dwc && dw && c_in > 0 && c_out > 0 && stride >= 2 && stride % 2 == 0,
                "fs2_convT_wgrad_fold: needs k = 2*stride, even stride (got stride %d)", stride);
  FS2_CHECK_ARG((db == nullptr) == (dbc == nullptr), "fs2_convT_wgrad_fold: dbc and db go together");
  const int64_t n = c_in * c_out * 2 * stride;
  FS2_CHECK_ARG(n < (1ll << 38), "fs2_convT_wgrad_fold: weight too large");
  convT_fold_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(
      dwc, dbc, (int)c_in, (int)c_out, stride, dw, db);
  return launch_status("fs2_convT_wgrad_fold");
}

int64_t fs2_mel_l1_ws_bytes(void) { return L1_MAX_BLOCKS * (int64_t)sizeof(double); }

int fs2_mel_l1(const float* a, const float* b, int64_t n, float* loss, float* d_a, float* ws,
               int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(n >= 1 && a && b && loss && ws, "fs2_mel_l1: missing operand or n %lld < 1",
                (long long)n);
  FS2_CHECK_ARG(ws_bytes >= fs2_mel_l1_ws_bytes(), "fs2_mel_l1: workspace too small");
  int64_t blocks = (n + 255) / 256;
  blocks = blocks > L1_MAX_BLOCKS ? L1_MAX_BLOCKS : blocks;
  FS2_CHECK_ARG(((uintptr_t)ws & 7) == 0, "fs2_mel_l1: the workspace must be 8-B aligned");
  hipStream_t st = as_stream(stream);
  double* part = reinterpret_cast<double*>(ws);
  mel_l1_partial<<<(unsigned)blocks, 256, 0, st>>>(a, b, n, (float)(1.0 / (double)n), d_a, part);
  mel_l1_final<<<1, 64, 0, st>>>(part, (int)blocks, n, loss);
  return launch_status("fs2_mel_l1");
}

}  // extern "C"
