// The ResCNN speaker encoder (speech_embedder_net.py:19-63, module.py:59-117): Conv2d,
// BatchNorm2d (+ residual, ReLU), the mean over time with dropout and the channel-major
// flatten, and the embedding / domain-classifier head at any input width.  fp32 throughout;
// every reduction runs in a fixed order (no atomics), so gradients repeat bitwise.
//
// Activations are channels-last with TIME as the outer spatial axis: (N, W, H, C), W = time,
// H = mel.  The encoder's input x (N, T, 80) is exactly that with C = 1, so conv1 reads it
// with no transpose pass.  A torch weight (C_out, C_in, kh, kw) has kh over H and kw over W;
// the tap index used here is tap = kw * k + kh (outer axis first).
//
// Convolutions with C_in % 16 == 0 are implicit GEMMs on v_mfma_f32_16x16x4_f32 (exact f32):
// rows = output positions, columns = output channels, K = taps x C_in.  A wave owns 32
// positions x (16 NT) channels.  Per tap and block of 16 input channels lane (l & 15, g = l >> 4)
// loads ONE float4 of A, channels 4g .. 4g + 3 of its position, and one float4 of B per
// column tile; MFMA step j multiplies component j of both, i.e. the K index of step j in lane
// group g is channel 4g + j.  The prepared weight is laid out for that:
//   w_fwd[tap][ci / 16][g][co][j],  ci = 16 (ci / 16) + 4 g + j
// and the data gradient is the same kernel on dy with the roles of the channels exchanged
// (w_bwd[tap][co / 16][g][ci][j]) and the gather rule  w_out = (w_in + pad - kw) / s  when that
// divides and is in range (for stride 2: the output positions of matching parity).
#include <math.h>

#include "common.hpp"

namespace fs2 {

struct Conv2 {
  const float* x;      // source (N, Ws, Hs, Cs): the input (forward) or dy (data gradient)
  const float* wk;     // prepared weight
  const float* bias;   // (Cd) or NULL
  const float* scale;  // (Cd) or NULL: folded eval BatchNorm  y = y * scale + shift
  const float* shift;
  const float* res;    // (M, Cd) or NULL, added before the ReLU
  float* y;            // (N, Wd, Hd, Cd)
  int N, Ws, Hs, Cs, Wd, Hd, Cd, k, s, pad, relu;
  int64_t M;           // N * Wd * Hd
};

// source position of destination (wd, hd) under tap (kw, kh); false = padding / no such output
template <bool DGRAD>
FS2_DEV bool tap_src(const Conv2& a, int wd, int hd, int kw, int kh, int& ws, int& hs) {
  if (!DGRAD) {
    ws = wd * a.s - a.pad + kw;
    hs = hd * a.s - a.pad + kh;
    return ws >= 0 && ws < a.Ws && hs >= 0 && hs < a.Hs;
  }
  const int tw = wd + a.pad - kw, th = hd + a.pad - kh;
  if (tw < 0 || th < 0 || tw % a.s || th % a.s) return false;
  ws = tw / a.s;
  hs = th / a.s;
  return ws < a.Ws && hs < a.Hs;
}

FS2_DEV float epilogue(const Conv2& a, float v, int64_t pos, int col) {
  if (a.bias) v += a.bias[col];
  if (a.scale) v = v * a.scale[col] + a.shift[col];
  if (a.res) v += a.res[pos * a.Cd + col];
  return a.relu ? fmaxf(v, 0.f) : v;
}

template <int NT, bool DGRAD>
__global__ __launch_bounds__(256) void conv2d_mfma(Conv2 a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int64_t base = ((int64_t)blockIdx.x * 4 + wave) * 32;
  if (base >= a.M) return;  // whole wave
  const int n0 = blockIdx.y * 16 * NT;
  int pn[2], pw[2], ph[2];
  bool live[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int64_t p = base + mt * 16 + l15;
    live[mt] = p < a.M;
    const int64_t q = live[mt] ? p : 0;
    ph[mt] = (int)(q % a.Hd);
    pw[mt] = (int)((q / a.Hd) % a.Wd);
    pn[mt] = (int)(q / ((int64_t)a.Hd * a.Wd));
  }
  f32x4 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int cblocks = a.Cs >> 4;
  for (int kw = 0; kw < a.k; ++kw) {
    for (int kh = 0; kh < a.k; ++kh) {
      const float* src[2];
      bool ok[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        int ws = 0, hs = 0;
        ok[mt] = live[mt] && tap_src<DGRAD>(a, pw[mt], ph[mt], kw, kh, ws, hs);
        src[mt] = a.x + (((int64_t)pn[mt] * a.Ws + ws) * a.Hs + hs) * a.Cs + 4 * g;
      }
      if (!__any(ok[0] || ok[1])) continue;  // wave-uniform: the tap is padding for all 32
      const float* wt = a.wk + (((int64_t)(kw * a.k + kh) * cblocks * 4 + g) * a.Cd + n0 + l15) * 4;
      // the tap's channels are summed on their own and then added to the running total: the
      // fma chains stay C_in long instead of k * k * C_in (blocked summation, smaller error)
      f32x4 tacc[2][NT];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) tacc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int cb = 0; cb < cblocks; ++cb) {
        f32x4 av[2], bv[NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
          av[mt] = ok[mt] ? ld4(src[mt] + cb * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = ld4(wt + ((int64_t)cb * 4 * a.Cd + nt * 16) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              tacc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][j], bv[nt][j],
                                                                  tacc[mt][nt], 0, 0, 0);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] += tacc[mt][nt];
    }
  }
  // D[row 4g + i][col l15]
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t pos = base + mt * 16 + 4 * g + i;
      if (pos >= a.M) continue;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + nt * 16 + l15;
        a.y[pos * a.Cd + col] = epilogue(a, acc[mt][nt][i], pos, col);
      }
    }
}

// C_in = 1 (conv1): 4 output channels of one position per thread, the k*k taps of the
// (tap, co) weight from LDS
constexpr int DIRECT_W = 1024;
__global__ __launch_bounds__(256) void conv2d_direct_fwd(Conv2 a) {
  __shared__ float wl[DIRECT_W];
  const int nw = a.k * a.k * a.Cd;
  for (int i = threadIdx.x; i < nw; i += 256) wl[i] = a.wk[i];
  __syncthreads();
  const int quads = a.Cd >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.M * quads) return;
  const int64_t pos = idx / quads;
  const int c0 = (int)(idx % quads) * 4;
  const int hd = (int)(pos % a.Hd), wd = (int)((pos / a.Hd) % a.Wd);
  const int64_t n = pos / ((int64_t)a.Hd * a.Wd);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kw = 0; kw < a.k; ++kw)
    for (int kh = 0; kh < a.k; ++kh) {
      int ws, hs;
      if (!tap_src<false>(a, wd, hd, kw, kh, ws, hs)) continue;
      const float xv = a.x[(n * a.Ws + ws) * a.Hs + hs];
      const float* w = wl + (kw * a.k + kh) * a.Cd + c0;
      acc += f32x4{w[0], w[1], w[2], w[3]} * xv;
    }
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = epilogue(a, acc[j], pos, c0 + j);
  st4(a.y + pos * a.Cd + c0, o);
}

// data gradient into a one-channel input (conv1 -> the mel input): one input position per
// thread, all Cs output channels of every matching output position
__global__ __launch_bounds__(256) void conv2d_direct_dgrad(Conv2 a) {
  __shared__ float wl[DIRECT_W];
  const int nw = a.k * a.k * a.Cs;
  for (int i = threadIdx.x; i < nw; i += 256) wl[i] = a.wk[i];
  __syncthreads();
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pos >= a.M) return;
  const int hd = (int)(pos % a.Hd), wd = (int)((pos / a.Hd) % a.Wd);
  const int64_t n = pos / ((int64_t)a.Hd * a.Wd);
  float acc = 0.f;
  for (int kw = 0; kw < a.k; ++kw)
    for (int kh = 0; kh < a.k; ++kh) {
      int ws, hs;
      if (!tap_src<true>(a, wd, hd, kw, kh, ws, hs)) continue;
      const float* d = a.x + ((n * a.Ws + ws) * a.Hs + hs) * a.Cs;
      const float* w = wl + (kw * a.k + kh) * a.Cs;
      float t = 0.f;  // the tap's channels first, then the running total
      for (int c = 0; c < a.Cs; c += 4) {
        const f32x4 dv = ld4(d + c);
        t += dv.x * w[c] + dv.y * w[c + 1] + dv.z * w[c + 2] + dv.w * w[c + 3];
      }
      acc += t;
    }
  a.y[pos] = a.res ? acc + a.res[pos] : acc;
}

// torch (Co, Ci, kh, kw) -> the kernel layouts above
__global__ void conv2d_weight_prep(const float* w, int Co, int Ci, int k, float* wf, float* wb) {
  const int64_t total = (int64_t)Co * Ci * k * k;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int kw = (int)(e % k), kh = (int)((e / k) % k);
  const int ci = (int)((e / (k * k)) % Ci), co = (int)(e / ((int64_t)k * k * Ci));
  const int tap = kw * k + kh;
  const float v = w[e];
  if (wf) {
    if (Ci % 16 == 0)
      wf[((((int64_t)tap * (Ci / 16) + ci / 16) * 4 + (ci % 16) / 4) * Co + co) * 4 + ci % 4] = v;
    else  // C_in = 1
      wf[(int64_t)tap * Co + co] = v;
  }
  if (wb) {
    if (Ci % 16 == 0)
      wb[((((int64_t)tap * (Co / 16) + co / 16) * 4 + (co % 16) / 4) * Ci + ci) * 4 + co % 4] = v;
    else
      wb[(int64_t)tap * Co + co] = v;
  }
}

// ---------------------------------------------------------------- weight gradient
// dw[co][ci][kh][kw] = sum_p dy[p][co] x[src(p, tap)][ci].  A wave owns one tap, a
// (16 MT) x (16 NT) tile of (co, ci) and one slice of the positions; MFMA K = 4 consecutive
// positions (lane group g takes position p + g).  Slice partials go to ws[slice][tap][co][ci]
// and are added in slice order.  Within a slice the sum is blocked: WG_FLUSH MFMA steps run into
// an inner accumulator that is then added to the slice's total (shorter fma chains).
constexpr int WG_FLUSH = 16;
struct Wgrad2 {
  const float* x;   // (N, Wi, Hi, Ci)
  const float* dy;  // (N, Wo, Ho, Co)
  float* ws;
  int N, Wi, Hi, Ci, Wo, Ho, Co, k, s, pad, splits;
  int64_t M, chunk;  // N * Wo * Ho; positions per slice (a multiple of 4)
};

template <int MT, int NT>
__global__ __launch_bounds__(256) void conv2d_wgrad_mfma(Wgrad2 a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int split = blockIdx.y * 4 + wave;
  if (split >= a.splits) return;  // whole wave
  const int tn = a.Ci / (16 * NT), tm = a.Co / (16 * MT);
  const int tap = blockIdx.x / (tn * tm), tile = blockIdx.x % (tn * tm);
  const int co0 = (tile / tn) * 16 * MT, ci0 = (tile % tn) * 16 * NT;
  const int kw = tap / a.k, kh = tap % a.k;
  f32x4 acc[MT][NT], tot[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = tot[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t p0 = (int64_t)split * a.chunk;
  const int64_t p1 = p0 + a.chunk < a.M ? p0 + a.chunk : a.M;
  int it = 0;
  for (int64_t pb = p0; pb < p1; pb += 4, ++it) {
    if (it == WG_FLUSH) {
      it = 0;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          tot[mt][nt] += acc[mt][nt];
          acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const int64_t p = pb + g;
    const bool live = p < p1;
    const int64_t q = live ? p : 0;
    const int ho = (int)(q % a.Ho), wo = (int)((q / a.Ho) % a.Wo);
    const int64_t n = q / ((int64_t)a.Ho * a.Wo);
    const int wi = wo * a.s - a.pad + kw, hi = ho * a.s - a.pad + kh;
    const bool ok = live && wi >= 0 && wi < a.Wi && hi >= 0 && hi < a.Hi;
    if (!__any(ok)) continue;
    const float* dp = a.dy + q * a.Co + co0 + l15;
    const float* xp = a.x + ((n * a.Wi + (ok ? wi : 0)) * a.Hi + (ok ? hi : 0)) * a.Ci + ci0 + l15;
    float av[MT], bv[NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) av[mt] = ok ? dp[mt * 16] : 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bv[nt] = ok ? xp[nt * 16] : 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
  }
  float* out = a.ws + ((int64_t)split * a.k * a.k + tap) * a.Co * a.Ci;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        out[(int64_t)(co0 + mt * 16 + 4 * g + i) * a.Ci + ci0 + nt * 16 + l15] =
            tot[mt][nt][i] + acc[mt][nt][i];
}

// C_in = 1: one thread per (tap, co), a block per slice, positions in order
__global__ __launch_bounds__(256) void conv2d_wgrad_direct(Wgrad2 a) {
  const int split = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.k * a.k * a.Co) return;
  const int tap = e / a.Co, co = e % a.Co;
  const int kw = tap / a.k, kh = tap % a.k;
  const int64_t p0 = (int64_t)split * a.chunk;
  const int64_t p1 = p0 + a.chunk < a.M ? p0 + a.chunk : a.M;
  float s = 0.f, tot = 0.f;
  for (int64_t p = p0; p < p1; ++p) {
    if (((p - p0) & 63) == 0) {  // blocked summation, 64 positions at a time
      tot += s;
      s = 0.f;
    }
    const int ho = (int)(p % a.Ho), wo = (int)((p / a.Ho) % a.Wo);
    const int64_t n = p / ((int64_t)a.Ho * a.Wo);
    const int wi = wo * a.s - a.pad + kw, hi = ho * a.s - a.pad + kh;
    if (wi < 0 || wi >= a.Wi || hi < 0 || hi >= a.Hi) continue;
    s = fmaf(a.dy[p * a.Co + co], a.x[(n * a.Wi + wi) * a.Hi + hi], s);
  }
  a.ws[(int64_t)split * a.k * a.k * a.Co + e] = tot + s;
}

__global__ void conv2d_wgrad_sum(const float* ws, int splits, int Co, int Ci, int k, int beta,
                                 float* dw) {
  const int64_t total = (int64_t)Co * Ci * k * k;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int kw = (int)(e % k), kh = (int)((e / k) % k);
  const int ci = (int)((e / (k * k)) % Ci), co = (int)(e / ((int64_t)k * k * Ci));
  const int64_t src = ((int64_t)(kw * k + kh) * Co + co) * Ci + ci;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += ws[sp * total + src];
  dw[e] = beta ? dw[e] + s : s;
}

// ---------------------------------------------------------------- BatchNorm2d
// Training statistics over (rows, c) exactly as fs2_bn_fwd documents: per block of BN2_ROWS
// rows its column sum and centred second moment, combined as
//   M2 = sum_b [M2_b + n_b (mean_b - mean)^2]  in block order.
// The lane layout follows the width: c / 4 column groups x 256 / (c / 4) row lanes, so the
// 16-channel layers keep every lane busy.
constexpr int BN2_ROWS = 256;

// sum over the rl row lanes of red[ry * cg + gx] as a fixed binary tree (rl a power of two);
// the result is in red[gx].  Ends with a barrier.
FS2_DEV void lane_tree(f32x4* red, int t, int cg, int rl) {
  __syncthreads();
  for (int half = rl >> 1; half > 0; half >>= 1) {
    if (t < half * cg) red[t] += red[t + half * cg];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void bn2_stats(const float* z, int64_t rows, int c, float* psum,
                                                 float* pm2) {
  __shared__ f32x4 red[256];
  const int cg = c >> 2, rl = 256 / cg;
  const int t = threadIdx.x, gx = t % cg, ry = t / cg;
  const int64_t r0 = (int64_t)blockIdx.x * BN2_ROWS;
  const int64_t r1 = r0 + BN2_ROWS < rows ? r0 + BN2_ROWS : rows;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0 + ry; r < r1; r += rl) s += ld4(z + r * c + 4 * gx);
  red[t] = s;
  lane_tree(red, t, cg, rl);
  const f32x4 tot = red[gx];
  __syncthreads();
  const f32x4 mu = tot / (float)(r1 - r0);
  f32x4 q = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0 + ry; r < r1; r += rl) {
    const f32x4 d = ld4(z + r * c + 4 * gx) - mu;
    q += d * d;
  }
  red[t] = q;
  lane_tree(red, t, cg, rl);
  if (ry == 0) {
    st4(psum + (int64_t)blockIdx.x * c + 4 * gx, tot);
    st4(pm2 + (int64_t)blockIdx.x * c + 4 * gx, red[gx]);
  }
}

__global__ __launch_bounds__(1024) void bn2_stats_final(const float* psum, const float* pm2,
                                                        int64_t nparts, int64_t rows, int c,
                                                        float eps, float mom, float* mean,
                                                        float* rstd, float* rm, float* rv,
                                                        int64_t* nbt) {
  __shared__ float red[32][33];
  __shared__ float mu_s[32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + tx;
  float s = 0.f;
  if (col < c)
    for (int64_t p = ty; p < nparts; p += 32) s += psum[p * c + col];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0) {
    float t = 0.f;
    for (int y = 0; y < 32; ++y) t += red[y][tx];
    mu_s[tx] = t / (float)rows;
  }
  __syncthreads();
  const float mu = mu_s[tx];
  float q = 0.f;
  if (col < c)
    for (int64_t p = ty; p < nparts; p += 32) {
      const int64_t left = rows - p * BN2_ROWS;
      const float n = (float)(left < BN2_ROWS ? left : BN2_ROWS);
      const float d = psum[p * c + col] / n - mu;
      q += pm2[p * c + col] + n * d * d;
    }
  red[ty][tx] = q;
  __syncthreads();
  if (ty != 0 || col >= c) return;
  float t = 0.f;
  for (int y = 0; y < 32; ++y) t += red[y][tx];
  const float var = t / (float)rows;
  mean[col] = mu;
  rstd[col] = 1.f / sqrtf(var + eps);
  if (rm) rm[col] = (1.f - mom) * rm[col] + mom * mu;
  if (rv) rv[col] = (1.f - mom) * rv[col] + mom * (rows > 1 ? t / (float)(rows - 1) : var);
  if (nbt && col == 0) nbt[0] += 1;
}

// out = relu(BN(z) + res), 4 channels per lane
__global__ __launch_bounds__(256) void bn2_apply(const float* z, const float* mean,
                                                 const float* rstd, const float* gamma,
                                                 const float* beta, const float* res, int64_t n4,
                                                 int c, int relu, float* out) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = q * 4;
    const int col = (int)(e0 % c);
    f32x4 v = (ld4(z + e0) - ld4(mean + col)) * ld4(rstd + col) * ld4(gamma + col) + ld4(beta + col);
    if (res) v += ld4(res + e0);
    if (relu) v = f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
    st4(out + e0, v);
  }
}

// eval mode: the per-channel scale and shift the conv epilogue applies
__global__ void bn2_fold(const float* gamma, const float* beta, const float* rm, const float* rv,
                         float eps, int c, float* scale, float* shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  const float sc = gamma[i] / sqrtf(rv[i] + eps);
  scale[i] = sc;
  shift[i] = beta[i] - rm[i] * sc;
}

// backward, pass 1: g = dout * (out > 0) (written out: it is also the residual branch's
// gradient) and the block's column sums of g and g * xhat
__global__ __launch_bounds__(256) void bn2_bwd_partial(const float* dout, const float* out,
                                                       const float* z, const float* mean,
                                                       const float* rstd, int64_t rows, int c,
                                                       int relu, float* gbuf, float* part_g,
                                                       float* part_gx) {
  __shared__ f32x4 red[2][256];
  const int cg = c >> 2, rl = 256 / cg;
  const int t = threadIdx.x, gx = t % cg, ry = t / cg;
  const int64_t r0 = (int64_t)blockIdx.x * BN2_ROWS;
  const int64_t r1 = r0 + BN2_ROWS < rows ? r0 + BN2_ROWS : rows;
  const f32x4 mu = ld4(mean + 4 * gx), rs = ld4(rstd + 4 * gx);
  f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgx = sg;
  for (int64_t r = r0 + ry; r < r1; r += rl) {
    const int64_t e = r * c + 4 * gx;
    f32x4 gv = ld4(dout + e);
    if (relu) {
      const f32x4 o = ld4(out + e);
      gv = f32x4{o.x > 0.f ? gv.x : 0.f, o.y > 0.f ? gv.y : 0.f, o.z > 0.f ? gv.z : 0.f,
                 o.w > 0.f ? gv.w : 0.f};
    }
    st4(gbuf + e, gv);
    sg += gv;
    sgx += gv * ((ld4(z + e) - mu) * rs);
  }
  red[0][t] = sg;
  red[1][t] = sgx;
  lane_tree(red[0], t, cg, rl);
  lane_tree(red[1], t, cg, rl);
  if (ry == 0) {
    st4(part_g + (int64_t)blockIdx.x * c + 4 * gx, red[0][gx]);
    st4(part_gx + (int64_t)blockIdx.x * c + 4 * gx, red[1][gx]);
  }
}

__global__ __launch_bounds__(1024) void bn2_bwd_final(const float* part_g, const float* part_gx,
                                                      int64_t nparts, int c, float* sums,
                                                      float* dgamma, float* dbeta) {
  __shared__ float red[32][2][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + tx;
  float a = 0.f, b = 0.f;
  if (col < c)
    for (int64_t p = ty; p < nparts; p += 32) {
      a += part_g[p * c + col];
      b += part_gx[p * c + col];
    }
  red[ty][0][tx] = a;
  red[ty][1][tx] = b;
  __syncthreads();
  if (ty != 0 || col >= c) return;
  float sg = 0.f, sgx = 0.f;
  for (int y = 0; y < 32; ++y) {
    sg += red[y][0][tx];
    sgx += red[y][1][tx];
  }
  sums[col] = sg;
  sums[c + col] = sgx;
  if (dbeta) dbeta[col] = sg;
  if (dgamma) dgamma[col] = sgx;
}

__global__ __launch_bounds__(256) void bn2_bwd_apply(const float* gbuf, const float* z,
                                                     const float* mean, const float* rstd,
                                                     const float* gamma, const float* sums,
                                                     int64_t n4, int64_t rows, int c, float* dz) {
  const float inv_m = 1.f / (float)rows;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4;
       q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = q * 4;
    const int col = (int)(e0 % c);
    const f32x4 rs = ld4(rstd + col);
    const f32x4 xh = (ld4(z + e0) - ld4(mean + col)) * rs;
    st4(dz + e0, ld4(gamma + col) * rs *
                     (ld4(gbuf + e0) - ld4(sums + col) * inv_m - xh * ld4(sums + c + col) * inv_m));
  }
}

// ---------------------------------------------------------------- pool + dropout + flatten
// out[n][c * H + h] = mean_w x[n, w, h, c] * keep(n * C * H + c * H + h)
__global__ void pool_drop_fwd(const float* x, int64_t N, int W, int H, int C, float p,
                              const uint64_t* seed_p, uint64_t site, float* out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * H * C) return;
  const int c = (int)(idx % C), h = (int)((idx / C) % H);
  const int64_t n = idx / ((int64_t)C * H);
  float s = 0.f;
  for (int w = 0; w < W; ++w) s += x[((n * W + w) * H + h) * C + c];
  const int64_t e = n * C * H + (int64_t)c * H + h;
  const float keep = p > 0.f ? dropout1(*seed_p, site, (uint64_t)e, p) : 1.f;
  out[e] = s / (float)W * keep;
}

__global__ void pool_drop_bwd(const float* dout, int64_t N, int W, int H, int C, float p,
                              const uint64_t* seed_p, uint64_t site, float* dx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * H * C) return;
  const int c = (int)(idx % C), h = (int)((idx / C) % H);
  const int64_t n = idx / ((int64_t)C * H);
  const int64_t e = n * C * H + (int64_t)c * H + h;
  const float keep = p > 0.f ? dropout1(*seed_p, site, (uint64_t)e, p) : 1.f;
  const float v = dout[e] * keep / (float)W;
  for (int w = 0; w < W; ++w) dx[((n * W + w) * H + h) * C + c] = v;
}

// ---------------------------------------------------------------- head at width D
// clf_head_kernel (lstm.hip) with the projection's input width as an argument: one wave per
// row, the same arithmetic and dropout elements.  With `rows` the wave leaves its vectors
// [dp | e | dz0 | a0 | dz1 | a1 | dlogit] for the weight-gradient sums instead of forming dx.
constexpr int HD_MAX = 1024, HD_P = 64, HD_ROW = 6 * HD_P + 4;

struct HeadW {
  const float* x;
  int64_t ldx;
  const float* wp;
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
  int N, D;
  float p_drop;
  const uint64_t* seed;
  uint64_t site;
  float* emb;
  float* logit;
  const float* demb;
  const float* dlogit;
  float* dx;
  int64_t lddx;
  float* rows;
};

__global__ __launch_bounds__(256) void clf_head_w_kernel(HeadW a) {
  __shared__ float xs[4][HD_MAX];
  __shared__ float vs[4][HD_P];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  if (n >= a.N) return;  // whole wave
  const int D = a.D;
  const uint64_t seed = a.seed ? *a.seed : 0ull;
  for (int k = lane; k < D; k += 64) xs[wave][k] = a.x[(int64_t)n * a.ldx + k];
  __builtin_amdgcn_wave_barrier();
  float pa[4] = {a.bp[lane], 0.f, 0.f, 0.f};  // four interleaved chains, added pairwise
  for (int k = 0; k < D; k += 4)
#pragma unroll
    for (int j = 0; j < 4; ++j) pa[j] = fmaf(a.wpt[(k + j) * HD_P + lane], xs[wave][k + j], pa[j]);
  const float p = (pa[0] + pa[1]) + (pa[2] + pa[3]);
  const float nrm = sqrtf(wave_sum(p * p));
  const float e = p / nrm;
  const uint64_t el = (uint64_t)n * (2 * HD_P);
  const float m0 = a.p_drop > 0.f ? dropout1(seed, a.site, el + lane, a.p_drop) : 1.f;
  const float m1 = a.p_drop > 0.f ? dropout1(seed, a.site, el + HD_P + lane, a.p_drop) : 1.f;
  vs[wave][lane] = e;
  __builtin_amdgcn_wave_barrier();
  float z0 = a.b0[lane];
  for (int k = 0; k < HD_P; ++k) z0 = fmaf(a.w0t[k * HD_P + lane], vs[wave][k], z0);
  const float a0 = fmaxf(z0 * m0, 0.f);
  __builtin_amdgcn_wave_barrier();
  vs[wave][lane] = a0;
  __builtin_amdgcn_wave_barrier();
  float z1 = a.b1[lane];
  for (int k = 0; k < HD_P; ++k) z1 = fmaf(a.w1t[k * HD_P + lane], vs[wave][k], z1);
  const float a1 = fmaxf(z1 * m1, 0.f);
  const float lg = wave_sum(a.w2[lane] * a1) + a.b2[0];
  if (a.emb) a.emb[(int64_t)n * HD_P + lane] = e;
  if (a.logit && lane == 0) a.logit[n] = lg;
  if (!a.dx && !a.rows) return;
  // ---- backward
  const float dl = a.dlogit ? a.dlogit[n] : 0.f;
  const float dz1 = (a1 > 0.f ? dl * a.w2[lane] : 0.f) * m1;
  __builtin_amdgcn_wave_barrier();
  vs[wave][lane] = dz1;
  __builtin_amdgcn_wave_barrier();
  float da0 = 0.f;
  for (int o = 0; o < HD_P; ++o) da0 = fmaf(a.w1[o * HD_P + lane], vs[wave][o], da0);
  const float dz0 = (a0 > 0.f ? da0 : 0.f) * m0;
  __builtin_amdgcn_wave_barrier();
  vs[wave][lane] = dz0;
  __builtin_amdgcn_wave_barrier();
  float de = a.demb ? a.demb[(int64_t)n * HD_P + lane] : 0.f;
  for (int o = 0; o < HD_P; ++o) de = fmaf(a.w0[o * HD_P + lane], vs[wave][o], de);
  const float ed = wave_sum(e * de);
  const float dp = (de - e * ed) / nrm;
  if (a.rows) {
    float* r = a.rows + (int64_t)n * HD_ROW;
    r[lane] = dp;
    r[HD_P + lane] = e;
    r[2 * HD_P + lane] = dz0;
    r[3 * HD_P + lane] = a0;
    r[4 * HD_P + lane] = dz1;
    r[5 * HD_P + lane] = a1;
    if (lane == 0) r[6 * HD_P] = dl;
    return;
  }
  __builtin_amdgcn_wave_barrier();
  vs[wave][lane] = dp;
  __builtin_amdgcn_wave_barrier();
  for (int k = lane; k < D; k += 64) {
    float s = 0.f;
    for (int o = 0; o < HD_P; ++o) s = fmaf(a.wp[o * D + k], vs[wave][o], s);
    a.dx[(int64_t)n * a.lddx + k] = s;
  }
}

struct HeadWOut {
  const float* x;
  int64_t ldx;
  const float* rows;
  int N, D, beta;
  float* dwp;
  float* dbp;
  float* dw0;
  float* db0;
  float* dw1;
  float* db1;
  float* dw2;
  float* db2;
};

// every output element one thread that adds the rows in row order (head_wgrad_sum's scheme)
__global__ __launch_bounds__(256) void head_w_wgrad_sum(HeadWOut a) {
  const int P = HD_P, D = a.D;
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * D + P + 2 * (P * P + P) + P + 1) return;
  float* out;
  int ca, cb = -1;
  const float* xr = nullptr;
  if (idx < P * D) {
    out = a.dwp + idx, ca = idx / D, xr = a.x + idx % D;
  } else if ((idx -= P * D) < P) {
    out = a.dbp + idx, ca = idx;
  } else if ((idx -= P) < P * P) {
    out = a.dw0 + idx, ca = 2 * P + idx / P, cb = P + idx % P;
  } else if ((idx -= P * P) < P) {
    out = a.db0 + idx, ca = 2 * P + idx;
  } else if ((idx -= P) < P * P) {
    out = a.dw1 + idx, ca = 4 * P + idx / P, cb = 3 * P + idx % P;
  } else if ((idx -= P * P) < P) {
    out = a.db1 + idx, ca = 4 * P + idx;
  } else if ((idx -= P) < P) {
    out = a.dw2 + idx, ca = 6 * P, cb = 5 * P + idx;
  } else {
    out = a.db2, ca = 6 * P;
  }
  float s = 0.f;
  for (int n = 0; n < a.N; ++n) {
    const float* r = a.rows + (int64_t)n * HD_ROW;
    const float rhs = xr ? xr[(int64_t)n * a.ldx] : cb >= 0 ? r[cb] : 1.f;
    s = fmaf(r[ca], rhs, s);
  }
  *out = a.beta ? *out + s : s;
}

static unsigned ew_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  return (unsigned)(b < 1 ? 1 : b);
}

static int out_extent(int64_t in, int k, int s, int pad) { return (int)((in + 2 * pad - k) / s + 1); }

static int wgrad_splits(int64_t m) {
  int64_t s = (m + 1023) / 1024;
  return (int)(s < 1 ? 1 : s > 1024 ? 1024 : s);
}

template <int MT>
static void wgrad_launch_nt(const Wgrad2& a, int nt, dim3 grid, hipStream_t st) {
  if (nt == 4) conv2d_wgrad_mfma<MT, 4><<<grid, 256, 0, st>>>(a);
  else if (nt == 2) conv2d_wgrad_mfma<MT, 2><<<grid, 256, 0, st>>>(a);
  else conv2d_wgrad_mfma<MT, 1><<<grid, 256, 0, st>>>(a);
}

}  // namespace fs2

using namespace fs2;

extern "C" {

static int conv2d_shape_ok(const char* what, int64_t n, int64_t wi, int64_t hi, int64_t c_in,
                           int64_t c_out, int k, int stride, int pad) {
  FS2_CHECK_ARG(n >= 1 && wi >= 1 && hi >= 1, "%s: empty input (n %lld, w %lld, h %lld)", what,
                (long long)n, (long long)wi, (long long)hi);
  FS2_CHECK_ARG(k >= 1 && k <= 7 && (k & 1) && stride >= 1 && stride <= 2 && pad >= 0 && pad < k,
                "%s: kernel %d, stride %d, pad %d not built", what, k, stride, pad);
  FS2_CHECK_ARG(c_in == 1 || (c_in % 16 == 0 && c_in <= 1024),
                "%s: c_in %lld (1 or a multiple of 16)", what, (long long)c_in);
  FS2_CHECK_ARG(c_out % 16 == 0 && c_out >= 16 && c_out <= 1024,
                "%s: c_out %lld (a multiple of 16)", what, (long long)c_out);
  FS2_CHECK_ARG(c_in != 1 || (int64_t)k * k * c_out <= DIRECT_W,
                "%s: c_in = 1 needs k * k * c_out <= %d", what, DIRECT_W);
  FS2_CHECK_ARG(wi + 2 * pad >= k && hi + 2 * pad >= k, "%s: input smaller than the kernel", what);
  FS2_CHECK_ARG(n * wi * hi < (1ll << 31) / 4, "%s: too many positions", what);
  return FS2_OK;
}

int fs2_conv2d_weight_prep(const float* w, int64_t c_out, int64_t c_in, int k, float* w_fwd,
                           float* w_bwd, void* stream) {
  FS2_CHECK_ARG(w && (w_fwd || w_bwd), "fs2_conv2d_weight_prep: missing operand");
  if (int rc = conv2d_shape_ok("fs2_conv2d_weight_prep", 1, k, k, c_in, c_out, k, 1, k / 2)) return rc;
  const int64_t total = c_out * c_in * k * k;
  conv2d_weight_prep<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(
      w, (int)c_out, (int)c_in, k, w_fwd, w_bwd);
  return launch_status("fs2_conv2d_weight_prep");
}

int fs2_conv2d_fwd(const float* x, int64_t n, int64_t wi, int64_t hi, int64_t c_in,
                   const float* w_fwd, const float* bias, int64_t c_out, int k, int stride, int pad,
                   const float* scale, const float* shift, const float* res, int relu, float* y,
                   void* stream) {
  if (int rc = conv2d_shape_ok("fs2_conv2d_fwd", n, wi, hi, c_in, c_out, k, stride, pad)) return rc;
  FS2_CHECK_ARG(x && w_fwd && y, "fs2_conv2d_fwd: missing operand");
  FS2_CHECK_ARG((scale != nullptr) == (shift != nullptr), "fs2_conv2d_fwd: scale without shift");
  Conv2 a{x, w_fwd, bias, scale, shift, res, y, (int)n, (int)wi, (int)hi, (int)c_in,
          out_extent(wi, k, stride, pad), out_extent(hi, k, stride, pad), (int)c_out, k, stride, pad,
          relu, 0};
  a.M = n * a.Wd * a.Hd;
  hipStream_t st = as_stream(stream);
  if (c_in == 1) {
    conv2d_direct_fwd<<<(unsigned)((a.M * (c_out / 4) + 255) / 256), 256, 0, st>>>(a);
    return launch_status("fs2_conv2d_fwd");
  }
  const int nt = c_out % 64 == 0 ? 4 : c_out % 32 == 0 ? 2 : 1;
  dim3 grid((unsigned)((a.M + 127) / 128), (unsigned)(c_out / (16 * nt)));
  if (nt == 4) conv2d_mfma<4, false><<<grid, 256, 0, st>>>(a);
  else if (nt == 2) conv2d_mfma<2, false><<<grid, 256, 0, st>>>(a);
  else conv2d_mfma<1, false><<<grid, 256, 0, st>>>(a);
  return launch_status("fs2_conv2d_fwd");
}

int fs2_conv2d_dgrad(const float* dy, int64_t n, int64_t wi, int64_t hi, int64_t c_in,
                     const float* w_bwd, int64_t c_out, int k, int stride, int pad,
                     const float* add, float* dx, void* stream) {
  if (int rc = conv2d_shape_ok("fs2_conv2d_dgrad", n, wi, hi, c_in, c_out, k, stride, pad)) return rc;
  FS2_CHECK_ARG(dy && w_bwd && dx, "fs2_conv2d_dgrad: missing operand");
  // source = dy (N, Wo, Ho, Co), destination = dx (N, Wi, Hi, Ci)
  Conv2 a{dy, w_bwd, nullptr, nullptr, nullptr, add, dx, (int)n, out_extent(wi, k, stride, pad),
          out_extent(hi, k, stride, pad), (int)c_out, (int)wi, (int)hi, (int)c_in, k, stride, pad,
          0, n * wi * hi};
  hipStream_t st = as_stream(stream);
  if (c_in == 1) {
    conv2d_direct_dgrad<<<(unsigned)((a.M + 255) / 256), 256, 0, st>>>(a);
    return launch_status("fs2_conv2d_dgrad");
  }
  const int nt = c_in % 64 == 0 ? 4 : c_in % 32 == 0 ? 2 : 1;
  dim3 grid((unsigned)((a.M + 127) / 128), (unsigned)(c_in / (16 * nt)));
  if (nt == 4) conv2d_mfma<4, true><<<grid, 256, 0, st>>>(a);
  else if (nt == 2) conv2d_mfma<2, true><<<grid, 256, 0, st>>>(a);
  else conv2d_mfma<1, true><<<grid, 256, 0, st>>>(a);
  return launch_status("fs2_conv2d_dgrad");
}

int64_t fs2_conv2d_wgrad_ws_bytes(int64_t n, int64_t wi, int64_t hi, int64_t c_in, int64_t c_out,
                                  int k, int stride, int pad) {
  if (n < 1 || wi < 1 || hi < 1 || k < 1 || stride < 1 || wi + 2 * pad < k || hi + 2 * pad < k)
    return 0;
  const int64_t m = n * out_extent(wi, k, stride, pad) * out_extent(hi, k, stride, pad);
  const int64_t slab = (int64_t)wgrad_splits(m) * k * k * c_in * c_out;
  return (slab + ((m + 255) / 256) * c_out) * 4;  // + the bias gradient's column partials
}

int fs2_conv2d_wgrad(const float* x, const float* dy, int64_t n, int64_t wi, int64_t hi,
                     int64_t c_in, int64_t c_out, int k, int stride, int pad, float* dw, float* db,
                     int beta, float* ws, int64_t ws_bytes, void* stream) {
  if (int rc = conv2d_shape_ok("fs2_conv2d_wgrad", n, wi, hi, c_in, c_out, k, stride, pad)) return rc;
  FS2_CHECK_ARG(x && dy && dw && ws, "fs2_conv2d_wgrad: missing operand");
  FS2_CHECK_ARG(beta == 0 || beta == 1, "fs2_conv2d_wgrad: beta %d (0 or 1)", beta);
  FS2_CHECK_ARG(ws_bytes >= fs2_conv2d_wgrad_ws_bytes(n, wi, hi, c_in, c_out, k, stride, pad),
                "fs2_conv2d_wgrad: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  Wgrad2 a{x, dy, ws, (int)n, (int)wi, (int)hi, (int)c_in, out_extent(wi, k, stride, pad),
           out_extent(hi, k, stride, pad), (int)c_out, k, stride, pad, 0, 0, 0};
  a.M = n * a.Wo * a.Ho;
  a.splits = wgrad_splits(a.M);
  a.chunk = ((a.M + a.splits - 1) / a.splits + 3) / 4 * 4;
  const int64_t slab = (int64_t)k * k * c_in * c_out;
  if (c_in == 1) {
    dim3 grid((unsigned)((k * k * c_out + 255) / 256), (unsigned)a.splits);
    conv2d_wgrad_direct<<<grid, 256, 0, st>>>(a);
  } else {
    const int mt = c_out % 64 == 0 ? 4 : c_out % 32 == 0 ? 2 : 1;
    const int nt = c_in % 64 == 0 ? 4 : c_in % 32 == 0 ? 2 : 1;
    dim3 grid((unsigned)(k * k * (c_out / (16 * mt)) * (c_in / (16 * nt))),
              (unsigned)((a.splits + 3) / 4));
    if (mt == 4) wgrad_launch_nt<4>(a, nt, grid, st);
    else if (mt == 2) wgrad_launch_nt<2>(a, nt, grid, st);
    else wgrad_launch_nt<1>(a, nt, grid, st);
  }
  conv2d_wgrad_sum<<<(unsigned)((slab + 255) / 256), 256, 0, st>>>(ws, a.splits, (int)c_out,
                                                                    (int)c_in, k, beta, dw);
  if (db) return colsum_launch(dy, c_out, a.M, c_out, db, beta, ws + a.splits * slab, st);
  return launch_status("fs2_conv2d_wgrad");
}

int64_t fs2_bn2d_ws_bytes(int64_t rows, int64_t c) {
  if (rows < 1 || c < 1) return 0;
  return (2 * ((rows + BN2_ROWS - 1) / BN2_ROWS) * c + 2 * c) * 4;
}

static int bn2d_shape_ok(const char* what, int64_t rows, int64_t c, int64_t ws_bytes) {
  FS2_CHECK_ARG(rows >= 1, "%s: empty input", what);
  FS2_CHECK_ARG(c >= 8 && c % 8 == 0 && c <= 1024 && 256 % (c / 4) == 0,
                "%s: channel count %lld (8, 16, ..., a power of two up to 1024)", what, (long long)c);
  FS2_CHECK_ARG(ws_bytes >= fs2_bn2d_ws_bytes(rows, c), "%s: workspace too small", what);
  return FS2_OK;
}

int fs2_bn2d_fwd(const float* z, int64_t rows, int64_t c, const float* gamma, const float* beta,
                 float eps, float momentum, float* running_mean, float* running_var,
                 int64_t* num_batches_tracked, float* mean, float* rstd, const float* res, int relu,
                 float* out, float* ws, int64_t ws_bytes, void* stream) {
  if (int rc = bn2d_shape_ok("fs2_bn2d_fwd", rows, c, ws_bytes)) return rc;
  FS2_CHECK_ARG(z && gamma && beta && mean && rstd && out && ws, "fs2_bn2d_fwd: missing operand");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const int64_t nparts = (rows + BN2_ROWS - 1) / BN2_ROWS;
  bn2_stats<<<(unsigned)nparts, 256, 0, st>>>(z, rows, (int)c, ws, ws + nparts * c);
  bn2_stats_final<<<(unsigned)((c + 31) / 32), 1024, 0, st>>>(
      ws, ws + nparts * c, nparts, rows, (int)c, eps, momentum, mean, rstd, running_mean,
      running_var, num_batches_tracked);
  bn2_apply<<<ew_blocks(rows * c / 4), 256, 0, st>>>(z, mean, rstd, gamma, beta, res, rows * c / 4,
                                                     (int)c, relu, out);
  return launch_status("fs2_bn2d_fwd");
}

int fs2_bn2d_fold(const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, int64_t c, float* scale, float* shift,
                  void* stream) {
  FS2_CHECK_ARG(c >= 1 && gamma && beta && running_mean && running_var && scale && shift,
                "fs2_bn2d_fold: missing operand");
  bn2_fold<<<(unsigned)((c + 255) / 256), 256, 0, as_stream(stream)>>>(
      gamma, beta, running_mean, running_var, eps, (int)c, scale, shift);
  return launch_status("fs2_bn2d_fold");
}

int fs2_bn2d_bwd(const float* dout, const float* out, const float* z, const float* mean,
                 const float* rstd, const float* gamma, int64_t rows, int64_t c, int relu, float* g,
                 float* dz, float* dgamma, float* dbeta, float* ws, int64_t ws_bytes, void* stream) {
  if (int rc = bn2d_shape_ok("fs2_bn2d_bwd", rows, c, ws_bytes)) return rc;
  FS2_CHECK_ARG(dout && z && mean && rstd && gamma && g && dz && ws && (out || !relu),
                "fs2_bn2d_bwd: missing operand");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const int64_t nparts = (rows + BN2_ROWS - 1) / BN2_ROWS;
  float* part_g = ws;
  float* part_gx = ws + nparts * c;
  float* sums = ws + 2 * nparts * c;
  bn2_bwd_partial<<<(unsigned)nparts, 256, 0, st>>>(dout, out, z, mean, rstd, rows, (int)c, relu, g,
                                                    part_g, part_gx);
  bn2_bwd_final<<<(unsigned)((c + 31) / 32), 1024, 0, st>>>(part_g, part_gx, nparts, (int)c, sums,
                                                           dgamma, dbeta);
  bn2_bwd_apply<<<ew_blocks(rows * c / 4), 256, 0, st>>>(g, z, mean, rstd, gamma, sums,
                                                         rows * c / 4, rows, (int)c, dz);
  return launch_status("fs2_bn2d_bwd");
}

static int pool_shape_ok(const char* what, int64_t n, int64_t w, int64_t h, int64_t c, float p,
                         const uint64_t* seed) {
  FS2_CHECK_ARG(n >= 1 && w >= 1 && h >= 1 && c >= 1 && w < (1 << 24) && h * c < (1 << 24),
                "%s: bad shape (n %lld, w %lld, h %lld, c %lld)", what, (long long)n, (long long)w,
                (long long)h, (long long)c);
  FS2_CHECK_ARG(p >= 0.f && p < 1.f, "%s: dropout %g outside [0, 1)", what, (double)p);
  FS2_CHECK_ARG(p <= 0.f || seed, "%s: dropout needs a seed", what);
  return FS2_OK;
}

int fs2_pool_drop_fwd(const float* x, int64_t n, int64_t w, int64_t h, int64_t c, float p,
                      const uint64_t* seed, uint64_t site, float* out, void* stream) {
  if (int rc = pool_shape_ok("fs2_pool_drop_fwd", n, w, h, c, p, seed)) return rc;
  FS2_CHECK_ARG(x && out, "fs2_pool_drop_fwd: missing operand");
  pool_drop_fwd<<<(unsigned)((n * h * c + 255) / 256), 256, 0, as_stream(stream)>>>(
      x, n, (int)w, (int)h, (int)c, p, seed, site, out);
  return launch_status("fs2_pool_drop_fwd");
}

int fs2_pool_drop_bwd(const float* dout, int64_t n, int64_t w, int64_t h, int64_t c, float p,
                      const uint64_t* seed, uint64_t site, float* dx, void* stream) {
  if (int rc = pool_shape_ok("fs2_pool_drop_bwd", n, w, h, c, p, seed)) return rc;
  FS2_CHECK_ARG(dout && dx, "fs2_pool_drop_bwd: missing operand");
  pool_drop_bwd<<<(unsigned)((n * h * c + 255) / 256), 256, 0, as_stream(stream)>>>(
      dout, n, (int)w, (int)h, (int)c, p, seed, site, dx);
  return launch_status("fs2_pool_drop_bwd");
}

static int head_w_ok(const char* what, int64_t n, int64_t d) {
  FS2_CHECK_ARG(d >= 64 && d % 64 == 0 && d <= HD_MAX, "%s: width %lld (a multiple of 64, <= %d)",
                what, (long long)d, HD_MAX);
  FS2_CHECK_ARG(n >= 0 && n < (1ll << 24), "%s: n %lld", what, (long long)n);
  return FS2_OK;
}

int fs2_clf_head_w(const float* x, int64_t ldx, int64_t n, int64_t d, const float* wp,
                   const float* wpt, const float* bp, const float* w0, const float* w0t,
                   const float* b0, const float* w1, const float* w1t, const float* b1,
                   const float* w2, const float* b2, float p_drop, const uint64_t* seed,
                   uint64_t site, float* emb, float* logit, const float* demb, const float* dlogit,
                   float* dx, int64_t lddx, void* stream) {
  if (int rc = head_w_ok("fs2_clf_head_w", n, d)) return rc;
  FS2_CHECK_ARG(x && wpt && bp && w0t && b0 && w1t && b1 && w2 && b2,
                "fs2_clf_head_w: missing forward operand");
  FS2_CHECK_ARG(!dx || (wp && w0 && w1), "fs2_clf_head_w: backward needs the natural weights");
  FS2_CHECK_ARG(p_drop <= 0.f || seed, "fs2_clf_head_w: dropout needs a seed");
  if (n == 0) return FS2_OK;
  HeadW a{x, ldx, wp, wpt, bp, w0, w0t, b0, w1, w1t, b1, w2, b2, (int)n, (int)d, p_drop, seed, site,
          emb, logit, demb, dlogit, dx, lddx, nullptr};
  clf_head_w_kernel<<<(unsigned)((n + 3) / 4), 256, 0, as_stream(stream)>>>(a);
  return launch_status("fs2_clf_head_w");
}

int64_t fs2_clf_head_w_wgrad_ws_bytes(int64_t n) { return (n < 1 ? 1 : n) * HD_ROW * 4; }

int fs2_clf_head_w_wgrad(const float* x, int64_t ldx, int64_t n, int64_t d, const float* wp,
                         const float* wpt, const float* bp, const float* w0, const float* w0t,
                         const float* b0, const float* w1, const float* w1t, const float* b1,
                         const float* w2, const float* b2, float p_drop, const uint64_t* seed,
                         uint64_t site, const float* demb, const float* dlogit, float* dwp,
                         float* dbp, float* dw0, float* db0, float* dw1, float* db1, float* dw2,
                         float* db2, int beta, float* ws, int64_t ws_bytes, void* stream) {
  if (int rc = head_w_ok("fs2_clf_head_w_wgrad", n, d)) return rc;
  FS2_CHECK_ARG(x && wpt && bp && w0 && w0t && b0 && w1 && w1t && b1 && w2 && b2 && ws,
                "fs2_clf_head_w_wgrad: missing weight operand");
  FS2_CHECK_ARG(dwp && dbp && dw0 && db0 && dw1 && db1 && dw2 && db2,
                "fs2_clf_head_w_wgrad: missing output");
  FS2_CHECK_ARG(p_drop <= 0.f || seed, "fs2_clf_head_w_wgrad: dropout needs a seed");
  FS2_CHECK_ARG(beta == 0 || beta == 1, "fs2_clf_head_w_wgrad: beta %d (0 or 1)", beta);
  FS2_CHECK_ARG(ws_bytes >= fs2_clf_head_w_wgrad_ws_bytes(n),
                "fs2_clf_head_w_wgrad: workspace too small");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  if (n > 0) {
    HeadW a{x, ldx, wp, wpt, bp, w0, w0t, b0, w1, w1t, b1, w2, b2, (int)n, (int)d, p_drop, seed,
            site, nullptr, nullptr, demb, dlogit, nullptr, 0, ws};
    clf_head_w_kernel<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(a);
  }
  HeadWOut o{x, ldx, ws, (int)n, (int)d, beta, dwp, dbp, dw0, db0, dw1, db1, dw2, db2};
  const int outs = HD_P * (int)d + HD_P + 2 * (HD_P * HD_P + HD_P) + HD_P + 1;
  head_w_wgrad_sum<<<(unsigned)((outs + 255) / 256), 256, 0, st>>>(o);
  return launch_status("fs2_clf_head_w_wgrad");
}

}  // extern "C"
