// Arguments and epilogues shared by the forward / data-gradient conv kernels (gemm_glds.hip,
// gemm_tapreg.hip) and their dispatch (conv_dispatch.hip).
#pragma once
#include "glds.hpp"

namespace fs2 {

struct GldsArgs {
  const u16* x;
  int64_t ldx;
  const u16* w;
  void* y;
  int64_t ldy;
  int64_t M, T;
  int Cin, N, taps, pad, K;
  const float* bias;
  int flags;
  const void* aux;
  int64_t ld_aux;
  int tiles_m, tiles_n;
  int vec;    // 8-wide epilogue legal (N, ldy, ld_aux multiples of 8; aligned pointers)
  int group;  // n-tiles per tile group (see the block order below)
  const int64_t* lens;  // optional utterance lengths: all-padding row tiles are not computed
  int dil;              // tap dilation (vocoder convs; 1 elsewhere)
  float alpha, scale;   // FS2_EPI_LRELU slope, FS2_EPI_ACC_Y scale
  u16* y2;              // FS2_EPI_Y2 bf16 output (ld = N)
  float alpha2;
  int kz;               // halo kernel: channel-block splits (0/1 = none; see halo_splitk_reduce)
  float* slab;          // kz > 1: [kz][M][N] fp32 partial products
  // LayerNorm epilogue (fs2_conv_gemm_ln; 256-wide tiles hold whole rows): ln_xhat != NULL.
  // The residual is ln_res (fp32) or, rebuilt per row, ln_res_xhat * ln_res_gamma + ln_res_beta
  // (0 on rows masked by lens); ln_out NULL: no fp32 store
  const float* ln_res;
  const float* ln_gamma;
  const float* ln_beta;
  float* ln_out;
  u16* ln_out_t;
  float* ln_xhat;
  float* ln_rstd;
  const uint64_t* ln_seed;
  uint64_t ln_site;
  float ln_p;
  // LayerNorm-backward epilogue (fs2_conv_gemm_ln_bwd, ln_mode 1): ln_out = dres, ln_out_t =
  // the bf16 dy copy, ln_xhat / ln_rstd read; column partials into ln_part ([4][ln_nblk][256])
  int ln_mode;
  int ln_dres_add;
  float* ln_part;
  int64_t ln_nblk;
  const float* ln_res_xhat;
  const float* ln_res_gamma;
  const float* ln_res_beta;
};

// With lens (all-padding row tiles skipped) the XCD-contiguous tile order would give each XCD
// a contiguous run of utterances, and the XCD holding the longest ones would set the launch
// time.  m-tiles are therefore visited in a stride permutation (tm' -> tm' * s mod tiles_m,
// s ~ tiles_m / 8 coprime with tiles_m): each XCD's contiguous run of tm' lands on m-tiles
// spread over the whole batch.  Every n-tile of an m-tile stays on one XCD (A-row reuse).
FS2_DEV int igcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

FS2_DEV int m_interleave(int tm, int tiles_m, bool on) {
  if (!on || tiles_m < 16) return tm;
  int s = tiles_m / 8 + 1;
  while (igcd(s, tiles_m) != 1) ++s;
  return (int)(((int64_t)tm * s) % tiles_m);
}

// LayerNorm epilogue of a 256-wide tile (whole rows): the fs2_ln_fwd row computation on the
// accumulators instead of a stored fp32 y -- z = dropout(acc + bias, p) + res, mean / variance
// over the half-wave's 256 channels (8 per lane, the fs2_ln_fwd lane layout), out = xhat *
// gamma + beta, padded rows written as 0 (xhat / rstd not written there: the backward skips
// them).  Same operations in the same order as fs2_conv_gemm + fs2_ln_fwd: bitwise equal.
// A normalised residual (ln_res_xhat) is read only on the rows that pass the lens test: its
// producer left xhat unwritten on the others, where the residual is 0.
template <int BM, int NWAVE, int WN>
FS2_DEV void nt_epilogue_ln(const GldsArgs& a, f32x4 (&acc)[BM / 32][256 / WN / 16], u16* smem,
                            int64_t m0, bool skip, int tid, int wm, int wn, int g, int r16) {
  constexpr int MI = BM / 32, NI = 256 / WN / 16, EPI_LD = 256 + 4;
  constexpr int RPP = NWAVE * 2;  // rows per pass: one per half-wave
  float* Cs = reinterpret_cast<float*>(smem);
  const int hl = tid & 31;
  const uint64_t seed = a.ln_seed ? *a.ln_seed : 0ull;
  const f32x4 ga0 = ld4(a.ln_gamma + 8 * hl), ga1 = ld4(a.ln_gamma + 8 * hl + 4);
  const f32x4 be0 = ld4(a.ln_beta + 8 * hl), be1 = ld4(a.ln_beta + 8 * hl + 4);
  f32x4 rg0 = f32x4{0.f, 0.f, 0.f, 0.f}, rg1 = rg0, rb0 = rg0, rb1 = rg0;
  if (a.ln_res_xhat && !skip) {
    rg0 = ld4(a.ln_res_gamma + 8 * hl);
    rg1 = ld4(a.ln_res_gamma + 8 * hl + 4);
    rb0 = ld4(a.ln_res_beta + 8 * hl);
    rb1 = ld4(a.ln_res_beta + 8 * hl + 4);
  }
  f32x4 bi0 = f32x4{0.f, 0.f, 0.f, 0.f}, bi1 = bi0;
  if ((a.flags & FS2_EPI_BIAS) && !skip) {
    bi0 = ld4(a.bias + 8 * hl);
    bi1 = ld4(a.bias + 8 * hl + 4);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (wm == h) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(i * 16 + 4 * g + r) * EPI_LD + wn * (256 / WN) + j * 16 + r16] = acc[i][j][r];
    }
    epi_barrier();
#pragma unroll
    for (int p = 0; p < (BM / 2) / RPP; ++p) {
      const int rr = p * RPP + (tid >> 5);
      const int64_t m = m0 + h * (BM / 2) + rr;
      if (m >= a.M) continue;  // half-wave uniform
      const int64_t e0 = m * 256 + 8 * hl;
      const bool pad = a.lens && (m % a.T) >= a.lens[m / a.T];
      if (pad) {
        const f32x4 zz = {0.f, 0.f, 0.f, 0.f};
        if (a.ln_out) {
          st4(a.ln_out + e0, zz);
          st4(a.ln_out + e0 + 4, zz);
        }
        if (a.ln_out_t) st8_bf16(a.ln_out_t + e0, zz, zz);
        continue;
      }
      f32x4 z0 = *reinterpret_cast<const f32x4*>(Cs + rr * EPI_LD + 8 * hl);
      f32x4 z1 = *reinterpret_cast<const f32x4*>(Cs + rr * EPI_LD + 8 * hl + 4);
      z0 += bi0;
      z1 += bi1;
      if (a.ln_p > 0.f) {
        f32x4 k0, k1;
        dropout8(seed, a.ln_site, (uint64_t)e0, a.ln_p, k0, k1);
        z0 *= k0;
        z1 *= k1;
      }
      if (a.ln_res) {
        z0 += ld4(a.ln_res + e0);
        z1 += ld4(a.ln_res + e0 + 4);
      } else if (a.ln_res_xhat) {  // this row is valid (the padded ones left above)
        z0 += ln_affine(ld4(a.ln_res_xhat + e0), rg0, rb0);
        z1 += ln_affine(ld4(a.ln_res_xhat + e0 + 4), rg1, rb1);
      }
      const float mean =
          half_sum((z0.x + z0.y + z0.z + z0.w) + (z1.x + z1.y + z1.z + z1.w)) * (1.f / 256);
      const f32x4 c0 = z0 - mean, c1 = z1 - mean;
      const float var = half_sum((c0.x * c0.x + c0.y * c0.y + c0.z * c0.z + c0.w * c0.w) +
                                 (c1.x * c1.x + c1.y * c1.y + c1.z * c1.z + c1.w * c1.w)) *
                        (1.f / 256);
      const float rs = 1.f / sqrtf(var + 1e-5f);
      const f32x4 xh0 = c0 * rs, xh1 = c1 * rs;
      const f32x4 u0 = ln_affine(xh0, ga0, be0), u1 = ln_affine(xh1, ga1, be1);
      if (a.ln_out) {
        st4(a.ln_out + e0, u0);
        st4(a.ln_out + e0 + 4, u1);
      }
      if (a.ln_out_t) st8_bf16(a.ln_out_t + e0, u0, u1);
      st4(a.ln_xhat + e0, xh0);
      st4(a.ln_xhat + e0 + 4, xh1);
      if (hl == 0) a.ln_rstd[m] = rs;
    }
    epi_barrier();
  }
}

// LayerNorm-BACKWARD epilogue of a 256-wide tile: the GEMM's rows are the upstream gradient of
// a LayerNorm (dout = acc + aux, the residual-gradient add of fs2_conv_gemm's FS2_EPI_ADD_AUX),
// and fs2_ln_bwd's row computation runs on them: dz = rstd (g dout - mean(g dout) - xhat
// mean(g dout xhat)) into dres (written, or added with dres_add), dy = dz * dropout_in into the
// bf16 copy, padded rows zero.  Each 32-row half of the tile is one fs2_ln_bwd block: its
// column partials of dout xhat, dout and dy (dgamma, dbeta, the fused bias gradient) are summed
// over the 8 half-waves in a fixed order into ln_part, reduced by fs2_ln_bwd_final.
template <int BM, int NWAVE, int WN>
FS2_DEV void nt_epilogue_lnbwd(const GldsArgs& a, f32x4 (&acc)[BM / 32][256 / WN / 16], u16* smem,
                               int64_t m0, int tid, int wm, int wn, int g, int r16) {
  static_assert(BM / 2 == 32 && NWAVE == 4, "one 32-row LayerNorm block per tile half");
  constexpr int MI = BM / 32, NI = 256 / WN / 16, EPI_LD = 256 + 4;
  float* Cs = reinterpret_cast<float*>(smem);
  f32x4* red = reinterpret_cast<f32x4*>(Cs + 32 * EPI_LD);  // [3 kinds][8 half-waves][64]
  const int hl = tid & 31, hw = tid >> 5;
  const bool use_aux = a.flags & FS2_EPI_ADD_AUX;
  const uint64_t seed = a.ln_seed ? *a.ln_seed : 0ull;
  const f32x4 gam0 = ld4(a.ln_gamma + 8 * hl), gam1 = ld4(a.ln_gamma + 8 * hl + 4);
  const f32x4 zz = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (wm == h) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(i * 16 + 4 * g + r) * EPI_LD + wn * (256 / WN) + j * 16 + r16] = acc[i][j][r];
    }
    epi_barrier();
    f32x4 pg0 = zz, pg1 = zz, pb0 = zz, pb1 = zz, py0 = zz, py1 = zz;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int rr = hw + 8 * p;
      const int64_t m = m0 + h * 32 + rr;
      if (m >= a.M) continue;  // half-wave uniform
      const int64_t e0 = m * 256 + 8 * hl;
      const bool pad = a.lens && (m % a.T) >= a.lens[m / a.T];
      if (pad) {  // masked row: zero upstream gradient
        if (!a.ln_dres_add) {
          st4(a.ln_out + e0, zz);
          st4(a.ln_out + e0 + 4, zz);
        }
        if (a.ln_out_t) st8_bf16(a.ln_out_t + e0, zz, zz);
        continue;
      }
      f32x4 du0 = *reinterpret_cast<const f32x4*>(Cs + rr * EPI_LD + 8 * hl);
      f32x4 du1 = *reinterpret_cast<const f32x4*>(Cs + rr * EPI_LD + 8 * hl + 4);
      if (use_aux) {
        const float* ap = (const float*)a.aux + m * a.ld_aux + 8 * hl;
        du0 += ld4(ap);
        du1 += ld4(ap + 4);
      }
      const f32x4 xh0 = ld4(a.ln_xhat + e0), xh1 = ld4(a.ln_xhat + e0 + 4);
      pg0 += du0 * xh0;
      pg1 += du1 * xh1;
      pb0 += du0;
      pb1 += du1;
      const f32x4 dxh0 = du0 * gam0, dxh1 = du1 * gam1;
      const float m1 = half_sum((dxh0.x + dxh0.y + dxh0.z + dxh0.w) + (dxh1.x + dxh1.y + dxh1.z + dxh1.w)) *
                       (1.f / 256);
      const float m2 = half_sum((dxh0.x * xh0.x + dxh0.y * xh0.y + dxh0.z * xh0.z + dxh0.w * xh0.w) +
                                (dxh1.x * xh1.x + dxh1.y * xh1.y + dxh1.z * xh1.z + dxh1.w * xh1.w)) *
                       (1.f / 256);
      const float rs = a.ln_rstd[m];
      const f32x4 dz0 = rs * (dxh0 - m1 - xh0 * m2), dz1 = rs * (dxh1 - m1 - xh1 * m2);
      st4(a.ln_out + e0, a.ln_dres_add ? ld4(a.ln_out + e0) + dz0 : dz0);
      st4(a.ln_out + e0 + 4, a.ln_dres_add ? ld4(a.ln_out + e0 + 4) + dz1 : dz1);
      f32x4 dy0 = dz0, dy1 = dz1;
      if (a.ln_p > 0.f) {
        f32x4 mi0, mi1;
        dropout8(seed, a.ln_site, (uint64_t)e0, a.ln_p, mi0, mi1);
        dy0 *= mi0;
        dy1 *= mi1;
      }
      if (a.ln_out_t) st8_bf16(a.ln_out_t + e0, dy0, dy1);
      py0 += dy0;
      py1 += dy1;
    }
    const int64_t blk = (m0 + h * 32) / 32;
    const bool live = m0 + h * 32 < a.M;  // block-uniform
    red[(0 * 8 + hw) * 64 + 2 * hl] = pg0;
    red[(0 * 8 + hw) * 64 + 2 * hl + 1] = pg1;
    red[(1 * 8 + hw) * 64 + 2 * hl] = pb0;
    red[(1 * 8 + hw) * 64 + 2 * hl + 1] = pb1;
    red[(2 * 8 + hw) * 64 + 2 * hl] = py0;
    red[(2 * 8 + hw) * 64 + 2 * hl + 1] = py1;
    epi_barrier();
    if (live && tid < 3 * 64) {  // waves 0-2: one kind each, the 8 half-waves in order
      const int kind = tid >> 6, q = tid & 63;
      f32x4 s = red[(kind * 8) * 64 + q];
#pragma unroll
      for (int k = 1; k < 8; ++k) s += red[(kind * 8 + k) * 64 + q];
      const int slot = kind == 2 ? 3 : kind;  // fs2_ln_bwd's part layout: dgamma, dbeta, -, dbias
      st4(a.ln_part + ((int64_t)slot * a.ln_nblk + blk) * 256 + 4 * q, s);
    }
    epi_barrier();
  }
}

// Epilogue through LDS, one half of the tile's rows at a time: bias, aux add, ReLU / ReLU-mask,
// bf16 cast on 8-element row vectors (16-B / 32-B coalesced stores).  Shared by the NT kernels.
// WM waves per column of the tile (each BM / WM rows, MI = BM / WM / 16 fragments; WM / 2 per
// half).  SROW > 0 (conv_gemm_tapreg): fragment i of a wave holds the rows i + SROW * m
// (m = 0..15) of its band; the fragments are staged as usual and the store pass maps each
// output row back to its (fragment, m) slot.
template <int BM, int BN, bool VOC, int NWAVE = 4, int WN = 2, int WM = 2, int SROW = 0,
          bool BF16D = false>
FS2_DEV void nt_epilogue(const GldsArgs& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16], u16* smem,
                         int64_t m0, int n0, bool skip, int tid, int wm, int wn, int g, int r16) {
  constexpr int MI = BM / WM / 16, NI = BN / WN / 16;
  constexpr int WR = BM / WM, WPH = WM / 2;  // rows per wave, waves per half
  static_assert(WM % 2 == 0 && (SROW == 0 || MI % SROW == 0), "epilogue layout");
  constexpr int EPI_LD = BN + 4;
  if constexpr (BN == 256 && !VOC && WM == 2 && SROW == 0) {
    if (a.ln_xhat) {
      if constexpr (BM == 64) {
        if (a.ln_mode == 1) {
          nt_epilogue_lnbwd<BM, NWAVE, WN>(a, acc, smem, m0, tid, wm, wn, g, r16);
          return;
        }
      }
      nt_epilogue_ln<BM, NWAVE, WN>(a, acc, smem, m0, skip, tid, wm, wn, g, r16);
      return;
    }
  }
  if (skip && (a.flags & FS2_EPI_SKIP_NOSTORE)) return;  // block-uniform
  if constexpr (BF16D && !VOC) {
    // bf16 output with a column-only epilogue (bias, ReLU): applied in the accumulator layout
    // (the bias of a lane's column is one value per 16-column fragment), rounded to bf16 and
    // written to LDS as ONE whole tile -- half the LDS bytes of the fp32 half-tile passes and a
    // single barrier -- then stored as 16-B row vectors.  Same operations per element: bitwise
    // equal to the fp32 path below.
    constexpr int LDB = BN + 4;  // u16 row stride: 8 B pad
    static_assert(BM * LDB <= (BM / 2) * (BN + 4) * 2, "bf16 tile fits the epilogue region");
    const bool rmask = (a.flags & FS2_EPI_RELU_MASK_AUX) && (a.flags & FS2_EPI_AUX_BF16);
    if (a.vec && (a.flags & FS2_EPI_OUT_BF16) && !(a.flags & FS2_EPI_ADD_AUX) &&
        (rmask || !(a.flags & FS2_EPI_RELU_MASK_AUX))) {
      constexpr int TPR = BN / 8, RPP = NWAVE * 64 / TPR, NPB = BM / RPP, NPF = NPB / 2;
      const int cc = (tid % TPR) * 8;
      const int n = n0 + cc;
      // ReLU mask (bf16 aux > 0): applied to the bf16 row vectors -- rounding 0 gives 0, so the
      // mask commutes with the rounding.  The first half of the passes' aux rows is loaded
      // before the LDS write, the second half one pass ahead of its use.
      uint4 am[NPB];
      if (rmask) {
#pragma unroll
        for (int p = 0; p < NPF; ++p) {
          const int64_t m = m0 + p * RPP + tid / TPR;
          am[p] = m < a.M && n < a.N ? *reinterpret_cast<const uint4*>((const u16*)a.aux + m * a.ld_aux + n)
                                      : uint4{0u, 0u, 0u, 0u};
        }
      }
      const bool relu = a.flags & FS2_EPI_RELU;
      const bool bias = (a.flags & FS2_EPI_BIAS) && !skip;
      float bj[NI];
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int col = n0 + wn * (BN / WN) + j * 16 + r16;
        bj[j] = bias && col < a.N ? a.bias[col] : 0.f;
      }
      u16* Cb = smem;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = acc[i][j][r];
            if (bias) v += bj[j];
            if (relu) v = fmaxf(v, 0.f);
            // output row of accumulator (i, 4g + r): SROW > 0 (conv_gemm_tapreg) holds rows
            // i % SROW + SROW * m of the wave's band i / SROW (see below)
            const int row = SROW > 0 ? wm * WR + (i / (SROW > 0 ? SROW : 1)) * 16 * SROW +
                                           i % (SROW > 0 ? SROW : 1) + SROW * (4 * g + r)
                                     : wm * WR + i * 16 + 4 * g + r;
            Cb[row * LDB + wn * (BN / WN) + j * 16 + r16] = to_bf16(v);
          }
      epi_barrier();
#pragma unroll
      for (int p = 0; p < NPB; ++p) {
        if (rmask && p + NPF < NPB) {
          const int64_t m = m0 + (p + NPF) * RPP + tid / TPR;
          am[p + NPF] = m < a.M && n < a.N
                            ? *reinterpret_cast<const uint4*>((const u16*)a.aux + m * a.ld_aux + n)
                            : uint4{0u, 0u, 0u, 0u};
        }
        const int rr = p * RPP + tid / TPR;
        const int64_t m = m0 + rr;
        if (m >= a.M || n >= a.N) continue;
        uint4 o = *reinterpret_cast<const uint4*>(Cb + rr * LDB + cc);
        if (rmask) {  // keep each bf16 half where its aux half is > 0: sign clear, 0 < |x| <= inf
          auto pos = [](uint32_t h) { return (h & 0x8000u) == 0 && (h & 0x7fffu) != 0 && (h & 0x7fffu) <= 0x7f80u; };
          auto keep = [&](uint32_t y, uint32_t x) {
            return y & ((pos(x & 0xffffu) ? 0x0000ffffu : 0u) | (pos(x >> 16) ? 0xffff0000u : 0u));
          };
          o.x = keep(o.x, am[p].x);
          o.y = keep(o.y, am[p].y);
          o.z = keep(o.z, am[p].z);
          o.w = keep(o.w, am[p].w);
        }
        *reinterpret_cast<uint4*>((u16*)a.y + m * a.ldy + n) = o;
      }
      epi_barrier();
      return;
    }
  }
  float* Cs = reinterpret_cast<float*>(smem);
  const bool out_bf16 = a.flags & FS2_EPI_OUT_BF16, aux_bf16 = a.flags & FS2_EPI_AUX_BF16;
  constexpr int TPR = BN / 8;            // threads per row
  constexpr int RPP = NWAVE * 64 / TPR;  // rows per pass
  constexpr int NP = (BM / 2) / RPP;     // passes per half
  const int cc = (tid % TPR) * 8;
  const int n = n0 + cc;
  // The bias (the same 8 columns in every pass) and a half's aux rows are loaded BEFORE the
  // half's LDS write: their latency then overlaps it.  Loaded inside each pass, they put a
  // dependent global load between the pass's LDS read and its store, four passes in series
  // (k = 1 QKV projection: 28.5 us with, 15.1 us without the epilogue; its LDS transpose
  // alone costs 2.4 us and its stores alone 4.1 us; profiles/r4_ab_experiments.txt).
  // (fp32 aux rows only where a half has at most two passes: four would cost 32 registers)
  constexpr bool PF32 = NP <= 2;
  const bool pf = !VOC && a.vec && n < a.N;
  const bool pf_aux = pf && (a.flags & (FS2_EPI_ADD_AUX | FS2_EPI_RELU_MASK_AUX)) &&
                      (aux_bf16 || PF32);
  f32x4 bz0 = f32x4{0.f, 0.f, 0.f, 0.f}, bz1 = bz0;
  if (pf && (a.flags & FS2_EPI_BIAS) && !skip) {
    bz0 = *reinterpret_cast<const f32x4*>(a.bias + n);
    bz1 = *reinterpret_cast<const f32x4*>(a.bias + n + 4);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint4 araw[NP][PF32 ? 2 : 1];  // aux rows of this half: bf16 in [p][0], fp32 in [p][0..1]
    if (pf_aux) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int64_t m = m0 + h * (BM / 2) + p * RPP + tid / TPR;
#pragma unroll
        for (int q = 0; q < (PF32 ? 2 : 1); ++q) araw[p][q] = uint4{0u, 0u, 0u, 0u};
        if (m < a.M) {
          if (aux_bf16) {
            araw[p][0] = *reinterpret_cast<const uint4*>((const u16*)a.aux + m * a.ld_aux + n);
          } else if constexpr (PF32) {
            const uint4* ap = reinterpret_cast<const uint4*>((const float*)a.aux + m * a.ld_aux + n);
            araw[p][0] = ap[0];
            araw[p][1] = ap[1];
          }
        }
      }
    }
    if (wm / WPH == h) {
      const int rb = (wm % WPH) * WR;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(rb + i * 16 + 4 * g + r) * EPI_LD + wn * (BN / WN) + j * 16 + r16] = acc[i][j][r];
    }
    epi_barrier();
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int rr = p * RPP + tid / TPR;
      const int64_t m = m0 + h * (BM / 2) + rr;
      if (m >= a.M || n >= a.N) continue;
      int rq = rr;
      if constexpr (SROW > 0) {  // row b + i + SROW * q of a band of 16 * SROW rows
        const int w = rr / WR, rw = rr % WR, bnd = rw / (16 * SROW), rb2 = rw % (16 * SROW);
        rq = w * WR + (bnd * SROW + rb2 % SROW) * 16 + rb2 / SROW;
      }
      float v[8];
      const f32x4 lo = *reinterpret_cast<const f32x4*>(Cs + rq * EPI_LD + cc);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(Cs + rq * EPI_LD + cc + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = lo[e];
        v[e + 4] = hi[e];
      }
      if (a.vec) {
        if ((a.flags & FS2_EPI_BIAS) && !skip) {
          const f32x4 b0 = pf ? bz0 : *reinterpret_cast<const f32x4*>(a.bias + n);
          const f32x4 b1 = pf ? bz1 : *reinterpret_cast<const f32x4*>(a.bias + n + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] += b0[e];
            v[e + 4] += b1[e];
          }
        }
        float av[8];
        if (pf_aux) {
          if (aux_bf16) {
            const uint4 raw = araw[p][0];
            const uint32_t wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              av[2 * e] = __uint_as_float(wv[e] << 16);
              av[2 * e + 1] = __uint_as_float(wv[e] & 0xffff0000u);
            }
          } else if constexpr (PF32) {
            const uint4 r0 = araw[p][0], r1 = araw[p][1];
            av[0] = __uint_as_float(r0.x); av[1] = __uint_as_float(r0.y);
            av[2] = __uint_as_float(r0.z); av[3] = __uint_as_float(r0.w);
            av[4] = __uint_as_float(r1.x); av[5] = __uint_as_float(r1.y);
            av[6] = __uint_as_float(r1.z); av[7] = __uint_as_float(r1.w);
          }
        } else if (a.flags & (FS2_EPI_ADD_AUX | FS2_EPI_RELU_MASK_AUX)) {
          if (aux_bf16) {
            const uint4 raw = *reinterpret_cast<const uint4*>((const u16*)a.aux + m * a.ld_aux + n);
            const uint32_t wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              av[2 * e] = __uint_as_float(wv[e] << 16);
              av[2 * e + 1] = __uint_as_float(wv[e] & 0xffff0000u);
            }
          } else {
            const float* ap = (const float*)a.aux + m * a.ld_aux + n;
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(ap + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              av[e] = a0[e];
              av[e + 4] = a1[e];
            }
          }
        }
        float yo[8];
        if (VOC && (a.flags & FS2_EPI_ACC_Y)) {
          if (out_bf16) {
            const uint4 raw = *reinterpret_cast<const uint4*>((const u16*)a.y + m * a.ldy + n);
            const uint32_t wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              yo[2 * e] = __uint_as_float(wv[e] << 16);
              yo[2 * e + 1] = __uint_as_float(wv[e] & 0xffff0000u);
            }
          } else {
            const float* yp = (const float*)a.y + m * a.ldy + n;
            const f32x4 y0 = *reinterpret_cast<const f32x4*>(yp);
            const f32x4 y1 = *reinterpret_cast<const f32x4*>(yp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              yo[e] = y0[e];
              yo[e + 4] = y1[e];
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (a.flags & FS2_EPI_ADD_AUX) v[e] += av[e];
          if (VOC && (a.flags & FS2_EPI_ACC_Y)) v[e] = (v[e] + yo[e]) * a.scale;
          if (a.flags & FS2_EPI_RELU) v[e] = fmaxf(v[e], 0.f);
          if (VOC && (a.flags & FS2_EPI_LRELU)) v[e] = v[e] >= 0.f ? v[e] : a.alpha * v[e];
          if (a.flags & FS2_EPI_RELU_MASK_AUX) v[e] = av[e] > 0.f ? v[e] : 0.f;
        }
        if (VOC && (a.flags & FS2_EPI_Y2)) {
          float w2[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) w2[e] = v[e] >= 0.f ? v[e] : a.alpha2 * v[e];
          uint4 o;
          o.x = (uint32_t)to_bf16(w2[0]) | ((uint32_t)to_bf16(w2[1]) << 16);
          o.y = (uint32_t)to_bf16(w2[2]) | ((uint32_t)to_bf16(w2[3]) << 16);
          o.z = (uint32_t)to_bf16(w2[4]) | ((uint32_t)to_bf16(w2[5]) << 16);
          o.w = (uint32_t)to_bf16(w2[6]) | ((uint32_t)to_bf16(w2[7]) << 16);
          *reinterpret_cast<uint4*>(a.y2 + m * a.N + n) = o;
        }
        if (VOC && !a.y) continue;
        if (out_bf16) {
          uint4 o;
          o.x = (uint32_t)to_bf16(v[0]) | ((uint32_t)to_bf16(v[1]) << 16);
          o.y = (uint32_t)to_bf16(v[2]) | ((uint32_t)to_bf16(v[3]) << 16);
          o.z = (uint32_t)to_bf16(v[4]) | ((uint32_t)to_bf16(v[5]) << 16);
          o.w = (uint32_t)to_bf16(v[6]) | ((uint32_t)to_bf16(v[7]) << 16);
          *reinterpret_cast<uint4*>((u16*)a.y + m * a.ldy + n) = o;
        } else {
          float* yp = (float*)a.y + m * a.ldy + n;
          *reinterpret_cast<f32x4*>(yp) = f32x4{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(yp + 4) = f32x4{v[4], v[5], v[6], v[7]};
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (n + e >= a.N) break;
          float x = v[e];
          if ((a.flags & FS2_EPI_BIAS) && !skip) x += a.bias[n + e];
          float av = 0.f;
          if (a.flags & (FS2_EPI_ADD_AUX | FS2_EPI_RELU_MASK_AUX))
            av = aux_bf16 ? bf2f(((const u16*)a.aux)[m * a.ld_aux + n + e])
                          : ((const float*)a.aux)[m * a.ld_aux + n + e];
          if (a.flags & FS2_EPI_ADD_AUX) x += av;
          if (VOC && (a.flags & FS2_EPI_ACC_Y))
            x = (x + (out_bf16 ? bf2f(((const u16*)a.y)[m * a.ldy + n + e])
                               : ((const float*)a.y)[m * a.ldy + n + e])) * a.scale;
          if (a.flags & FS2_EPI_RELU) x = fmaxf(x, 0.f);
          if (VOC && (a.flags & FS2_EPI_LRELU)) x = x >= 0.f ? x : a.alpha * x;
          if (a.flags & FS2_EPI_RELU_MASK_AUX) x = av > 0.f ? x : 0.f;
          if (VOC && (a.flags & FS2_EPI_Y2)) a.y2[m * a.N + n + e] = to_bf16(x >= 0.f ? x : a.alpha2 * x);
          if (VOC && !a.y) continue;
          if (out_bf16) ((u16*)a.y)[m * a.ldy + n + e] = to_bf16(x);
          else ((float*)a.y)[m * a.ldy + n + e] = x;
        }
      }
    }
    epi_barrier();
  }
}

// K1: taps == 1 and K % 64 == 0 (the Linear / 1x1 projections) -- A and B stage through buffer
// descriptors based at the tile's first row: per-lane 32-bit offsets fixed over the k loop, the
// k-step in the scalar offset, rows past M / N out of the descriptors' range (zeros).
// (the K1 128 x 128 one-stage build, the projections' workhorse, is held to three blocks per CU)
// One launcher per kernel family: each maps a plan (conv_plan.hpp) to its template instance and
// launches it.  A plan no instance is built for is an error of the call, never another kernel.
struct ConvPlan;
int launch_conv_nt(const ConvPlan& p, const GldsArgs& a, hipStream_t st);      // gemm_glds.hip
int launch_conv_halo(const ConvPlan& p, GldsArgs& a, hipStream_t st);          // gemm_glds.hip
int launch_conv_tapreg(const ConvPlan& p, const GldsArgs& a, hipStream_t st);  // gemm_tapreg.hip

}  // namespace fs2
