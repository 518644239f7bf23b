// Which kernel a bf16 fs2_conv_gemm* / fs2_conv_wgrad* call runs: the one place that decides.
//
// plan_conv_gemm / plan_conv_gemm_ln / plan_conv_wgrad / plan_wgrad_k1_multi map a shape, the
// tuning knobs and the CU count to a plan: kernel family, the template parameters chosen at run
// time, the tiling, the grid and the reduce that follows.  The launchers (conv_dispatch.hip and
// one function per kernel family) only turn a plan into a launch; the workspace size queries
// call the same functions, so size and choice cannot drift apart.  fs2_debug_conv_plan prints
// a plan.  Host-only and HIP-free (plain C++17): no locks, no allocation, no device queries.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/fs2hip.h"

namespace fs2 {

// ------------------------------------------------------------------ forward / data gradient
enum ConvKernel { CONV_NT = 0, CONV_HALO = 1, CONV_TAPREG = 2 };

struct ConvShape {
  int64_t rows, seq_len, c_in, c_out;
  int taps, pad, dilation, flags;
  bool has_lens;
  bool has_y;  // a y output exists (the vocoder's Y2-only calls have none)
  bool vec;    // 8-wide epilogue legal: c_out, ldy, ld_aux multiples of 8; y, bias, aux, y2 16-B aligned
};

struct ConvPlan {
  int kernel;                          // ConvKernel
  int bm, bn, stages, hx, waves, taps; // template parameters chosen at run time
  bool k1, tapaligned, voc, pipe;
  int tiles_m, tiles_n, group, kz;
  unsigned grid, block;                // grid: tiles_m * tiles_n * kz workgroups of `block` threads
  int reduce_bm;                       // kz > 1: halo_splitk_reduce<reduce_bm> follows
  unsigned reduce_grid;
};

// n-tiles per tile group of the halo kernels (FS2_TUNE_NT_GROUP; default: all of them)
inline int halo_group(int tiles_n, const int* tune) {
  const int g = tune[FS2_TUNE_NT_GROUP];
  return g > 0 && g < tiles_n ? g : tiles_n;
}

// Split-K choice for the halo kernel.  A grid below ~3 blocks per CU with a long channel loop
// (the encoder's k=9 data gradient: 384 tiles, 16 channel blocks x 9 taps each) leaves CUs with
// one block and the rest with two; splitting the channel blocks kz ways fills the chip and
// halves each block's serial loop, at the cost of kz fp32 partial products summed by
// halo_splitk_reduce.  The decomposition is a function of the shape alone: no stream, capture
// or allocation state can change it, so every call of a shape sums in one fp32 order.
inline int halo_splitk_count(const ConvShape& s, const int* tune, unsigned grid, bool voc, bool hx64) {
  const int knob = tune[FS2_TUNE_HALO_SPLITK];
  const int ncb = (int)s.c_in / 64;
  const int keep = FS2_EPI_BIAS | FS2_EPI_RELU | FS2_EPI_ADD_AUX | FS2_EPI_RELU_MASK_AUX |
                   FS2_EPI_OUT_BF16 | FS2_EPI_AUX_BF16;
  if (knob == -1 || voc || hx64 || !s.vec || (s.flags & ~keep) || s.c_out % 8) return 1;
  int kz = knob > 0 ? knob : (grid < 512 && ncb >= 8 ? (int)((768 + grid - 1) / grid) : 1);
  if (kz > ncb / 4) kz = ncb / 4;
  return kz < 2 ? 1 : kz;
}

// the tap-major kernel on bm x bn tiles
inline void plan_nt(ConvPlan& p, const ConvShape& s, const int* tune, int bm, int bn, int stages,
                    bool voc) {
  p.kernel = CONV_NT;
  p.bm = bm;
  p.bn = bn;
  p.tiles_m = (int)((s.rows + bm - 1) / bm);
  p.tiles_n = (int)((s.c_out + bn - 1) / bn);
  // n-tiles per group: all of them by default (measured: smaller weight-slice groups did not
  // pay on the step's shapes and multiplied the A re-reads of the long-K data gradient)
  const int g = tune[FS2_TUNE_NT_GROUP] > 0 ? tune[FS2_TUNE_NT_GROUP] : p.tiles_n;
  p.group = g > p.tiles_n ? p.tiles_n : g;
  p.grid = (unsigned)(p.tiles_m * p.tiles_n);
  p.voc = voc;
  // vocoder convs: one pipeline depth, dilation + the extended epilogue
  p.stages = voc ? 2 : stages;
  // K1: taps == 1 and K % 64 == 0 (the Linear / 1x1 projections) stage through buffer descriptors
  p.k1 = !voc && p.tapaligned && s.taps == 1 && tune[FS2_TUNE_NT_K1] >= 0;
}

// one of the halo kernel's builds: hx64 (dilated vocoder convs) and voc take the vocoder
// epilogue without the pipelined loop, the rest the pipelined 4-wave build
inline void plan_halo_tile(ConvPlan& p, int bm, int bn, bool hx64, bool voc) {
  p.kernel = CONV_HALO;
  p.bm = bm;
  p.bn = bn;
  p.stages = 2;
  p.hx = hx64 ? 64 : 16;
  p.voc = hx64 || voc;
  p.pipe = !(hx64 || voc);
}

inline void plan_halo_split(ConvPlan& p, const ConvShape& s, int bm, int bn, bool pipe, int kz) {
  plan_halo_tile(p, bm, bn, false, false);
  p.pipe = pipe;
  p.kz = kz;
  p.grid *= (unsigned)kz;
  p.reduce_bm = bm == 64 ? 64 : 128;
  const int64_t n8 = s.rows * (s.c_out / 8);
  p.reduce_grid = (unsigned)((n8 + 255) / 256 < 2048 ? (n8 + 255) / 256 : 2048);
}

inline ConvPlan plan_base(const ConvShape& s) {
  ConvPlan p{};
  p.block = 256;
  p.waves = 4;
  p.kz = 1;
  p.group = 1;
  p.taps = s.taps;
  p.tapaligned = s.c_in % 64 == 0;
  return p;
}

inline ConvPlan plan_conv_gemm(const ConvShape& s, const int* tune, int cu_count) {
  ConvPlan p = plan_base(s);
  const int64_t rows = s.rows, seq_len = s.seq_len, c_in = s.c_in, c_out = s.c_out;
  const int taps = s.taps, dil = s.dilation, flags = s.flags;
  const int K = (int)(taps * c_in);
  const bool tapaligned = p.tapaligned;
  const bool voc = dil != 1 || (flags & (FS2_EPI_LRELU | FS2_EPI_ACC_Y | FS2_EPI_Y2)) || !s.has_y;
  const int64_t big = ((rows + 127) / 128) * ((c_out + 127) / 128);
  // narrow vocoder convs (HiFi-GAN's 64- and 32-channel stages, millions of rows): the
  // n-tile matches c_out instead of wasting 1/2-3/4 of a 128-wide tile's MFMAs
  if (voc && c_out <= 64 && big >= 128) {
    if (c_out <= 32) {
      plan_nt(p, s, tune, 128, 32, 2, true);
    } else if (taps > 1 && (taps - 1) * dil <= 64 && tapaligned && seq_len % 128 == 0 &&
               tune[FS2_TUNE_NT_HALO] >= 0) {
      plan_halo_tile(p, 128, 64, (taps - 1) * dil > 16, true);
      p.tiles_m = (int)((rows + 127) / 128);
      p.tiles_n = 1;
      p.group = 1;
      p.grid = (unsigned)p.tiles_m;
    } else {
      plan_nt(p, s, tune, 128, 64, 2, true);
    }
    return p;
  }
  // tap-register halo kernel (conv_gemm_tapreg): 4-wave 128 x 64 tiles at 3 blocks per CU when
  // they fill at least one round of the CUs (decoder k=9 forward, encoder k=9 forward, PostNet
  // 512 -> 512; smaller grids keep the halo kernels' split-K / 64-row paths).  Alone, decoder
  // k=9 forward: 89.7 us vs 94.4 (128 x 128, 2 blocks per CU) and 97.7 (8-wave 256 x 128, one
  // block per CU): independent blocks overlap one another's barrier / DMA phases.  Narrow
  // outputs (c_out <= 256: the decoder k=9 data gradient, which runs beside the side stream's
  // k=9 weight gradient) take the 128 x 128 tiles at 2 blocks per CU: slower alone (109 vs
  // 87 us) but the dgrad||wgrad pair is 181 vs 191 us and the step 7.40 vs 7.55 ms
  const int trk = tune[FS2_TUNE_TAPREG];
  if (trk >= 0 && !voc && tapaligned && (taps == 5 || taps == 9) && s.pad >= 0 && s.pad < taps) {
    const int64_t t4 = (rows / 128) * ((c_out + 63) / 64);
    const bool ok4 = seq_len % 128 == 0 && rows % 128 == 0 && rows % seq_len == 0;
    int pick = 0;
    if (trk == 1) pick = ok4 ? 4 : 0;                  // force 128 x 64
    else if (trk == 3) pick = ok4 ? 3 : 0;             // force 128 x 128
    else if (ok4 && c_out <= 256 && t4 >= 3 * cu_count) pick = 3;
    else if (ok4 && t4 >= 3 * cu_count) pick = 4;
    if (pick) {
      const bool n64 = pick == 4;
      p.kernel = CONV_TAPREG;
      p.bm = 128;
      p.bn = n64 ? 64 : 128;  // 128 x 128: 2 blocks per CU, 128 x 64: 3
      p.stages = 2;
      p.tiles_m = (int)(rows / 128);
      p.tiles_n = (int)((c_out + (n64 ? 63 : 127)) / (n64 ? 64 : 128));
      // tile group: the n-tiles whose weight slice (~1.25 MB) an XCD's resident blocks share in
      // its 4 MB L2 while they walk the m-tiles (all 16 n-tiles of the decoder k=9 forward, a
      // 4.7 MB weight, re-fetched it past L2: 187 MB per launch; groups of 4: 92 -> 85 us)
      if (tune[FS2_TUNE_NT_GROUP] > 0) {
        p.group = halo_group(p.tiles_n, tune);
      } else {
        const int64_t slice = (int64_t)(n64 ? 64 : 128) * K * 2;
        const int gr = (int)(((int64_t)5 << 18) / slice);
        p.group = gr < 1 ? 1 : gr > p.tiles_n ? p.tiles_n : gr;
      }
      p.grid = (unsigned)(p.tiles_m * p.tiles_n);
      return p;
    }
  }
  // halo kernel (tile sizes as the tap-major choice below: 128x128 / 128x64 / 64x64 by grid;
  // FS2_TUNE_NT_HALO = 2 forces 128 x 128).  Every row tile must lie inside one utterance.
  const bool halo_wide = big >= 512 || tune[FS2_TUNE_NT_HALO] == 2;
  int halo_bm = halo_wide || big >= 128 ? 128 : 64;
  // utterances a multiple of 64 rows only (the vocoder's 64-rows-per-frame stage over an odd
  // frame count): 64-row tiles keep the halo kernel (the tap-major one re-stages A per tap)
  if (halo_bm == 128 && seq_len % 128 != 0 && seq_len % 64 == 0) halo_bm = 64;
  // 8-wave 256 x 128 halo tiles, one block per CU with the weight prefetch in flight across the
  // barrier, for the wide forward shapes (c_in <= 256, >= 512 128x128 tiles, T % 256 == 0) that
  // the tap-register kernel does not take (k=9 decoder forward 114 -> 102 us alone,
  // scripts/halo_check.py; FS2_TUNE_NT_HALO 1 disables it).  C_in 512 (the PostNet convs) ran
  // faster on the 4-wave 128 x 128 tiles (78 -> 73 / 84 -> 77 us: the 8-wave grid of 384 blocks
  // is 1.5 rounds of the CUs there).  Deeper rings and 128 x 128 8-wave tiles measured slower.
  if (tune[FS2_TUNE_NT_HALO] == 0 && big >= 512 && c_in <= 256 && taps > 1 &&
      (taps - 1) * dil <= 16 && tapaligned && !voc && seq_len % 256 == 0) {
    plan_halo_tile(p, 256, 128, false, false);
    p.waves = 8;
    p.block = 512;
    p.tiles_m = (int)((rows + 255) / 256);
    p.tiles_n = (int)((c_out + 127) / 128);
    p.group = halo_group(p.tiles_n, tune);
    p.grid = (unsigned)(p.tiles_m * p.tiles_n);
    return p;
  }
  if (taps > 1 && (taps - 1) * dil <= 64 && tapaligned && seq_len % halo_bm == 0 &&
      tune[FS2_TUNE_NT_HALO] >= 0) {
    p.tiles_m = (int)((rows + halo_bm - 1) / halo_bm);
    p.tiles_n = (int)((c_out + (halo_wide ? 127 : 63)) / (halo_wide ? 128 : 64));
    p.group = halo_group(p.tiles_n, tune);
    p.grid = (unsigned)(p.tiles_m * p.tiles_n);
    // HX: halo rows beyond the tile, 16 (taps <= 17 undilated: the FFT/PostNet/VP convs) or
    // 64 (dilated vocoder convs; the larger A image leaves 2 blocks per CU)
    const bool hx64 = (taps - 1) * dil > 16;
    // a forced split count (FS2_TUNE_HALO_SPLITK > 0) also applies to full 128-row grids
    const int forced = tune[FS2_TUNE_HALO_SPLITK] > 0 ? halo_splitk_count(s, tune, p.grid, voc, hx64) : 1;
    if (halo_wide && halo_bm == 128) {
      if (forced > 1) plan_halo_split(p, s, 128, 128, false, forced);  // (experiments)
      else plan_halo_tile(p, 128, 128, hx64, voc);
    } else if (halo_wide) {
      plan_halo_tile(p, 64, 128, hx64, voc);
    } else if (halo_bm == 128) {
      if (forced > 1) plan_halo_split(p, s, 128, 64, true, forced);
      else plan_halo_tile(p, 128, 64, hx64, voc);
    } else {
      // under-filled 64x64 grid: with 128-row utterance multiples, 128x64 tiles split kz ways
      // (half the weight-tile re-staging per output row of 64x64 tiles); else 64x64 split
      const int tiles_m2 = (int)((rows + 127) / 128);
      const unsigned grid2 = (unsigned)(tiles_m2 * p.tiles_n);
      const int kz2 = seq_len % 128 == 0 && tune[FS2_TUNE_HALO_SPLITK] != -2
                          ? halo_splitk_count(s, tune, grid2, voc, hx64) : 1;
      const int kz = kz2 > 1 ? 1 : halo_splitk_count(s, tune, p.grid, voc, hx64);
      if (kz2 > 1) {
        p.tiles_m = tiles_m2;
        p.grid = grid2;
        plan_halo_split(p, s, 128, 64, true, kz2);
      } else if (kz > 1) {
        plan_halo_split(p, s, 64, 64, true, kz);
      } else {
        plan_halo_tile(p, 64, 64, hx64, voc);
      }
    }
    return p;
  }
  // tap-major kernel.  LDS stages (scripts/nt_sweep.py): 128x128 tiles run 3-4 blocks per CU
  // and overlap one another's load phase with one stage; the smaller-grid tilings prefetch
  // (2 stages, 4 for 64x64 tiles with K >= 4096, where each block walks 144 k-tiles)
  const int st = tune[FS2_TUNE_GEMM_STAGES];
  auto stages = [&](int dflt) { return st == 2 || st == 3 || st == 4 ? st : st ? 1 : dflt; };
  if ((big >= 512 && tune[FS2_TUNE_NT_TILE] == 0) || tune[FS2_TUNE_NT_TILE] == 1)
    plan_nt(p, s, tune, 128, 128, stages(1), voc);
  else if ((big >= 128 && tune[FS2_TUNE_NT_TILE] == 0) || tune[FS2_TUNE_NT_TILE] == 2)
    plan_nt(p, s, tune, 128, 64, stages(2), voc);
  else
    plan_nt(p, s, tune, 64, 64, stages(K >= 4096 ? 4 : 2), voc);
  return p;
}

// fs2_conv_gemm_ln / fs2_conv_gemm_ln_bwd: the tap-major kernel on 64 x 256 tiles (whole
// 256-wide rows; the forward takes 128 x 256 with FS2_TUNE_LN_TILE = 1)
inline ConvPlan plan_conv_gemm_ln(const ConvShape& s, const int* tune, bool bwd) {
  ConvPlan p = plan_base(s);
  const bool wide = !bwd && tune[FS2_TUNE_LN_TILE] == 1;
  p.kernel = CONV_NT;
  p.bm = wide ? 128 : 64;
  p.bn = 256;
  p.stages = 2;
  p.k1 = !wide && p.tapaligned && s.taps == 1 && tune[FS2_TUNE_NT_K1] >= 0;
  p.tiles_m = (int)((s.rows + p.bm - 1) / p.bm);
  p.tiles_n = 1;
  p.grid = (unsigned)p.tiles_m;
  return p;
}

// ------------------------------------------------------------------ weight gradient
enum WgradKernel { WGRAD_K1_MULTI = 0, WGRAD_WIDE = 1, WGRAD_BAND = 2, WGRAD_HALO = 3, WGRAD_TN = 4 };
enum WgradReduce { WRED_NONE = 0, WRED_K1_MULTI = 1, WRED_K1 = 2, WRED_ROWS = 3, WRED_TAPS = 4 };

// limits of the kernels' LDS lists (static_asserted against the kernels' constants)
constexpr int kWgradRowsMax = 9 * 1024;  // wgrad_reduce_rows: floats of one output row in LDS
constexpr int kWideMaxBands = 2048;      // conv_wgrad_wide: 64-row bands listed in LDS with lens
constexpr int kBandMaxBands = 1024;      // conv_wgrad_band: likewise
constexpr int kColsumRows = 256;         // rows per column-sum partial (gemm.hip)

struct WgradShape {
  int64_t rows, seq_len, c_in, c_out;
  int taps, pad;
  bool has_lens, has_db;
  bool dw16;  // dw 16-B aligned
  bool ws16;  // ws != NULL and 16-B aligned
};

struct WgradPlan {
  int kernel;              // WgradKernel
  int tile, stages, taps;  // template parameters chosen at run time
  int splits, tiles_o, tiles_k;
  unsigned grid, block;
  int reduce;              // WgradReduce
  unsigned reduce_grid;    // workgroups (wgrad_reduce_taps: x * y)
  unsigned reduce_grid_x;
};

// Weight-gradient decomposition (measured on the step's shapes, scripts/wgrad_sweep.py):
// 128-wide tiles with <= 8 row splits for the large k>1 products, 64-wide tiles with 4..24
// splits (>= 8 k-tiles of 64 rows each) for the small ones, ~1024 blocks where possible.
inline int wgrad_tile(int64_t c_in, int64_t c_out, int taps, const int* tune) {
  if (tune[FS2_TUNE_WGRAD_TILE]) return tune[FS2_TUNE_WGRAD_TILE] == 64 ? 64 : 128;
  return (int64_t)taps * c_in * c_out >= (1 << 20) ? 128 : 64;
}

inline int wgrad_splits(int64_t rows, int64_t c_in, int64_t c_out, int taps, const int* tune) {
  if (tune[FS2_TUNE_WGRAD_SPLITS]) {
    const int s = tune[FS2_TUNE_WGRAD_SPLITS];
    return s < 1 ? 1 : s > 64 ? 64 : s;
  }
  const int64_t Kp = (int64_t)taps * c_in;
  const int bt = wgrad_tile(c_in, c_out, taps, tune);
  const int64_t tiles = ((c_out + bt - 1) / bt) * ((Kp + bt - 1) / bt);
  // k = 1 (tap-major kernel, 4 blocks per CU): at most one round of 1024 blocks -- rounding
  // the split count up put 32 of the decoder QKV product's 1056 blocks in a second round
  // (45.9 -> 33.6 us alone with 21 splits instead of 22)
  int64_t s = taps == 1 ? 1024 / tiles : (1024 + tiles - 1) / tiles;
  const int64_t hi = bt == 128 ? 8 : 24;
  if (s > hi) s = hi;
  if (s < 4) s = 4;
  if (s > rows / 512) s = rows / 512;
  if (s < 1) s = 1;
  return (int)s;
}

// grouped k = 1 weight gradient: splits chosen so that the grid is about 256 blocks of
// 128 x 128 tiles
inline int k1_multi_splits(int64_t tiles_total, int64_t rows) {
  int64_t s = (256 + tiles_total / 2) / tiles_total;
  if (s > rows / 512) s = rows / 512;  // >= 8 k-tiles per split (small products: fewer slabs)
  return (int)(s < 1 ? 1 : s);
}

// jobs: host int64 rows {dy, ldy, x, ldx, dw, db, c_in, c_out}
inline WgradPlan plan_wgrad_k1_multi(const int64_t* jobs, int n, int64_t rows, const int* tune) {
  WgradPlan p{};
  int64_t tiles = 0, ub = 0, bb = 0;
  for (int j = 0; j < n; ++j) {
    const int64_t cin = jobs[8 * j + 6], cout = jobs[8 * j + 7];
    tiles += ((cout + 127) / 128) * ((cin + 127) / 128);
    ub += cout * cin / 4;
    bb += jobs[8 * j + 5] ? cout : 0;
  }
  p.kernel = WGRAD_K1_MULTI;
  p.tile = 128;
  p.taps = 1;
  p.splits = k1_multi_splits(tiles > 0 ? tiles : 1, rows);
  // LDS ring depth (FS2_TUNE_WGRAD_K1M_STAGES, A/B): 0 = 4 slots (128 KB, three k-tiles in flight)
  const int stg = tune[FS2_TUNE_WGRAD_K1M_STAGES];
  p.stages = stg == 2 || stg == 3 ? stg : 4;
  p.grid = (unsigned)(tiles * p.splits);
  p.block = 512;
  p.reduce = WRED_K1_MULTI;
  p.reduce_grid = p.reduce_grid_x = (unsigned)((ub + bb + 255) / 256);
  return p;
}

inline int64_t wgrad_k1_multi_ws_floats(const int64_t* jobs, int n, int64_t rows, const int* tune) {
  const int S = plan_wgrad_k1_multi(jobs, n, rows, tune).splits;
  int64_t f = 0;
  for (int j = 0; j < n; ++j) {
    const int64_t cin = jobs[8 * j + 6], cout = jobs[8 * j + 7];
    f += S * cout * cin + (jobs[8 * j + 5] ? S * cout : 0);
    f = (f + 3) / 4 * 4;
  }
  return f;
}

// wide-tile kernel's split count: about 256 blocks, >= 4 bands per split (FS2_TUNE_WGRAD_WIDE
// > 1 forces it); 0 = not eligible
inline int wgrad_wide_splits(int64_t rows, int64_t c_in, int64_t c_out, int taps, const int* tune) {
  const int v = tune[FS2_TUNE_WGRAD_WIDE];
  if (v < 0) return 0;
  if (!(taps == 3 || taps == 5 || taps == 9)) return 0;
  // default: the channel counts that are not 64-multiples (the PostNet's 80-channel convs:
  // 97.5 -> 36 us alone against the band kernel).  On the 64-multiple shapes it was neutral to
  // slower alone and 0.54 ms/step slower in the step (its 163-VGPR waves, two per SIMD, leave
  // no room for the concurrent data gradient's 244-VGPR waves; profiles/r5_wide_ab.txt)
  if (v == 0 && c_in % 64 == 0 && c_out % 64 == 0) return 0;
  if (rows % 64 || rows / 64 > (1 << 15) || rows < 256) return 0;
  if (c_in % 8 || c_out % 8 || (c_in * taps) % 4) return 0;
  const int64_t tiles = ((c_out + 63) / 64) * ((c_in + 63) / 64);
  const int64_t nb = rows / 64;
  int64_t z = v > 1 ? v : (256 + tiles / 2) / tiles;
  if (z > nb / 4) z = nb / 4;
  if (z > 64) z = 64;
  return (int)(z < 1 ? 1 : z);
}

// slab workspace (floats) the wide kernel needs at this shape (0 when it needs none)
inline int64_t wgrad_wide_ws_floats(int64_t rows, int64_t c_in, int64_t c_out, int taps, const int* tune) {
  const int z = wgrad_wide_splits(rows, c_in, c_out, taps, tune);
  if (z <= 1) return 0;
  return (int64_t)z * c_out * (c_in * taps + 1);
}

// workspace of fs2_conv_wgrad: split slabs [S][c_out][taps c_in], then the bias partials;
// or the wide kernel's slabs, or the grouped k = 1 kernel's with one job
inline int64_t wgrad_ws_bytes(int64_t rows, int64_t c_in, int64_t c_out, int taps, const int* tune) {
  const int64_t S = wgrad_splits(rows, c_in, c_out, taps, tune);
  const int64_t parts = ((rows + kColsumRows - 1) / kColsumRows) * c_out;
  const int64_t bias_part = S * c_out > parts ? S * c_out : parts;
  int64_t b = (S * c_out * taps * c_in + bias_part) * 4;
  const int64_t wide = wgrad_wide_ws_floats(rows, c_in, c_out, taps, tune) * 4;
  b = wide > b ? wide : b;
  if (taps == 1) {
    const int64_t job[8] = {0, c_out, 0, c_in, 0, 1, c_in, c_out};
    const int64_t m = wgrad_k1_multi_ws_floats(job, 1, rows, tune) * 4;
    b = m > b ? m : b;
  }
  return b;
}

// bf16 fs2_conv_wgrad.  The caller has checked that the channel counts and strides are
// multiples of 8 and that dy / x are 16-B aligned.
inline WgradPlan plan_conv_wgrad(const WgradShape& s, const int* tune) {
  const int64_t rows = s.rows, seq_len = s.seq_len, c_in = s.c_in, c_out = s.c_out;
  const int taps = s.taps;
  if (taps == 1 && tune[FS2_TUNE_WGRAD_K1] == 0) {
    // k = 1: the grouped split-K kernel with one job (128 x 128 tiles, one reduce)
    const int64_t job[8] = {0, 0, 0, 0, 0, s.has_db ? 1 : 0, c_in, c_out};
    return plan_wgrad_k1_multi(job, 1, rows, tune);
  }
  WgradPlan p{};
  p.taps = taps;
  p.block = 256;
  const bool pad_ok = s.pad >= 0 && s.pad <= taps - 1;
  if (taps > 1 && tune[FS2_TUNE_WGRAD_HALO] == 0) {
    // 64 x 64 x taps tiles shared by eight waves (conv_wgrad_wide)
    const int Z = wgrad_wide_splits(rows, c_in, c_out, taps, tune);
    if (Z >= 1 && seq_len > 0 && seq_len % 64 == 0 && rows % seq_len == 0 &&
        !(s.has_lens && rows / 64 > kWideMaxBands) && pad_ok && s.dw16 && !(Z > 1 && !s.ws16)) {
      p.kernel = WGRAD_WIDE;
      p.tile = 64;
      p.stages = 3;
      p.splits = Z;
      p.tiles_o = (int)((c_out + 63) / 64);
      p.tiles_k = (int)((c_in + 63) / 64);
      p.block = 512;
      p.grid = (unsigned)(p.tiles_o * p.tiles_k * Z + (s.has_db ? Z * p.tiles_o : 0));
      if (Z > 1) {
        p.reduce = WRED_K1_MULTI;
        p.reduce_grid = p.reduce_grid_x =
            (unsigned)((c_out * c_in * taps / 4 + (s.has_db ? c_out : 0) + 255) / 256);
      }
      return p;
    }
    // no split slabs where the output tiles fill the chip (conv_wgrad_band): 32 x 32 x taps
    // output tiles over all rows, bands of 64 rows inside one utterance
    const int BR = 64;
    const bool halo_ok = c_in % 64 == 0 && c_out % 64 == 0 && seq_len % 64 == 0;
    const int to = (int)((c_out + 31) / 32), tc = (int)((c_in + 31) / 32);
    // grids under half the CUs keep the split-K kernels (the variance predictors' 256 x 256 k=3
    // convs at T = 128: 64 tiles), unless those would be the tap-major kernel (C % 64 != 0: the
    // PostNet's 80-channel convs, 48 tiles -- 26 vs 47 us alone, on 48 CUs)
    const int min_tiles = tune[FS2_TUNE_WGRAD_BAND] == 3 ? 128 : halo_ok ? 128 : 32;
    const bool band =
        (taps == 3 || taps == 5 || taps == 9) && pad_ok && seq_len % BR == 0 &&
        rows % seq_len == 0 && rows / BR <= (1 << 15) &&
        !(s.has_lens && rows / BR > kBandMaxBands) &&  // the kernel's LDS band list
        c_in >= 32 && c_out >= 32 &&
        // taps 3 / 5 with 64-multiple channels (PostNet 512, variance predictors) stay on the
        // split-K halo kernel: step 6.91 vs 6.98 ms with the band kernel there
        // (profiles/r4_ab_experiments.txt)
        !(tune[FS2_TUNE_WGRAD_BAND] != 4 && taps != 9 && halo_ok) &&
        to * tc >= min_tiles &&
        // f32x4 read-modify-writes of dw: rows of c_in * taps floats, tile columns 32 * taps
        s.dw16 && (c_in * taps) % 4 == 0;
    if (band) {
      // (4-slot rings and 8-wave blocks measured slower in the step and were removed in round
      // 5: profiles/r4_ab_experiments.txt)
      p.kernel = WGRAD_BAND;
      p.tile = 32;
      p.stages = 2;
      p.tiles_o = to;
      p.tiles_k = tc;
      p.grid = (unsigned)(to * tc);
      return p;
    }
  }
  // split-K: the halo kernel (64 x 64 x taps tiles) or the tap-major one, then a reduce
  p.splits = wgrad_splits(rows, c_in, c_out, taps, tune);
  const int64_t Kp = (int64_t)taps * c_in;
  const bool halo = (taps == 3 || taps == 5 || taps == 9) && c_in % 64 == 0 && c_out % 64 == 0 &&
                    seq_len % 64 == 0 && tune[FS2_TUNE_WGRAD_HALO] >= 0;
  if (halo) {
    p.kernel = WGRAD_HALO;
    p.tile = 64;
    p.stages = 2;
    p.tiles_o = (int)(c_out / 64);
    p.tiles_k = (int)(c_in / 64);
  } else {
    p.kernel = WGRAD_TN;
    p.tile = wgrad_tile(c_in, c_out, taps, tune);
    const int st = tune[FS2_TUNE_WGRAD_STAGES];
    p.stages = st >= 1 && st <= 4 ? st : (p.tile == 128 ? 1 : 2);
    p.tiles_o = (int)((c_out + p.tile - 1) / p.tile);
    p.tiles_k = (int)((Kp + p.tile - 1) / p.tile);
  }
  p.grid = (unsigned)(p.tiles_o * p.tiles_k * p.splits);
  if (taps == 1) {
    const int64_t total = c_out * c_in;  // multiple of 64 (both channel counts % 8 == 0)
    p.reduce = WRED_K1;
    p.reduce_grid = p.reduce_grid_x = (unsigned)((total / 4 + 63) / 64);
  } else if (Kp <= kWgradRowsMax && c_in % 4 == 0) {
    p.reduce = WRED_ROWS;
    p.reduce_grid = p.reduce_grid_x = (unsigned)c_out;
  } else {
    p.reduce = WRED_TAPS;
    p.reduce_grid_x = (unsigned)((c_in + 63) / 64);
    p.reduce_grid = p.reduce_grid_x * (unsigned)c_out;
  }
  return p;
}

// ------------------------------------------------------------------ names
// The kernel a plan launches, in the profiler's demangled form without the `void fs2::` prefix
// and the argument list.
inline const char* tf(bool b) { return b ? "true" : "false"; }

inline void conv_plan_kernel_name(const ConvPlan& p, char* out, int cap) {
  if (p.kernel == CONV_TAPREG)
    snprintf(out, cap, "conv_gemm_tapreg<128, %d, 2, 2, 4, %d, 2, %d>", p.bn, p.taps, p.bn == 128 ? 2 : 3);
  else if (p.kernel == CONV_HALO)
    snprintf(out, cap, "conv_gemm_halo<%d, %d, 2, %d, %s, %d, %s>", p.bm, p.bn, p.hx, tf(p.voc), p.waves, tf(p.pipe));
  else
    snprintf(out, cap, "conv_gemm_nt_glds<%d, %d, %d, %s, %s, %s>", p.bm, p.bn, p.stages, tf(p.tapaligned), tf(p.voc), tf(p.k1));
}

inline void wgrad_plan_kernel_name(const WgradPlan& p, char* out, int cap) {
  switch (p.kernel) {
    case WGRAD_K1_MULTI: snprintf(out, cap, "wgrad_k1_multi<%d>", p.stages); break;
    case WGRAD_WIDE: snprintf(out, cap, "conv_wgrad_wide<%d, 3>", p.taps); break;
    case WGRAD_BAND: snprintf(out, cap, "conv_wgrad_band<%d, 2, 2, 4>", p.taps); break;
    case WGRAD_HALO: snprintf(out, cap, "conv_wgrad_halo<%d>", p.taps); break;
    default: snprintf(out, cap, "conv_wgrad_tn_glds<%d, %d>", p.tile, p.stages);
  }
}

inline const char* wgrad_reduce_name(int reduce) {
  static const char* const name[] = {"-", "wgrad_k1_multi_reduce", "wgrad_reduce_k1",
                                     "wgrad_reduce_rows", "wgrad_reduce_taps"};
  return reduce >= WRED_NONE && reduce <= WRED_TAPS ? name[reduce] : "-";
}

// "<kernel> grid=G group=g kz=k reduce=<kernel or -> reduce_grid=R"
inline void conv_plan_describe(const ConvPlan& p, char* out, int cap) {
  char name[96], red[48] = "-";
  conv_plan_kernel_name(p, name, sizeof name);
  if (p.kz > 1) snprintf(red, sizeof red, "halo_splitk_reduce<%d>", p.reduce_bm);
  snprintf(out, cap, "%s grid=%u group=%d kz=%d reduce=%s reduce_grid=%u", name, p.grid, p.group,
           p.kz, red, p.kz > 1 ? p.reduce_grid : 0u);
}

inline void wgrad_plan_describe(const WgradPlan& p, char* out, int cap) {
  char name[96];
  wgrad_plan_kernel_name(p, name, sizeof name);
  snprintf(out, cap, "%s grid=%u group=%d kz=%d reduce=%s reduce_grid=%u", name, p.grid, 0,
           p.splits, wgrad_reduce_name(p.reduce), p.reduce_grid);
}

}  // namespace fs2
