// bf16 implicit-GEMM Conv1d / Linear, forward and dX ("NT"), staged by LDS-DMA.
//
//   y[r, o] = epilogue( sum_{j,c} wk[o, j*Cin + c] * x[r + j - pad, c] )
//
// Tile BM x BN x 64, 4 waves (2 x 2), v_mfma_f32_16x16x32_bf16.  Both operand tiles are
// filled with global_load_lds_dwordx4: one wave-instruction writes 1 KiB = 8 rows x 128 B of
// a lane-linear [rows][64] bf16 image.  The image is XOR-swizzled on the SOURCE address
// (16-B chunk c of row R lands at chunk c ^ ((R >> 1) & 7)), so the ds_read_b128 fragment
// reads of 16 consecutive rows hit 16 distinct 16-B bank slots.  The conv tap shift lives in
// the per-lane source address: rows outside their utterance (and rows/channels past the
// matrix edge) read a 16-B zero line instead, so padding costs no branches in the loop.
// Row-dependent address parts (utterance start, frame index) are computed once per block;
// per k-tile only the tap index and channel offset change (scalar when Cin % 64 == 0).
//
// STAGES = 1: load; vmcnt(0); barrier; MFMA; barrier (occupancy 3-4 blocks/CU hides the
//             load phase of one block under the MFMA phase of the others).
// STAGES = 2: the next tile's DMA is issued before the current tile's MFMAs and stays in
//             flight across the barrier (counted vmcnt, raw s_barrier).
//
// Blocks are renumbered XCD-aware (bijective remap): each XCD runs a contiguous range of
// (m, n) tiles, n fastest, so an A row band is fetched from HBM once per XCD L2.
//
// Epilogue: accumulators go through LDS (fp32, 132-float rows, conflict-free writes) and
// leave as 8-element row vectors: bias, residual/aux add, ReLU, ReLU-mask and the bf16 cast
// are applied on 16-B (bf16) / 32-B (fp32) coalesced stores.
// The halo kernels share this unit with the tap-major ones: conv_gemm_halo<128, 64, ..> and
// <64, 64, ..> use the same nt_epilogue instantiations as the tap-major kernels of those
// tiles, and hipcc emits different (equivalent) epilogue address arithmetic for them when the
// two families are compiled apart.
#include <mutex>

#include "conv_nt.hpp"
#include "conv_plan.hpp"

namespace fs2 {

template <int BM, int BN, int STAGES, bool TAPALIGNED, bool VOC, bool K1 = false>
__global__ __launch_bounds__(256, (K1 && BM == 128 && BN == 128 && STAGES == 1) ? 3 : 1) void
conv_gemm_nt_glds(GldsArgs a) {
  static_assert(!K1 || (TAPALIGNED && !VOC), "K1: taps == 1, K % 64 == 0, no vocoder epilogue");
  const int dil = VOC ? a.dil : 1;
  constexpr int BK = 64;
  constexpr int AW = BM / 32, BW = BN / 32;  // glds per wave per tile (8 rows each)
  constexpr int MI = BM / 32, NI = BN / 32;  // 16x16 fragments per wave (2x2 waves)
  constexpr int STAGE_E = (BM + BN) * BK;    // elements per stage
  constexpr int EPI_LD = BN + 4;             // fp32 epilogue row stride
  constexpr int EPI_E = (BM / 2) * EPI_LD * 2;
  constexpr int SMEM_E = STAGES * STAGE_E > EPI_E ? STAGES * STAGE_E : EPI_E;
  __shared__ __attribute__((aligned(1024))) u16 smem[SMEM_E];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, r16 = lane & 15;

  // XCD-aware bijective renumbering of the 1-D grid
  const int nwg = a.tiles_m * a.tiles_n;
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  // tile order: groups of `group` n-tiles (a weight slice that stays L2-resident), m-tiles
  // within a group, n fastest -- each XCD's contiguous share streams its A rows once per group
  const int gfull = a.tiles_m * a.group;
  const int ng = wg / gfull, rem = wg - ng * gfull;
  const int gsz = a.tiles_n - ng * a.group < a.group ? a.tiles_n - ng * a.group : a.group;
  const int tm = m_interleave(rem / gsz, a.tiles_m, a.lens != nullptr);
  const int tn = ng * a.group + (rem - (rem / gsz) * gsz);
  const int64_t m0 = (int64_t)tm * BM;
  const int n0 = tn * BN;
  const bool skip = a.lens && rows_all_padding(a.lens, a.T, m0, m0 + BM < a.M ? m0 + BM : a.M);

  // ---- per-lane source descriptors (fixed over the k loop)
  const int lrow = lane >> 3;  // row within the 8-row piece
  const u16* zero = reinterpret_cast<const u16*>(g_zero_line);
  int64_t a_base[AW];  // element offset of the row's utterance start (or -1: row invalid)
  int a_t[AW];         // frame index within the utterance
  int a_lc[AW];        // logical 16-B chunk this lane fetches
#pragma unroll
  for (int i = 0; i < AW; ++i) {
    const int R = (wave * AW + i) * 8 + lrow;
    const int64_t m = m0 + R;
    a_lc[i] = (lane & 7) ^ ((R >> 1) & 7);
    if (m < a.M) {
      const int64_t s = m / a.T;
      a_t[i] = (int)(m - s * a.T);
      a_base[i] = s * a.T;
    } else {
      a_t[i] = 0;
      a_base[i] = -1;
    }
  }
  const u16* b_src[BW];
  int b_lc[BW];
#pragma unroll
  for (int i = 0; i < BW; ++i) {
    const int R = (wave * BW + i) * 8 + lrow;
    const int n = n0 + R;
    b_lc[i] = (lane & 7) ^ ((R >> 1) & 7);
    b_src[i] = n < a.N ? a.w + (int64_t)n * a.K + b_lc[i] * 8 : nullptr;
  }

  const int nk = (a.K + BK - 1) / BK;
  // K1 staging: descriptors over the tile's BM rows of x / BN rows of w
  const auto x_rs = buf_rsrc(a.x + m0 * a.ldx, (a.M - m0 < BM ? a.M - m0 : BM) * a.ldx * 2);
  const auto w_rs = buf_rsrc(a.w + (int64_t)n0 * a.K, (int64_t)(a.N - n0 < BN ? a.N - n0 : BN) * a.K * 2);
  uint32_t a_vo[K1 ? AW : 1], b_vo[K1 ? BW : 1];
  if constexpr (K1) {
#pragma unroll
    for (int i = 0; i < AW; ++i)
      a_vo[i] = (uint32_t)((((wave * AW + i) * 8 + lrow) * a.ldx + a_lc[i] * 8) * 2);
#pragma unroll
    for (int i = 0; i < BW; ++i)
      b_vo[i] = (uint32_t)((((wave * BW + i) * 8 + lrow) * a.K + b_lc[i] * 8) * 2);
  }
  auto issue_k1 = [&](int kt, int stage) {
    u16* As = smem + stage * STAGE_E;
    u16* Bs = As + BM * BK;
    const uint32_t k0 = (uint32_t)(kt * BK * 2);
#pragma unroll
    for (int i = 0; i < AW; ++i) glds16_buf(x_rs, As + (wave * AW + i) * 8 * BK, a_vo[i], k0);
#pragma unroll
    for (int i = 0; i < BW; ++i) glds16_buf(w_rs, Bs + (wave * BW + i) * 8 * BK, b_vo[i], k0);
  };
  auto issue = [&](int kt, int stage) {
    u16* As = smem + stage * STAGE_E;
    u16* Bs = As + BM * BK;
    const int k0 = kt * BK;
    int j0 = 0, c0 = 0;
    if constexpr (TAPALIGNED) {
      j0 = k0 / a.Cin;
      c0 = k0 - j0 * a.Cin;
    }
#pragma unroll
    for (int i = 0; i < AW; ++i) {
      const u16* src = zero;
      int j = j0, c = c0 + a_lc[i] * 8;
      bool kok = true;
      if constexpr (!TAPALIGNED) {
        const int k = k0 + a_lc[i] * 8;
        kok = k < a.K;
        j = k / a.Cin;
        c = k - j * a.Cin;
      }
      const int tt = a_t[i] + j * dil - a.pad;
      if (kok && a_base[i] >= 0 && tt >= 0 && tt < a.T)
        src = a.x + (a_base[i] + tt) * a.ldx + c;
      glds16(src, As + (wave * AW + i) * 8 * BK);
    }
#pragma unroll
    for (int i = 0; i < BW; ++i) {
      const u16* src = zero;
      bool kok = true;
      if constexpr (!TAPALIGNED) kok = k0 + b_lc[i] * 8 < a.K;
      if (b_src[i] && kok) src = b_src[i] + k0;
      glds16(src, Bs + (wave * BW + i) * 8 * BK);
    }
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment element offsets (swizzle depends only on r16 because row bases are 16-aligned)
  const int sw = (r16 >> 1) & 7;
  const int fo0 = r16 * BK + ((0 * 4 + g) ^ sw) * 8;
  const int fo1 = r16 * BK + ((1 * 4 + g) ^ sw) * 8;
  auto compute = [&](int stage) {
    const u16* As = smem + stage * STAGE_E + wm * (BM / 2) * BK;
    const u16* Bs = smem + stage * STAGE_E + BM * BK + wn * (BN / 2) * BK;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int fo = ks ? fo1 : fo0;
      bf16x8 fa[MI], fb[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(As + i * 16 * BK + fo);
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(Bs + j * 16 * BK + fo);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  };

  if (!skip) {
    if constexpr (K1) kloop<STAGES, AW + BW>(nk, issue_k1, compute);
    else kloop<STAGES, AW + BW>(nk, issue, compute);
  }

  nt_epilogue<BM, BN, VOC, 4, 2, 2, 0, K1>(a, acc, smem, m0, n0, skip, tid, wm, wn, g, r16);
}

// ------------------------------------------------------------------------ halo variant
// Conv1d with taps > 1, Cin % 64 == 0 and T % BM == 0 (every row tile lies inside one
// utterance).  The reduction runs channel-block-major: for each 64-channel block the
// BM + taps - 1 input rows of the tile and its tap halo (zero outside the utterance) are
// staged in LDS ONCE, and tap j reads them at row offset j -- only the weight tile is
// re-staged per tap, through a 2-slot ring.  Against the tap-major kernel above this removes
// (taps-1)/taps of the A-operand LDS-DMA traffic: the k=9 FFN conv moves 18 KB instead of
// 32 KB per 64-deep step of a 128 x 128 tile.  LDS rows are swizzled chunk c -> c ^ (row & 7),
// which keeps the 16-row fragment reads conflict-free at every row offset.
template <int BM, int BN, int BST, int HX, bool VOC, int NWAVE = 4, bool PIPE = false>
__global__ __launch_bounds__(NWAVE * 64, NWAVE == 8 ? 1 : HX > 16 ? 2 : 3)
void conv_gemm_halo(GldsArgs a) {
  static_assert(BST == 2, "the 2-slot weight ring (1- and 3-slot rings measured slower, profiles/r2_ab_experiments.txt)");
  // NWAVE = 4: 2 x 2 waves; NWAVE = 8: 2 (rows) x 4 (columns) waves, one block per CU
  const int dil = VOC ? a.dil : 1;
  constexpr int BK = 64;
  constexpr int WN = NWAVE / 2;
  constexpr int MI = BM / 32, NI = BN / WN / 16;
  constexpr int HMAX = BM + HX;                     // halo rows allocated ((taps-1)*dil <= HX)
  constexpr int QMAX = (HMAX / 8 + NWAVE - 1) / NWAVE;  // 8-row halo pieces per wave
  constexpr int BW = BN / 8 / NWAVE;                // weight pieces per wave
  constexpr int A_E = HMAX * BK, B_E = BN * BK;
  // BST == 2: two halo slots -- channel block cb + 1's rows are staged while cb's taps run
  constexpr int NA = BST == 2 ? 2 : 1;
  constexpr int EPI_E = (BM / 2) * (BN + 4) * 2;
  constexpr int SMEM_E = NA * A_E + BST * B_E > EPI_E ? NA * A_E + BST * B_E : EPI_E;
  __shared__ __attribute__((aligned(1024))) u16 smem[SMEM_E];
  u16* As = smem;
  u16* Bs = smem + NA * A_E;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, r16 = lane & 15;

  // kz > 1 (split-K over channel blocks): split z owns channel blocks [cb0, cb1) of every
  // tile; the splits are the outer index of the XCD-contiguous order
  const int kz = a.kz > 1 ? a.kz : 1;
  const int nwg = a.tiles_m * a.tiles_n, nall = nwg * kz;
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nall >> 3, r8 = nall & 7;
  const int wga = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int z = wga / nwg, wg = wga - z * nwg;
  const int gfull = a.tiles_m * a.group;
  const int ng = wg / gfull, rem = wg - ng * gfull;
  const int gsz = a.tiles_n - ng * a.group < a.group ? a.tiles_n - ng * a.group : a.group;
  const int tm = m_interleave(rem / gsz, a.tiles_m, a.lens != nullptr);
  const int tn = ng * a.group + (rem - (rem / gsz) * gsz);
  const int64_t m0 = (int64_t)tm * BM;
  const int n0 = tn * BN;
  const bool skip = a.lens && rows_all_padding(a.lens, a.T, m0, m0 + BM < a.M ? m0 + BM : a.M);
  // this wave's half of the tile (BM/2 rows) all padding: it stages its share of the tiles but
  // issues no MFMAs (those outputs are masked downstream; the 256-row forward tiles of the
  // decoder's k=9 conv hold ~13 % such rows)
  const int64_t hr0 = m0 + wm * (BM / 2), hr1 = hr0 + BM / 2 < a.M ? hr0 + BM / 2 : a.M;
  const bool half_pad = !VOC && (hr0 >= a.M || (a.lens && rows_all_padding(a.lens, a.T, hr0, hr1)));
  const int ncb_all = a.Cin / 64, cb0 = z * ncb_all / kz, cb1 = (z + 1) * ncb_all / kz;

  const int lrow = lane >> 3;
  const int HR = BM + (a.taps - 1) * dil, HP = (HR + 7) / 8;
  const int64_t u0 = (m0 / a.T) * a.T;
  // input rows past the utterance's length are zero in the FFT blocks (Layers.py:25,28) and in
  // the upstream gradients: read them from the zero line (no HBM traffic).  Vocoder lens are
  // row limits of another meaning: the whole padded utterance is staged there.
  const int64_t ulen = (!VOC && a.lens) ? (a.lens[m0 / a.T] < a.T ? a.lens[m0 / a.T] : a.T) : a.T;
  const int64_t u1 = u0 + ulen < a.M ? u0 + ulen : a.M;
  // this wave's 16-row fragments holding a row below the utterance's length (input rows past
  // it are staged as zeros; outputs past it are masked downstream of the FFT / variance-
  // predictor convs -- the only lens users of this kernel)
  int mi_act = MI;
  if (!VOC && a.lens) {
    const int64_t nv = u1 - (m0 + wm * (BM / 2));
    mi_act = nv <= 0 ? 0 : nv >= BM / 2 ? MI : (int)((nv + 15) / 16);
  }
  // halo piece p = wave + NWAVE q: rows h = 8 p + lrow, global row m0 - pad + h.  Buffer
  // descriptors based at the tile's first halo row / first weight row; a lane whose row lies
  // outside the utterance (or past N) carries an out-of-range offset and stages zeros.  The
  // channel block and tap advance in the scalar offset.
  const auto x_rs = buf_rsrc(a.x + (m0 - a.pad) * a.ldx + cb0 * BK, (int64_t)HMAX * a.ldx * 2);
  const auto w_rs = buf_rsrc(a.w + (int64_t)n0 * a.K + cb0 * BK, (int64_t)BN * a.K * 2);
  uint32_t h_vo[QMAX];
#pragma unroll
  for (int q = 0; q < QMAX; ++q) {
    const int h = (wave + NWAVE * q) * 8 + lrow;
    const int64_t gr = m0 - a.pad + h;
    const int lc = (lane & 7) ^ (h & 7);
    h_vo[q] = (gr >= u0 && gr < u1) ? (uint32_t)((h * a.ldx + lc * 8) * 2) : kOOB;
  }
  uint32_t b_vo[BW];
#pragma unroll
  for (int i = 0; i < BW; ++i) {
    const int R = (wave * BW + i) * 8 + lrow;
    b_vo[i] = n0 + R < a.N ? (uint32_t)((R * a.K + ((lane & 7) ^ (R & 7)) * 8) * 2) : kOOB;
  }

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int a_row = wm * (BM / 2) + r16;
  const int b_row = wn * (BN / WN) + r16;
  const int b_off[2] = {b_row * BK + ((0 + g) ^ (b_row & 7)) * 8, b_row * BK + ((4 + g) ^ (b_row & 7)) * 8};
  // step s = cb * taps + j: weight tile (tap j, channel block cb) into ring slot s % BST; the
  // halo of channel block cb is staged at j == 0
  auto issue_a = [&](int cb, int aslot) {
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
      const int pc = wave + NWAVE * q;
      if (pc < HP) glds16_buf(x_rs, As + aslot * A_E + pc * 8 * BK, h_vo[q], (uint32_t)(cb * BK * 2));
    }
  };
  int qa = 0;  // this wave's halo pieces (its LDS-DMA count per halo stage)
#pragma unroll
  for (int q = 0; q < QMAX; ++q) qa += (wave + NWAVE * q) < HP ? 1 : 0;
  auto issue_b = [&](int cb, int j, int slot) {
    const uint32_t k0 = (uint32_t)((j * a.Cin + cb * BK) * 2);
#pragma unroll
    for (int i = 0; i < BW; ++i) glds16_buf(w_rs, Bs + slot * B_E + (wave * BW + i) * 8 * BK, b_vo[i], k0);
  };
  // PIPE: one k-half (ks) of step (j, slot, aslot) into a register set, and its MFMAs
  // (nact: compile-time count of this wave's 16-row fragments that hold a valid row; the
  // others are neither read nor multiplied -- see mi_act below)
  auto frag_ld = [&](auto nact, int j, int slot, int aslot, int ks, bf16x8 (&fa)[MI],
                     bf16x8 (&fb)[NI]) {
    constexpr int NACT = decltype(nact)::value;
    const int ha = a_row + j * dil, sa = ha & 7;
    const u16* pa = As + aslot * A_E + ha * BK + ((ks * 4 + g) ^ sa) * 8;
    const u16* pb = Bs + slot * B_E + b_off[ks];
#pragma unroll
    for (int i = 0; i < NACT; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(pa + i * 16 * BK);
#pragma unroll
    for (int jj = 0; jj < NI; ++jj) fb[jj] = *reinterpret_cast<const bf16x8*>(pb + jj * 16 * BK);
  };
  auto mfma_half = [&](auto nact, const bf16x8 (&fa)[MI], const bf16x8 (&fb)[NI]) {
    constexpr int NACT = decltype(nact)::value;
#pragma unroll
    for (int i = 0; i < NACT; ++i)
#pragma unroll
      for (int jj = 0; jj < NI; ++jj)
        acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[jj], acc[i][jj], 0, 0, 0);
  };
  auto compute = [&](int j, int slot, int aslot) {
    if (half_pad) return;
    // fragment rows differ by multiples of 16, so one swizzle serves all of them.  All 16
    // fragment reads of the step are issued before the first MFMA: the waits before the
    // MFMAs are then counted (the second k-half's reads land under the first half's MFMAs)
    const int ha = a_row + j * dil, sa = ha & 7;
    bf16x8 fa[2][MI], fb[2][NI];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const u16* pa = As + aslot * A_E + ha * BK + ((ks * 4 + g) ^ sa) * 8;
      const u16* pb = Bs + slot * B_E + b_off[ks];
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[ks][i] = *reinterpret_cast<const bf16x8*>(pa + i * 16 * BK);
#pragma unroll
      for (int jj = 0; jj < NI; ++jj) fb[ks][jj] = *reinterpret_cast<const bf16x8*>(pb + jj * 16 * BK);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int jj = 0; jj < NI; ++jj)
          acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ks][i], fb[ks][jj], acc[i][jj], 0, 0, 0);
  };
  if (!skip) {
    const int ncb = cb1 - cb0;
    if constexpr (PIPE) {
      // Fragment-pipelined 2-slot loop.  Step s = (cb, j) reads weight slot s & 1 and halo slot
      // cb & 1 as two k-halves held in two register sets: set 1 (s, ks 1) is read while set 0's
      // MFMAs issue; then ONE barrier, after which set 0 is refilled with step s + 1's first
      // half under set 1's MFMAs -- a wave never waits on LDS right after the barrier.
      // At the barrier of step s every wave has retired all its reads of step s (lgkmcnt(0)),
      // so weight slot s & 1 takes tile s + 2 and, after cb's last tap, halo slot cb & 1 takes
      // channel block cb + 2.  Tile s + 1 (and its halo, issued earlier) must have landed:
      // it was issued at the previous barrier, followed at most by one halo (`pend` pieces of
      // this wave), and loads retire in issue order.  A wave whose rows are all padding runs
      // the same loads and barriers without fragments or MFMAs (a separate loop body, so the
      // compute body has no per-step branches for the wait-count analysis to merge).
      const int S = ncb * a.taps;
      issue_a(0, 0);
      issue_b(0, 0, 0);
      issue_b(0, 1, 1);  // taps >= 2: step 1 = (0, 1)
      int pend0 = 0;
      if (ncb > 1) {
        issue_a(1, 1);
        pend0 = qa;
      }
      vm_wait_n(BW + pend0);  // halo 0 and weight tile 0 landed
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      auto pipe_loop = [&](auto nact) {
        constexpr bool C = decltype(nact)::value > 0;
        bf16x8 fa0[MI], fb0[NI], fa1[MI], fb1[NI];
        if constexpr (C) frag_ld(nact, 0, 0, 0, 0, fa0, fb0);
        int cb = 0, j = 0, pend = pend0;
        // steps 0 .. S-2 (the last step, with no successor, is peeled below: a loop body whose
        // barrier half were conditional would merge two wait states before set 1's MFMAs)
        for (int s = 0; s + 1 < S; ++s) {
          const bool last_tap = j + 1 == a.taps;
          const int jn = last_tap ? 0 : j + 1, cbn = last_tap ? cb + 1 : cb;
          // set 0 landed under the previous step's second half (free wait).  The builtin form
          // (not inline asm) lets the compiler's wait-count pass see it: with 2 x 10 reads in
          // flight (beyond the 15-deep LDS counter) it would otherwise wait for set 1 as well
          // before set 0's MFMAs.
          __builtin_amdgcn_s_waitcnt(kLgkm0);
          if constexpr (C) {
            frag_ld(nact, j, s & 1, cb & 1, 1, fa1, fb1);
            mfma_half(nact, fa0, fb0);
          }
          __builtin_amdgcn_sched_barrier(0);
          vm_wait_n(pend);
          __builtin_amdgcn_s_waitcnt(kLgkm0);
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
          pend = 0;
          if (s + 2 < S) {
            const bool l2 = jn + 1 == a.taps;
            issue_b(l2 ? cbn + 1 : cbn, l2 ? 0 : jn + 1, s & 1);
          }
          if (last_tap && cb + 2 < ncb) {
            issue_a(cb + 2, cb & 1);
            pend = qa;
          }
          if constexpr (C) {
            frag_ld(nact, jn, (s + 1) & 1, cbn & 1, 0, fa0, fb0);
            mfma_half(nact, fa1, fb1);
          }
          __builtin_amdgcn_sched_barrier(0);
          cb = cbn;
          j = jn;
        }
        if constexpr (C) {
          __builtin_amdgcn_s_waitcnt(kLgkm0);
          frag_ld(nact, j, (S - 1) & 1, cb & 1, 1, fa1, fb1);
          mfma_half(nact, fa0, fb0);
          mfma_half(nact, fa1, fb1);
        }
      };
      // with lens, a wave whose rows past the first half of its fragments are all padding
      // runs the half-width body (their outputs are masked downstream, as for half_pad)
      if (half_pad) pipe_loop(std::integral_constant<int, 0>{});
      else if (mi_act <= MI / 2) pipe_loop(std::integral_constant<int, MI / 2>{});
      else pipe_loop(std::integral_constant<int, MI>{});
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else {
      // weight-tile ring of BST slots, BST-1 tiles ahead: step s = (cb, j) reads slot s % BST
      // while tiles s+1 .. s+BST-1 are in flight.  At a channel-block boundary the single
      // halo buffer is reloaded after a barrier (everyone finished the previous block).
      const int S = ncb * a.taps;
      issue_a(0, 0);
      for (int d = 0; d < BST - 1 && d < S; ++d) issue_b(d / a.taps, d % a.taps, d);
      int cb = 0, j = 0, slot = 0;
      for (int s = 0; s < S; ++s) {
        if (j == 0 && s > 0) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          issue_a(cb, 0);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int sn = s + BST - 1;
        if (sn < S) {
          const int cbn = sn / a.taps;
          issue_b(cbn, sn - cbn * a.taps, sn % BST);
        }
        compute(j, slot, 0);
        slot = slot + 1 == BST ? 0 : slot + 1;
        if (++j == a.taps) {
          j = 0;
          ++cb;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
  if (kz > 1) {  // raw fp32 partial product into slab z (halo_splitk_reduce applies the epilogue)
    GldsArgs e = a;
    e.flags = 0;
    e.y = a.slab + (int64_t)z * a.M * a.N;
    e.ldy = a.N;
    e.vec = 1;
    nt_epilogue<BM, BN, VOC, NWAVE, WN>(e, acc, smem, m0, n0, skip, tid, wm, wn, g, r16);
    return;
  }
  nt_epilogue<BM, BN, VOC, NWAVE, WN>(a, acc, smem, m0, n0, skip, tid, wm, wn, g, r16);
}

// Split-K epilogue of the halo kernel: y = epilogue(sum_z slab[z]) in split order, 8 columns
// per thread, with nt_epilogue's non-vocoder semantics (bias, aux add, ReLU / ReLU mask, bf16
// cast; tiles of BM rows that are all padding get no bias, as in the unsplit kernel).
template <int BM>
__global__ __launch_bounds__(256) void halo_splitk_reduce(GldsArgs a) {
  const int64_t n8 = a.N / 8, total = a.M * n8;
  const bool out_bf16 = a.flags & FS2_EPI_OUT_BF16, aux_bf16 = a.flags & FS2_EPI_AUX_BF16;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / n8;
    const int n = (int)(e - m * n8) * 8;
    const float* sp = a.slab + m * a.N + n;
    f32x4 lo = ld4(sp), hi = ld4(sp + 4);
    for (int z = 1; z < a.kz; ++z) {
      const float* q = sp + (int64_t)z * a.M * a.N;
      lo += ld4(q);
      hi += ld4(q + 4);
    }
    float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const int64_t t0 = m / BM * BM;
    const bool skip = a.lens && rows_all_padding(a.lens, a.T, t0, t0 + BM < a.M ? t0 + BM : a.M);
    if ((a.flags & FS2_EPI_BIAS) && !skip) {
      const f32x4 b0 = ld4(a.bias + n), b1 = ld4(a.bias + n + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] += b0[i];
        v[i + 4] += b1[i];
      }
    }
    float av[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (a.flags & (FS2_EPI_ADD_AUX | FS2_EPI_RELU_MASK_AUX)) {
      if (aux_bf16) {
        const uint4 raw = *reinterpret_cast<const uint4*>((const u16*)a.aux + m * a.ld_aux + n);
        const uint32_t wv[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          av[2 * i] = __uint_as_float(wv[i] << 16);
          av[2 * i + 1] = __uint_as_float(wv[i] & 0xffff0000u);
        }
      } else {
        const float* ap = (const float*)a.aux + m * a.ld_aux + n;
        const f32x4 a0 = ld4(ap), a1 = ld4(ap + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          av[i] = a0[i];
          av[i + 4] = a1[i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (a.flags & FS2_EPI_ADD_AUX) v[i] += av[i];
      if (a.flags & FS2_EPI_RELU) v[i] = fmaxf(v[i], 0.f);
      if (a.flags & FS2_EPI_RELU_MASK_AUX) v[i] = av[i] > 0.f ? v[i] : 0.f;
    }
    if (out_bf16) {
      uint4 o;
      o.x = (uint32_t)to_bf16(v[0]) | ((uint32_t)to_bf16(v[1]) << 16);
      o.y = (uint32_t)to_bf16(v[2]) | ((uint32_t)to_bf16(v[3]) << 16);
      o.z = (uint32_t)to_bf16(v[4]) | ((uint32_t)to_bf16(v[5]) << 16);
      o.w = (uint32_t)to_bf16(v[6]) | ((uint32_t)to_bf16(v[7]) << 16);
      *reinterpret_cast<uint4*>((u16*)a.y + m * a.ldy + n) = o;
    } else {
      float* yp = (float*)a.y + m * a.ldy + n;
      st4(yp, f32x4{v[0], v[1], v[2], v[3]});
      st4(yp + 4, f32x4{v[4], v[5], v[6], v[7]});
    }
  }
}

// ------------------------------------------------------------------------ launchers
// One launcher per kernel family: each maps a plan (conv_plan.hpp) to its template instance and
// launches it.  A plan no instance is built for is an error of the call, never another kernel.
// Every *_try compares all of its template parameters with the plan, so at most one of a chain
// matches and the order of a chain does not matter.
template <int BM, int BN, int S, bool TA, bool VOC, bool K1 = false>
static bool nt_try(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  if (p.bm != BM || p.bn != BN || p.stages != S || p.tapaligned != TA || p.voc != VOC || p.k1 != K1)
    return false;
  conv_gemm_nt_glds<BM, BN, S, TA, VOC, K1><<<p.grid, 256, 0, st>>>(a);
  return true;
}

// the builds of one tile and pipeline depth: the vocoder's (two stages), K1, tap-aligned, general
template <int BM, int BN, int S>
static bool nt_try_tile(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  if (p.stages != (p.voc ? 2 : S)) return false;
  return nt_try<BM, BN, 2, true, true>(p, a, st) || nt_try<BM, BN, 2, false, true>(p, a, st) ||
         nt_try<BM, BN, S, true, false, true>(p, a, st) || nt_try<BM, BN, S, true, false>(p, a, st) ||
         nt_try<BM, BN, S, false, false>(p, a, st);
}

template <int BM, int BN>
static bool nt_try_stages(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  if (p.bm != BM || p.bn != BN) return false;
  return nt_try_tile<BM, BN, 1>(p, a, st) || nt_try_tile<BM, BN, 2>(p, a, st) ||
         nt_try_tile<BM, BN, 3>(p, a, st) || nt_try_tile<BM, BN, 4>(p, a, st);
}

int launch_conv_nt(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  const bool ok =
      p.bn == 256  // the LayerNorm epilogues' whole-row tiles
          ? nt_try<64, 256, 2, true, false, true>(p, a, st) || nt_try<64, 256, 2, true, false>(p, a, st) ||
                nt_try<64, 256, 2, false, false>(p, a, st) || nt_try<128, 256, 2, true, false>(p, a, st) ||
                nt_try<128, 256, 2, false, false>(p, a, st)
          : nt_try_stages<128, 128>(p, a, st) || nt_try_stages<128, 64>(p, a, st) ||
                nt_try_stages<64, 64>(p, a, st) || nt_try_tile<128, 32, 2>(p, a, st);
  return ok ? FS2_OK : no_instance("conv_gemm_nt_glds");
}

// Split-K workspace of the halo kernel.  A grid below ~3 blocks per CU with a
// long channel loop (the encoder's k=9 data gradient: 384 tiles, 16 channel blocks x 9 taps
// each) leaves CUs with one block and the rest with two; splitting the channel blocks kz ways
// fills the chip and halves each block's serial loop, at the cost of kz fp32 partial products
// summed by halo_splitk_reduce.
//
// The decomposition is a function of the shape alone (halo_splitk_count, conv_plan.hpp): no
// stream, capture or allocation state can change it, so every call of a shape sums in one fp32 order.  The
// partials live in process-wide buffers (halo_splitk_slab), one for eager calls and one for
// calls recorded into a graph (a replay must not share scratch with eager work on another
// stream); both grow together, outside capture only.  Any failure to provide them -- a capture
// needing more than an earlier eager call sized, an event or allocation error -- is an error
// of the call, never a silent switch to the unsplit launch.  (Rounds 4 / 5 fell back to the
// unsplit kernel, a different summation order, on such failures: a process-history-dependent
// result.)  Stream order between eager users: each eager split launch pair records one event
// after its reduce (halo_splitk_done) and the next eager user's stream always waits on it.
// A graph buffer is never freed while a graph may still replay it (retired on growth).
static std::mutex g_splitk_mu;
static hipEvent_t g_splitk_ev = nullptr;
static bool g_splitk_recorded = false;
static float* g_slab[2] = {nullptr, nullptr};  // [0] eager calls, [1] captured calls
static size_t g_slab_cap = 0;
static bool g_slab_captured = false;  // g_slab[1] is referenced by a captured graph
static void halo_splitk_done(hipStream_t st) {
  std::lock_guard<std::mutex> lock(g_splitk_mu);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;
  if (g_splitk_ev && hipEventRecord(g_splitk_ev, st) == hipSuccess) g_splitk_recorded = true;
}
static int halo_splitk_slab(GldsArgs& a, int kz, hipStream_t st) {
  const size_t need = (size_t)kz * (size_t)a.M * (size_t)a.N * sizeof(float);
  std::lock_guard<std::mutex> lock(g_splitk_mu);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    set_error("fs2_conv_gemm: split-K: stream capture query failed");
    return FS2_ERR_LAUNCH;
  }
  const bool capturing = cs != hipStreamCaptureStatusNone;
  if (capturing) {
    if (g_slab_cap < need) {
      set_error("fs2_conv_gemm: split-K partials of %zu bytes needed during graph capture; run the "
                "same shapes eagerly once before capturing (%zu bytes sized)", need, g_slab_cap);
      return FS2_ERR_LAUNCH;
    }
    g_slab_captured = true;
    a.slab = g_slab[1];
  } else {
    if (!g_splitk_ev && hipEventCreateWithFlags(&g_splitk_ev, hipEventDisableTiming) != hipSuccess) {
      g_splitk_ev = nullptr;
      set_error("fs2_conv_gemm: split-K: event creation failed");
      return FS2_ERR_LAUNCH;
    }
    // the previous eager user's reduce has read the buffer before this stream writes it
    if (g_splitk_recorded && hipStreamWaitEvent(st, g_splitk_ev, 0) != hipSuccess) {
      set_error("fs2_conv_gemm: split-K: stream wait failed");
      return FS2_ERR_LAUNCH;
    }
    if (g_slab_cap < need) {
      if (hipDeviceSynchronize() != hipSuccess) {
        set_error("fs2_conv_gemm: split-K: device synchronisation failed");
        return FS2_ERR_LAUNCH;
      }
      (void)hipFree(g_slab[0]);
      if (!g_slab_captured) (void)hipFree(g_slab[1]);  // else retired: a graph may replay it
      g_slab[0] = g_slab[1] = nullptr;
      g_slab_cap = 0;
      g_slab_captured = false;
      void *p0 = nullptr, *p1 = nullptr;
      if (hipMalloc(&p0, need) != hipSuccess || hipMalloc(&p1, need) != hipSuccess) {
        (void)hipFree(p0);
        set_error("fs2_conv_gemm: split-K: hipMalloc of %zu bytes failed", need);
        return FS2_ERR_LAUNCH;
      }
      g_slab[0] = static_cast<float*>(p0);
      g_slab[1] = static_cast<float*>(p1);
      g_slab_cap = need;
    }
    a.slab = g_slab[0];
  }
  poison(a.slab, (int64_t)need, st);
  return FS2_OK;
}

template <int BM, int BN, int HX, bool VOC, int NWAVE = 4, bool PIPE = false>
static bool halo_try(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  if (p.bm != BM || p.bn != BN || p.hx != HX || p.voc != VOC || p.waves != NWAVE || p.pipe != PIPE)
    return false;
  conv_gemm_halo<BM, BN, 2, HX, VOC, NWAVE, PIPE><<<p.grid, NWAVE * 64, 0, st>>>(a);
  return true;
}

// the builds of one 4-wave tile: dilated vocoder (HX 64), vocoder epilogue, pipelined
template <int BM, int BN>
static bool halo_try_tile(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  if (p.bm != BM || p.bn != BN) return false;
  return halo_try<BM, BN, 64, true>(p, a, st) || halo_try<BM, BN, 16, true>(p, a, st) ||
         halo_try<BM, BN, 16, false, 4, true>(p, a, st);
}

// kz > 1: partial products into the process-wide slab, then halo_splitk_reduce
int launch_conv_halo(const ConvPlan& p, GldsArgs& a, hipStream_t st) {
  if (p.kz > 1) {
    if (int rc = halo_splitk_slab(a, p.kz, st)) return rc;
    a.kz = p.kz;
  }
  const bool ok = halo_try<128, 64, 64, true>(p, a, st) || halo_try<128, 64, 16, true>(p, a, st) ||
                  halo_try<256, 128, 16, false, 8, true>(p, a, st) ||
                  halo_try<128, 128, 16, false>(p, a, st) ||  // forced split of 128 x 128 tiles
                  halo_try_tile<128, 128>(p, a, st) || halo_try_tile<64, 128>(p, a, st) ||
                  halo_try<128, 64, 16, false, 4, true>(p, a, st) || halo_try_tile<128, 64>(p, a, st) ||
                  halo_try<64, 64, 16, false, 4, true>(p, a, st) || halo_try_tile<64, 64>(p, a, st);
  if (!ok) return no_instance("conv_gemm_halo");
  if (p.kz > 1) {
    if (p.reduce_bm == 64) halo_splitk_reduce<64><<<p.reduce_grid, 256, 0, st>>>(a);
    else halo_splitk_reduce<128><<<p.reduce_grid, 256, 0, st>>>(a);
    halo_splitk_done(st);
  }
  return FS2_OK;
}

}  // namespace fs2
