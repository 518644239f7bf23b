#include "glds.hpp"
#include "conv_plan.hpp"

namespace fs2 {

// ------------------------------------------------------------------------ weight gradient
//   slab[z][o][kk] = sum_{m in split z} dy[m, o] * x~[m, kk],  x~[m, j*Cin + c] = x[m + j - pad, c]
//   bslab[z][o]    = sum_{m in split z} dy[m, o]            (bias gradient, optional)
//
// Both operands are k-major ([reduction rows][channels]).  Tiles 128 (o) x 128 (kk) x 64
// rows; each operand's LDS image is [64 rows][128] bf16 (256-B rows), filled lane-linearly by
// glds (4 rows per wave-instruction) with the 16-B chunk swizzle c ^ ((R & 7) << 1) on the
// source, and read with ds_read_b64_tr_b16: a fragment's 8 k come from rows {4g+q} and
// {16+4g+q} of the 32-row k-step, so each 32-lane half reads 8 distinct rows x 2 chunks =
// 16 distinct bank slots.  The frame index of each staged row is carried incrementally
// across k-tiles (no division in the loop).  The bias gradient rides on the same A
// fragments: the waves of the first kk column tile multiply them by a ones fragment.
struct WgradGlds {
  const u16* dy;
  int64_t ldy;
  const u16* x;
  int64_t ldx;
  float* slab;
  float* bslab;
  int64_t M, T;
  int Cin, Cout, taps, pad, Kp;
  int64_t rows_per_split;
  int tiles_o, tiles_k, splits;
  const int64_t* lens;  // optional: 64-row k-tiles made only of padding rows are skipped
};

template <int BT, int STAGES>
__global__ __launch_bounds__(256) void conv_wgrad_tn_glds(WgradGlds a) {
  constexpr int BM = BT, BN = BT, BK = 64;  // BT = 128 or 64 (o and kk tile widths)
  constexpr int MI = BM / 32, NI = BN / 32;
  constexpr int NCH = BT / 8;               // 16-B chunks per image row
  constexpr int RPI = 64 / NCH;             // image rows per glds wave-instruction
  constexpr int IPW = BK / RPI / 4;         // glds per wave per operand per tile
  constexpr int IMG = BK * BT;              // elements per operand image
  constexpr int STAGE_E = 2 * IMG;
  constexpr int EPI_LD = BN + 4;
  constexpr int EPI_E = (BM / 2) * EPI_LD * 2;
  constexpr int SMEM_E = STAGES * STAGE_E > EPI_E ? STAGES * STAGE_E : EPI_E;
  constexpr int MAXKT = 1024;  // k-tile list (skipping all-padding tiles) lives after the ring
  __shared__ __attribute__((aligned(1024))) u16 smem[SMEM_E + MAXKT + 64];
  short* ktl = reinterpret_cast<short*>(smem + SMEM_E);
  int* wcnt = reinterpret_cast<int*>(smem + SMEM_E + MAXKT);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3, r16 = lane & 15;

  const int per_split = a.tiles_o * a.tiles_k;
  const int nwg = per_split * a.splits;
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int z = wg / per_split, rem = wg - z * per_split;
  const int tk = rem % a.tiles_k, to = rem / a.tiles_k;
  const int o0 = to * BM, n0 = tk * BN;
  const int64_t r_begin = (int64_t)z * a.rows_per_split;
  int64_t r_end = r_begin + a.rows_per_split;
  if (r_end > a.M) r_end = a.M;
  const int nk_all = r_end > r_begin ? (int)((r_end - r_begin + BK - 1) / BK) : 0;
  // ordered list of the split's k-tiles that hold at least one real row (wave ballots +
  // prefix popcounts; skipped tiles add exact zeros, so the sums are unchanged bitwise)
  const bool use_list = a.lens != nullptr && nk_all <= MAXKT;
  int nk = nk_all;
  if (use_list) {
    int total = 0;
    for (int c0 = 0; c0 < nk_all; c0 += 256) {
      const int kt = c0 + tid;
      bool v = false;
      if (kt < nk_all) {
        const int64_t q0 = r_begin + (int64_t)kt * BK;
        v = !rows_all_padding(a.lens, a.T, q0, q0 + BK < r_end ? q0 + BK : r_end);
      }
      const uint64_t mask = __ballot(v);
      if (lane == 0) wcnt[wave] = __popcll(mask);
      __syncthreads();
      int before = total;
      for (int w = 0; w < wave; ++w) before += wcnt[w];
      const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
      if (v) ktl[before + below] = (short)kt;
      for (int w = 0; w < 4; ++w) total += wcnt[w];
      __syncthreads();
    }
    nk = total;
  }

  // per-lane staging descriptors: instruction i stages rows RPI*(wave*IPW+i) + lane/NCH.
  // Chunk swizzle f(R): 256-B rows (BT 128) (R & 7) << 1; 128-B rows (BT 64)
  // ((R >> 1) & 3) << 1 -- either way a 32-lane transposed read (8 rows x 2 chunks) hits
  // 16 distinct 16-B bank slots.
  auto swz_of = [](int R) { return BT == 128 ? (R & 7) << 1 : ((R >> 1) & 3) << 1; };
  const u16* zero = reinterpret_cast<const u16*>(g_zero_line);
  const int pc = lane % NCH;
  int R[IPW], t_i[IPW], a_col[IPW], b_j[IPW], b_c[IPW];
  int64_t base_i[IPW];
  bool a_ok[IPW], b_ok[IPW];
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    R[i] = (wave * IPW + i) * RPI + lane / NCH;
    const int lc = pc ^ swz_of(R[i]);
    a_col[i] = o0 + lc * 8;
    a_ok[i] = a_col[i] < a.Cout;
    const int kk = n0 + lc * 8;
    b_ok[i] = kk < a.Kp;
    b_j[i] = kk / a.Cin;
    b_c[i] = kk - b_j[i] * a.Cin;
    const int64_t m = r_begin + R[i];
    const int64_t s = m / a.T;
    t_i[i] = (int)(m - s * a.T);
    base_i[i] = s * a.T;
  }

  int cur_tile = 0;  // the k-tile whose rows t_i / base_i describe
  auto issue = [&](int kt, int stage) {
    u16* As = smem + stage * STAGE_E;
    u16* Bs = As + IMG;
    const int tile = use_list ? (int)ktl[kt] : kt;
    const int adv = (tile - cur_tile) * BK;
    cur_tile = tile;
    const int64_t k0 = r_begin + (int64_t)tile * BK;
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      t_i[i] += adv;
      while (t_i[i] >= a.T) {
        t_i[i] -= (int)a.T;
        base_i[i] += a.T;
      }
      const int64_t m = k0 + R[i];
      const bool mok = m < r_end;
      const u16* sa = (mok && a_ok[i]) ? a.dy + m * a.ldy + a_col[i] : zero;
      glds16(sa, As + (wave * IPW + i) * RPI * BT);
      const int tt = t_i[i] + b_j[i] - a.pad;
      const u16* sb = (mok && b_ok[i] && tt >= 0 && tt < a.T)
                          ? a.x + (base_i[i] + tt) * a.ldx + b_c[i] : zero;
      glds16(sb, Bs + (wave * IPW + i) * RPI * BT);
    }
  };

  f32x4 acc[MI][NI], accb[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bool do_bias = a.bslab != nullptr && tk == 0 && wn == 0;  // wave-uniform
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

  // transposed fragment: 16 columns at col0, k-step ks; rows {4g+q} and {16+4g+q}
  const int swz = swz_of(4 * g + q);
  // transposed fragment halves (asm reads, see ds_tr16): rows ks*32 + {4g+q} and + 16
  auto tr_lo = [&](const u16* img, int col0, int ks, int hi) -> s16x4 {
    const int lc = (col0 >> 3) + (p >> 1);
    const int off = (ks * 32 + 4 * g + q + 16 * hi) * BT + ((lc ^ swz) << 3) + ((p & 1) << 2);
    return ds_tr16(img + off);
  };
  // both k-halves' fragment reads issued up front; the first half's MFMAs start once its reads
  // (the older 2 (MI + NI)) landed
  auto compute = [&](int stage) {
    const u16* As = smem + stage * STAGE_E;
    const u16* Bs = As + IMG;
    s16x4 ra[2][MI][2], rb[2][NI][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) ra[ks][i][h] = tr_lo(As, wm * (BM / 2) + i * 16, ks, h);
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) rb[ks][j][h] = tr_lo(Bs, wn * (BN / 2) + j * 16, ks, h);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks == 0) lgkm_wait<(2 * (MI + NI) < 15 ? 2 * (MI + NI) : 15)>();  // 4-bit counter
      else lgkm_wait<0>();
      bf16x8 fa[MI], fb[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = tr16_cat(ra[ks][i][0], ra[ks][i][1]);
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[j] = tr16_cat(rb[ks][j][0], rb[ks][j][1]);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
          accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], ones, accb[i], 0, 0, 0);
      }
    }
  };

  kloop<STAGES, 2 * IPW>(nk, issue, compute);

  if (do_bias && r16 == 0) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + wm * (BM / 2) + i * 16 + 4 * g + r;
        if (o < a.Cout) a.bslab[(int64_t)z * a.Cout + o] = accb[i][r];
      }
  }
  // slab tile through LDS: rows o, 8 consecutive kk per thread (32-B stores)
  float* Cs = reinterpret_cast<float*>(smem);
  float* slab = a.slab + (int64_t)z * a.Cout * a.Kp;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (wm == h) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(i * 16 + 4 * g + r) * EPI_LD + wn * (BN / 2) + j * 16 + r16] = acc[i][j][r];
    }
    __syncthreads();
    constexpr int TPR = BN / 8, RPP = 256 / TPR;
    const int cc = (tid % TPR) * 8;
    const int kk = n0 + cc;
#pragma unroll
    for (int pp = 0; pp < (BM / 2) / RPP; ++pp) {
      const int rr = pp * RPP + tid / TPR;
      const int o = o0 + h * (BM / 2) + rr;
      if (o < a.Cout && kk < a.Kp) {
        float* dst = slab + (int64_t)o * a.Kp + kk;
        *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(Cs + rr * EPI_LD + cc);
        *reinterpret_cast<f32x4*>(dst + 4) = *reinterpret_cast<const f32x4*>(Cs + rr * EPI_LD + cc + 4);
      }
    }
    __syncthreads();
  }
}

// Halo weight gradient for Conv1d with 2 <= taps <= 9 (C_in, C_out multiples of 64, T a
// multiple of 64), the split-K path for grids that conv_wgrad_band (wgrad.hip) cannot fill:
// a block owns a 64 (o) x 64 (c) tile for ALL taps.  Per 64-row k-tile it stages the dy tile
// (64 x 64) and the x rows of the tile plus the tap halo (64 + taps - 1 rows, zero outside the
// utterance) ONCE, and tap j reads the x image at row offset j.  Both images are [rows][64]
// bf16 (128-B rows) filled by LDS-DMA with the chunk swizzle ((R >> 1) & 3) << 1 and read with
// ds_read_b64_tr_b16 (rows {4g+q} u {16+4g+q} of a 32-row step).  Each wave owns 64 (o) x 16
// (c) for all taps: the dy fragments (4 per k-step) are read once and reused by every tap, a
// tap costs ONE shifted x fragment for 4 MFMAs, and the next taps' x fragments are read under
// the current tap's MFMAs.  Each wave also carries the bias gradient of its 16 o rows.
// Output: the split-K slab layout (and bias slab) of conv_wgrad_tn_glds.
template <int TAPS>
__global__ __launch_bounds__(256, 2) void conv_wgrad_halo(WgradGlds a) {
  constexpr int BO = 64, BC = 64, BK = 64, STAGES = 2;
  constexpr int HX = 8;                      // halo rows allocated (taps <= 9)
  constexpr int A_E = BK * BO;               // dy image
  constexpr int X_E = (BK + HX) * BC;        // x halo image
  constexpr int STAGE_E = A_E + X_E;
  constexpr int MAXKT = 1024;
  __shared__ __attribute__((aligned(1024))) u16 smem[STAGES * STAGE_E + MAXKT + 64];
  short* ktl = reinterpret_cast<short*>(smem + STAGES * STAGE_E);
  int* wcnt = reinterpret_cast<int*>(smem + STAGES * STAGE_E + MAXKT);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3, r16 = lane & 15;

  const int per_split = a.tiles_o * a.tiles_k;  // tiles_k = C_in / 64 here
  const int nwg = per_split * a.splits;
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int z = wg / per_split, rem = wg - z * per_split;
  const int tc = rem % a.tiles_k, to = rem / a.tiles_k;
  const int o0 = to * BO, c0 = tc * BC;
  const int64_t r_begin = (int64_t)z * a.rows_per_split;
  int64_t r_end = r_begin + a.rows_per_split;
  if (r_end > a.M) r_end = a.M;
  const int nk_all = r_end > r_begin ? (int)((r_end - r_begin + BK - 1) / BK) : 0;
  const bool use_list = a.lens != nullptr && nk_all <= MAXKT;
  int nk = nk_all;
  if (use_list) {  // ordered list of k-tiles holding a real row (as conv_wgrad_tn_glds)
    int total = 0;
    for (int cc0 = 0; cc0 < nk_all; cc0 += 256) {
      const int kt = cc0 + tid;
      bool v = false;
      if (kt < nk_all) {
        const int64_t k0 = r_begin + (int64_t)kt * BK;
        v = !rows_all_padding(a.lens, a.T, k0, k0 + BK < r_end ? k0 + BK : r_end);
      }
      const uint64_t mask = __ballot(v);
      if (lane == 0) wcnt[wave] = __popcll(mask);
      __syncthreads();
      int before = total;
      for (int w = 0; w < wave; ++w) before += wcnt[w];
      const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
      if (v) ktl[before + below] = (short)kt;
      for (int w = 0; w < 4; ++w) total += wcnt[w];
      __syncthreads();
    }
    nk = total;
  }

  auto swz = [](int R) { return ((R >> 1) & 3) << 1; };
  const u16* zero = reinterpret_cast<const u16*>(g_zero_line);
  const int lrow = lane >> 3, lch = lane & 7;
  const int HR = BK + a.taps - 1, HP = (HR + 7) / 8;  // x halo rows / 8-row pieces
  auto issue = [&](int kt, int stage) {
    u16* As = smem + stage * STAGE_E;
    u16* Xs = As + A_E;
    const int tile = use_list ? (int)ktl[kt] : kt;
    const int64_t k0 = r_begin + (int64_t)tile * BK;
    // the 64 rows of a k-tile lie in one utterance (T % 64 == 0, splits are 64-row aligned)
    const int64_t u0 = (k0 / a.T) * a.T, u1 = u0 + a.T < a.M ? u0 + a.T : a.M;
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // dy: 8 pieces of 8 rows, 2 per wave
      const int R = (wave * 2 + i) * 8 + lrow;
      const int64_t m = k0 + R;
      const u16* src = m < r_end ? a.dy + m * a.ldy + o0 + ((lch ^ swz(R)) << 3) : zero;
      glds16(src, As + (wave * 2 + i) * 8 * BO);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // x halo: up to 9 pieces, wave + 4 i
      const int pc = wave + 4 * i;
      if (pc < HP) {
        const int h = pc * 8 + lrow;
        const int64_t gr = k0 - a.pad + h;
        // rows past the split's end only meet zero dy rows; only the utterance matters
        const u16* src = (gr >= u0 && gr < u1) ? a.x + gr * a.ldx + c0 + ((lch ^ swz(h)) << 3)
                                               : zero;
        glds16(src, Xs + pc * 8 * BC);
      }
    }
  };

  f32x4 acc[TAPS][4], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < TAPS; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = a.bslab != nullptr && tc == 0;  // block-uniform
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

  // transposed fragment (asm reads, see ds_tr16; the caller waits with lgkm_wait): 16 columns
  // at col0, rows rb + {4g+q} and rb + {16+4g+q}
  auto tr_frag = [&](const u16* img, int rb, int col0) -> bf16x8 {
    const int R = rb + 4 * g + q;
    const int lc = (col0 >> 3) + (p >> 1);
    const int off = R * 64 + ((lc ^ swz(R)) << 3) + ((p & 1) << 2);
    const s16x4 lo = ds_tr16(img + off);
    const s16x4 hi = ds_tr16(img + off + 16 * 64);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };
  auto compute = [&](int stage) {
    const u16* As = smem + stage * STAGE_E;
    const u16* Xs = As + A_E;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // x fragments two taps ahead in a ring of three: tap j's MFMAs wait only for the reads
      // up to its fragment (the LDS latency exceeds one tap's 4 MFMAs)
      bf16x8 fa[4], fb[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = tr_frag(As, ks * 32, i * 16);
      fb[0] = tr_frag(Xs, ks * 32, wave * 16);
      if (TAPS > 1) fb[1] = tr_frag(Xs, ks * 32 + 1, wave * 16);
#pragma unroll
      for (int j = 0; j < TAPS; ++j) {
        if (j + 2 < TAPS) {
          fb[(j + 2) % 3] = tr_frag(Xs, ks * 32 + j + 2, wave * 16);
          lgkm_wait<4>();  // all but the x fragments of taps j + 1, j + 2 landed
        } else if (j + 1 < TAPS) {
          lgkm_wait<2>();
        } else {
          lgkm_wait<0>();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j % 3], acc[j][i], 0, 0, 0);
      }
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i == wave) accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], ones, accb, 0, 0, 0);
      }
    }
  };

  kloop<STAGES, 5>(nk, issue, compute);  // per-wave DMA count varies (<= 5): vmcnt(0)-style

  if (do_bias && r16 == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a.bslab[(int64_t)z * a.Cout + o0 + wave * 16 + 4 * g + r] = accb[r];
  }
  // slab[z][o][j*Cin + c]: 16 consecutive c per row group (64-B runs)
  float* slab = a.slab + (int64_t)z * a.Cout * a.Kp;
#pragma unroll
  for (int j = 0; j < TAPS; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + i * 16 + 4 * g + r;
        const int c = c0 + wave * 16 + r16;
        slab[(int64_t)o * a.Kp + (int64_t)j * a.Cin + c] = acc[j][i][r];
      }
}

// dw[o][c][j] (+)= sum_z slab[z][o][j*Cin + c]; db[o] += sum_z bslab[z][o].  Split order is
// fixed (bitwise reproducible).  taps == 1: the layouts coincide, 4 consecutive elements per
// thread.  taps > 1: one block per (o, 64-channel chunk); slab rows are read as 256-B runs
// per tap and the [c][j] block is written contiguously.
__global__ __launch_bounds__(256) void wgrad_reduce_k1(const float* __restrict__ slab,
                                                       const float* __restrict__ bslab, int splits,
                                                       int Cout, int64_t total, float* dw, float* db) {
  // 64 float4 columns x 4 split groups: group y sums splits y, y+4, ... in order, then the
  // 4 group sums are added in group order (fixed order, bitwise reproducible)
  __shared__ f32x4 red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t i4 = ((int64_t)blockIdx.x * 64 + tx) * 4;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (i4 < total) {
#pragma unroll 4
    for (int zz = ty; zz < splits; zz += 4) s += ld4(slab + zz * total + i4);
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && i4 < total)
    st4(dw + i4, ld4(dw + i4) + (((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx]));
  // bias: one output per thread over the first blocks (block 0 looping over every output
  // made the launch's tail), split loads four at a time, summed in split order
  const int ob = blockIdx.x * 256 + threadIdx.x;
  if (db && ob < Cout) {
    float b = 0.f;
    int zz = 0;
    for (; zz + 3 < splits; zz += 4) {
      const float v0 = bslab[(int64_t)zz * Cout + ob], v1 = bslab[(int64_t)(zz + 1) * Cout + ob];
      const float v2 = bslab[(int64_t)(zz + 2) * Cout + ob], v3 = bslab[(int64_t)(zz + 3) * Cout + ob];
      b += v0;
      b += v1;
      b += v2;
      b += v3;
    }
    for (; zz < splits; ++zz) b += bslab[(int64_t)zz * Cout + ob];
    db[ob] += b;
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_taps(const float* __restrict__ slab,
                                                         const float* __restrict__ bslab,
                                                         int splits, int Cout, int Cin, int taps,
                                                         float* dw, float* db) {
  __shared__ float tile[64 * 33];
  const int o = blockIdx.y, c0 = blockIdx.x * 64;
  const int64_t Kp = (int64_t)taps * Cin, total = (int64_t)Cout * Kp;
  const int nc = Cin - c0 < 64 ? Cin - c0 : 64;
  for (int jb = 0; jb < taps; jb += 32) {
    const int nj = taps - jb < 32 ? taps - jb : 32;
    // 16-B loads: thread e owns 4 consecutive channels of one tap row (nc and every offset
    // are multiples of 4); split slabs four at a time, summed in split order
    for (int e = threadIdx.x; e < 16 * nj; e += 256) {
      const int jj = e >> 4, c = (e & 15) * 4;
      if (c < nc) {
        const int64_t off = (int64_t)o * Kp + (int64_t)(jb + jj) * Cin + c0 + c;
        f32x4 s = ld4(slab + off);
        int zz = 1;
        for (; zz + 3 < splits; zz += 4) {
          const f32x4 v0 = ld4(slab + zz * total + off), v1 = ld4(slab + (zz + 1) * total + off);
          const f32x4 v2 = ld4(slab + (zz + 2) * total + off), v3 = ld4(slab + (zz + 3) * total + off);
          s += v0;
          s += v1;
          s += v2;
          s += v3;
        }
        for (; zz < splits; ++zz) s += ld4(slab + zz * total + off);
        tile[(c + 0) * 33 + jj] = s.x;
        tile[(c + 1) * 33 + jj] = s.y;
        tile[(c + 2) * 33 + jj] = s.z;
        tile[(c + 3) * 33 + jj] = s.w;
      }
    }
    __syncthreads();
    float* out = dw + ((int64_t)o * Cin + c0) * taps;
    for (int e = threadIdx.x; e < nc * nj; e += 256) {
      const int c = e / nj, jj = e - c * nj;
      out[(int64_t)c * taps + jb + jj] += tile[c * 33 + jj];
    }
    __syncthreads();
  }
  if (db && blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.f;
    for (int zz = 0; zz < splits; ++zz) s += bslab[(int64_t)zz * Cout + o];
    db[o] += s;
  }
}

// taps > 1, one workgroup per output row o: the S slab rows (taps * Cin contiguous floats each)
// are summed in split order with 16-B loads, S loads in flight per chunk, into LDS, then added
// to dw[o][c][j] in output order (the [j][c] -> [c][j] transpose through LDS; coalesced 4-B
// read-modify-writes).  Same split order as wgrad_reduce_taps (bitwise equal), a quarter of its
// workgroups, every slab row read as one contiguous run.
constexpr int RROW_MAX = 9 * 1024;
__global__ __launch_bounds__(256) void wgrad_reduce_rows(const float* __restrict__ slab,
                                                         const float* __restrict__ bslab,
                                                         int splits, int Cout, int Cin, int taps,
                                                         float* dw, float* db) {
  __shared__ float row[RROW_MAX];
  const int o = blockIdx.x, Kp = taps * Cin;
  const int64_t total = (int64_t)Cout * Kp;
  const float* src = slab + (int64_t)o * Kp;
  for (int e4 = threadIdx.x; e4 < Kp / 4; e4 += 256) {
    f32x4 s = ld4(src + 4 * e4);
    for (int z = 1; z < splits; ++z) s += ld4(src + z * total + 4 * e4);
    *reinterpret_cast<f32x4*>(row + 4 * e4) = s;
  }
  __syncthreads();
  float* out = dw + (int64_t)o * Kp;
  for (int e = threadIdx.x; e < Kp; e += 256) {
    const int c = e / taps, j = e - c * taps;
    out[e] += row[j * Cin + c];
  }
  if (db && threadIdx.x == 0) {
    float b = 0.f;
    for (int z = 0; z < splits; ++z) b += bslab[(int64_t)z * Cout + o];
    db[o] += b;
  }
}

static_assert(RROW_MAX == kWgradRowsMax, "the planner's limit of wgrad_reduce_rows");

template <int BT, int S>
static bool wgrad_tn_try(const WgradPlan& p, const WgradGlds& a, hipStream_t st) {
  if (p.tile != BT || p.stages != S) return false;
  conv_wgrad_tn_glds<BT, S><<<p.grid, 256, 0, st>>>(a);
  return true;
}
template <int BT>
static bool wgrad_tn_try_stages(const WgradPlan& p, const WgradGlds& a, hipStream_t st) {
  return wgrad_tn_try<BT, 1>(p, a, st) || wgrad_tn_try<BT, 2>(p, a, st) ||
         wgrad_tn_try<BT, 3>(p, a, st) || wgrad_tn_try<BT, 4>(p, a, st);
}
template <int TAPS>
static bool wgrad_halo_try(const WgradPlan& p, const WgradGlds& a, hipStream_t st) {
  if (p.taps != TAPS) return false;
  conv_wgrad_halo<TAPS><<<p.grid, 256, 0, st>>>(a);
  return true;
}

// split slabs [splits][c_out][taps c_in] and the bias partials in ws, then the plan's reduce
int launch_wgrad_splitk(const WgradPlan& p, const WgradCall& c, hipStream_t st) {
  int64_t rps = (c.rows + p.splits - 1) / p.splits;
  rps = (rps + 63) / 64 * 64;
  const int64_t Kp = c.taps * c.c_in;
  float* bslab = c.db ? c.ws + p.splits * c.c_out * Kp : nullptr;
  const WgradGlds a{(const u16*)c.dy, c.ldy, (const u16*)c.x, c.ldx, c.ws, bslab, c.rows,
                    c.seq_len, (int)c.c_in, (int)c.c_out, c.taps, c.pad, (int)Kp, rps,
                    p.tiles_o, p.tiles_k, p.splits, c.lens};
  const bool ok = p.kernel == WGRAD_HALO
                      ? wgrad_halo_try<9>(p, a, st) || wgrad_halo_try<5>(p, a, st) ||
                            wgrad_halo_try<3>(p, a, st)
                      : wgrad_tn_try_stages<128>(p, a, st) || wgrad_tn_try_stages<64>(p, a, st);
  if (!ok) return no_instance("conv_wgrad (split-K)");
  const int Cout = (int)c.c_out, Cin = (int)c.c_in;
  if (p.reduce == WRED_K1) {
    wgrad_reduce_k1<<<p.reduce_grid, 256, 0, st>>>(c.ws, bslab, p.splits, Cout, c.c_out * c.c_in, c.dw, c.db);
  } else if (p.reduce == WRED_ROWS) {
    wgrad_reduce_rows<<<p.reduce_grid, 256, 0, st>>>(c.ws, bslab, p.splits, Cout, Cin, c.taps, c.dw, c.db);
  } else {
    dim3 rg(p.reduce_grid_x, (unsigned)c.c_out);
    wgrad_reduce_taps<<<rg, 256, 0, st>>>(c.ws, bslab, p.splits, Cout, Cin, c.taps, c.dw, c.db);
  }
  return FS2_OK;
}

}  // namespace fs2
