// Conv1d weight gradients on 64 x 64 x taps tiles shared by eight waves (conv_wgrad_wide) and the
// grouped k = 1 weight gradient (wgrad_k1_multi) with the split reduce both use.  The slab-free
// band kernel is in wgrad_band.hip.
#include "glds.hpp"
#include "conv_plan.hpp"

namespace fs2 {

// ---------------------------------------------------------------- wide-tile weight gradient
// conv_wgrad_wide: the same product on 64 (o) x 64 (c) x taps output tiles, the rows split Z
// ways (Z ~ 256 / tiles) into fp32 slabs summed in split order by one reduce launch.
//
// Why: the band kernel's 32 x 32 tile re-streams every dy column block 8 times and every x column
// block 32 times (684 MB through L2 -> LDS per decoder launch against 63 MB of operands), and
// every one of its waves stages its own operands, so each SIMD's one wave pays 9 LDS-DMA
// instructions and 48 transposed reads per 72 MFMAs with nothing to hide their latency.  A
// 64 x 64 tile halves the staged bytes per MAC (dy 64 + x 72 positions of 128 B per 64-row band
// for 64 x 64 x taps outputs), and the block's eight waves SHARE each staged band: wave (wo, wc)
// owns o 32 wo .. + 31 x c 16 wc .. + 15 x all taps (18 accumulator fragments, ~120 VGPRs: two
// waves per SIMD), the 17 LDS-DMA pieces of a band are spread over the waves, and one barrier
// per band guards a ST-slot ring (17 KB per slot).  The tap-register reduction order of the
// band kernel is kept: step s (s < 2) of a band reduces its rows s + 2 m, tap j of step s needs
// halo fragment F[s + j], and each F[f] is read from LDS once for every (s, j) with s + j = f.
// Per wave and band: 4 dy fragments + 10 x fragments (28 transposed reads) for 36 MFMAs.
//
// Rows: bands of 64 rows inside one utterance (T % 64 == 0); bands made only of rows past an
// utterance's length (lens given) are not visited; split z takes the list's bands
// [z nb / Z, (z + 1) nb / Z) in row order.  Within a block the sum runs over bands in order and
// over the two steps of a band in order; the slabs are summed in split order: bitwise
// reproducible for a given lens.  The bias gradient rides on the dy fragments of the waves with
// wc == 0 in the blocks of the first c tile (MFMA against a ones fragment).  Z == 1 adds the
// tile straight into dw / db.
constexpr int WIDE_MAXB = 2048;  // bands (of 64 rows) listed in LDS when lens are given
struct WgradWide {
  const u16* dy;
  int64_t ldy;
  const u16* x;
  int64_t ldx;
  float* dw;
  float* db;
  float* slab;   // [Z][Cout][Cin taps] (Z > 1)
  float* bslab;  // [Z][Cout] (Z > 1, db given)
  int64_t M, T;
  int Cin, Cout, pad;
  int tiles_o, tiles_c, Z;
  const int64_t* lens;
};

template <int TAPS, int ST>
__global__ __launch_bounds__(512, 4) void conv_wgrad_wide(WgradWide a) {
  constexpr int BO = 64, BC = 64, S = 2, BR = 64, NT = 512;
  constexpr int HR = BR + TAPS - 1, RS = (HR + 1) / 2, NF = S + TAPS - 1;
  constexpr int PB = 128;                                // bytes per image position (64 bf16)
  constexpr int DPOS = BR, XPOS = (2 * RS + 7) / 8 * 8;  // image positions
  constexpr int NPD = DPOS / 8, NPX = XPOS / 8, NP = NPD + NPX;  // 1-KB LDS-DMA pieces per band
  static_assert(NP > 8 && NP <= 24, "piece bookkeeping: 2 or 3 pieces per wave");
  constexpr int STAGE_B = (DPOS + XPOS) * PB;
  constexpr int RING_B = ST * STAGE_B;
  static_assert(RING_B < 65536, "fragment offsets fit the ds immediate");
  constexpr int QLD = BC * TAPS + 4;  // fp32 row stride of a 16-row epilogue slice
  constexpr int EPI_B = 16 * QLD * 4 > 64 * 68 * 4 ? 16 * QLD * 4 : 64 * 68 * 4;
  constexpr int SMEM_B = RING_B > EPI_B ? RING_B : EPI_B;
  constexpr int MAXB = WIDE_MAXB;
  constexpr int LOOK = 1;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM_B + 4 * MAXB + 64];
  short* blist = reinterpret_cast<short*>(smem + SMEM_B);          // band index
  short* brem = reinterpret_cast<short*>(smem + SMEM_B + 2 * MAXB);  // its rows below the length
  int* wcnt = reinterpret_cast<int*>(smem + SMEM_B + 4 * MAXB);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wo = wave >> 2, wc = wave & 3;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3, r16 = lane & 15;

  // block -> (split, o tile, c tile): XCD-contiguous runs, c fastest, then o, then split (an
  // XCD's blocks share the rows of one split)
  // (the bias gradient: Z * ceil(Cout / 64) further blocks after the tiles, see below)
  const int nmain = a.tiles_o * a.tiles_c * a.Z;
  const int nwg = nmain + (a.db != nullptr ? a.Z * a.tiles_o : 0);
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const bool bias_blk = wg >= nmain;  // block-uniform
  const int wb = wg - nmain;
  const int tc = bias_blk ? 0 : wg % a.tiles_c, t2 = bias_blk ? 0 : wg / a.tiles_c;
  const int to = bias_blk ? wb % a.tiles_o : t2 % a.tiles_o;
  const int z = bias_blk ? wb / a.tiles_o : t2 / a.tiles_o;
  const int o0 = to * BO, c0 = tc * BC;

  // bands holding a real row, in row order, with the count of their rows below the length
  // (the launcher admits lens only with nb_all <= MAXB).  Kept in LDS: a global load of lens in
  // the main loop would make the compiler wait vmcnt(0), draining the LDS-DMA ring every band.
  const int nbu = (int)(a.T / BR);
  const int nb_all = (int)(a.M / BR);
  const bool use_list = a.lens != nullptr;
  int nb = nb_all;
  if (use_list) {
    int total = 0;
    for (int k0 = 0; k0 < nb_all; k0 += NT) {
      const int k = k0 + tid;
      bool v = false;
      int rem = 0;
      if (k < nb_all) {
        const int b = k / nbu;
        const int64_t r = a.lens[b] - (int64_t)(k - b * nbu) * BR;
        v = r > 0;
        rem = r < BR ? (int)r : BR;
      }
      const uint64_t mask = __ballot(v);
      if (lane == 0) wcnt[wave] = __popcll(mask);
      __syncthreads();
      int before = total;
      for (int w = 0; w < wave; ++w) before += wcnt[w];
      const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
      if (v) {
        blist[before + below] = (short)k;
        brem[before + below] = (short)rem;
      }
      for (int w = 0; w < 8; ++w) total += wcnt[w];
      __syncthreads();
    }
    nb = total;
  }
  const int kb0 = (int)((int64_t)z * nb / a.Z), kb1 = (int)((int64_t)(z + 1) * nb / a.Z);
  const int nbs = kb1 - kb0;

  if (bias_blk) {
    // db[o0 .. o0 + 63] over this split's bands: thread (row t / 8, 8 columns) loads one 16-B
    // row piece per band (rows past the length skipped), then the 64 row partials of each
    // column are summed in row order through LDS -- kept out of the tile blocks, whose MFMA
    // bias accumulators would cost the registers that keep them at two waves per SIMD
    const int rr = tid >> 3, cc = o0 + (tid & 7) * 8;
    float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < nbs; ++i) {
      const int kk = kb0 + i;
      const int k = use_list ? (int)blist[kk] : kk;
      const int rem = use_list ? (int)brem[kk] : BR;
      const int b = k / nbu, t0 = (k - b * nbu) * BR;
      if (rr < rem && cc < a.Cout) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.dy + ((int64_t)b * a.T + t0 + rr) * a.ldy + cc);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sum[2 * e] += __uint_as_float(w4[e] << 16);
          sum[2 * e + 1] += __uint_as_float(w4[e] & 0xffff0000u);
        }
      }
    }
    float* R = reinterpret_cast<float*>(smem);  // [64 rows][64 + 4 columns]
#pragma unroll
    for (int e = 0; e < 8; ++e) R[rr * 68 + (tid & 7) * 8 + e] = sum[e];
    __syncthreads();
    if (tid < BO && o0 + tid < a.Cout) {
      float acc = 0.f;
      for (int r = 0; r < 64; ++r) acc += R[r * 68 + tid];
      if (a.Z == 1) a.db[o0 + tid] += acc;
      else a.bslab[(int64_t)z * a.Cout + o0 + tid] = acc;
    }
    return;
  }

  // position P's 16-B chunks are XOR-swizzled by ((P >> 1) & 3) << 1: any 8 consecutive
  // positions read as 16-column transposed fragments hit 64 distinct banks per half-wave
  auto swz = [](int P) { return ((P >> 1) & 3) << 1; };
  // LDS-DMA through buffer descriptors: dy from row 0, x from row -pad (the halo's first row);
  // a band's rows ride in the scalar offset, each piece's lanes have a fixed voffset; rows
  // outside the band's valid range select an out-of-range voffset (zeros)
  const auto dy_rs = buf_rsrc(a.dy, a.M * a.ldy * 2);
  const auto x_rs = buf_rsrc(a.x - (int64_t)a.pad * a.ldx, (a.M + a.pad) * a.ldx * 2);
  const int npw = wave + 16 < NP ? 3 : 2;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)smem;

  auto issue = [&](int i, int slot) {
    const int kk = kb0 + i;
    const int k = __builtin_amdgcn_readfirstlane(use_list ? (int)blist[kk] : kk);
    const int rem = __builtin_amdgcn_readfirstlane(use_list ? (int)brem[kk] : BR);
    const int b = k / nbu, t0 = (k - b * nbu) * BR;
    const int64_t r0 = (int64_t)b * a.T + t0;
    unsigned char* St = smem + slot * STAGE_B;
    // the pieces' per-lane rows / offsets are recomputed here (a few VALU) rather than held
    // across the loop: an opaque copy of the lane id keeps the compiler from hoisting them
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int lpos = ln >> 3, lch = ln & 7;
#pragma unroll
    for (int kp = 0; kp < 3; ++kp) {
      if (kp == 2 && npw < 3) break;
      const int pi = wave + 8 * kp;
      if (pi < NPD) {
        const int P = pi * 8 + lpos;
        const int h = (P & 31) * 2 + (P >> 5);
        const int col = o0 + ((lch ^ swz(P)) << 3);
        const bool ok = col < a.Cout && h < rem;
        glds16_buf(dy_rs, St + pi * 8 * PB, ok ? (uint32_t)((h * a.ldy + col) * 2) : kOOB,
                   (uint32_t)(r0 * a.ldy * 2));
      } else {
        const int P = (pi - NPD) * 8 + lpos;
        const int h = (P % RS) * 2 + P / RS;
        const int col = c0 + ((lch ^ swz(P)) << 3);
        const int t = t0 - a.pad + h;
        const bool ok = pi < NP && P < 2 * RS && h < HR && col < a.Cin && t >= 0 && t < (int)a.T;
        glds16_buf(x_rs, St + pi * 8 * PB, ok ? (uint32_t)((h * a.ldx + col) * 2) : kOOB,
                   (uint32_t)(r0 * a.ldx * 2));
      }
    }
  };
  // wait until this wave's pieces of all but the `ahead` youngest issued bands have landed
  auto vm = [&](int ahead) {
    const int n = ahead * npw;
    switch (n) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    }
  };

  f32x4 acc[2][TAPS];
#pragma unroll
  for (int io = 0; io < 2; ++io)
#pragma unroll
    for (int j = 0; j < TAPS; ++j) acc[io][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane fragment bases: a fragment of 32 positions from pb (rows pb + 4g + q and + 16) and
  // 16 columns at col0 reads base(pb mod 8, col0) + (pb - pb mod 8) * PB (+ 16 PB): the swizzle
  // of position pb + L depends on pb only through pb mod 8
  const int L = 4 * g + q;
  auto fbase = [&](int r, int col0, int img) -> uint32_t {
    const int lc = (col0 >> 3) + (p >> 1);
    return lds0 + (uint32_t)(img + (r + L) * PB + ((lc ^ swz(r + L)) << 4) + ((p & 1) << 3));
  };
  const uint32_t bA0 = fbase(0, wo * 32, 0), bA1 = fbase(0, wo * 32 + 16, 0);
  uint32_t bF[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) bF[r] = fbase(r, wc * 16, DPOS * PB);

  auto compute = [&](auto slot_c) {
    constexpr int SO = decltype(slot_c)::value * STAGE_B;
    bf16x8 A[S][2], F[LOOK + 1];
    static_for<S>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      A[s][0] = tr16_cat(ds_tr16_at<SO + s * 32 * PB>(bA0), ds_tr16_at<SO + (s * 32 + 16) * PB>(bA0));
      A[s][1] = tr16_cat(ds_tr16_at<SO + s * 32 * PB>(bA1), ds_tr16_at<SO + (s * 32 + 16) * PB>(bA1));
    });
    auto rdF = [&](auto fc) -> bf16x8 {
      constexpr int f = decltype(fc)::value;
      constexpr int pb = (f % S) * RS + f / S, r = pb & 7, off = SO + (pb - r) * PB;
      return tr16_cat(ds_tr16_at<off>(bF[r]), ds_tr16_at<off + 16 * PB>(bF[r]));
    };
    static_for<LOOK>([&](auto fc) { F[decltype(fc)::value] = rdF(fc); });
    static_for<NF>([&](auto fc) {
      constexpr int f = decltype(fc)::value;
      if constexpr (f + LOOK < NF) F[(f + LOOK) % (LOOK + 1)] = rdF(std::integral_constant<int, f + LOOK>{});
      constexpr int younger = (NF - 1 - f < LOOK ? NF - 1 - f : LOOK) * 2;
      lgkm_wait<younger>();
      const bf16x8 Ff = F[f % (LOOK + 1)];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int j = f - s;
        if (j < 0 || j >= TAPS) continue;
#pragma unroll
        for (int io = 0; io < 2; ++io)
          acc[io][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[s][io], Ff, acc[io][j], 0, 0, 0);
      }
    });
  };

  // ring: ST - 1 bands issued ahead; per band this wave's pieces waited for (counted vmcnt), one
  // raw barrier (every wave's pieces landed AND every wave finished the band whose slot the
  // refill overwrites: its reads were waited for inside compute), refill, MFMAs.  The loop is
  // unrolled by the ring depth so that each band's slot -- and with it every fragment address
  // -- is a compile-time offset.
  static_assert(ST == 3, "the unrolled ring below");
  for (int i = 0; i < ST - 1 && i < nbs; ++i) issue(i, i);
  auto band = [&](auto slot_c, int i) {
    constexpr int SL = decltype(slot_c)::value;
    const int ahead = nbs - 1 - i < ST - 2 ? nbs - 1 - i : ST - 2;
    vm(ahead);
    __builtin_amdgcn_s_barrier();
    if (i + ST - 1 < nbs) issue(i + ST - 1, (SL + ST - 1) % ST);
    compute(slot_c);
  };
  int i = 0;
  for (; i + 3 <= nbs; i += 3) {
    band(std::integral_constant<int, 0>{}, i);
    band(std::integral_constant<int, 1>{}, i + 1);
    band(std::integral_constant<int, 2>{}, i + 2);
  }
  if (i < nbs) band(std::integral_constant<int, 0>{}, i);
  if (i + 1 < nbs) band(std::integral_constant<int, 1>{}, i + 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // epilogue: four 16-row slices of the tile through LDS in the dw layout ([o][c][j]), stored
  // as f32x4 rows (Z == 1: added into dw; else written to this split's slab)
  float* Q = reinterpret_cast<float*>(smem);
  const int64_t Kp = (int64_t)a.Cin * TAPS;
  const int ncol = (a.Cin - c0 < BC ? a.Cin - c0 : BC) * TAPS;  // valid floats per row
  float* dst_base = a.Z == 1 ? a.dw : a.slab + (int64_t)z * a.Cout * Kp;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (wo == (k >> 1)) {
      const int io = k & 1;
#pragma unroll
      for (int j = 0; j < TAPS; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) Q[(4 * g + r) * QLD + (wc * 16 + r16) * TAPS + j] = acc[io][j][r];
    }
    __syncthreads();
    constexpr int V = BC * TAPS / 4;
    for (int e = tid; e < 16 * V; e += NT) {
      const int row = e / V, v4 = e - row * V;
      const int o = o0 + 16 * k + row;
      if (o >= a.Cout || 4 * v4 >= ncol) continue;
      const f32x4 v = ld4(Q + row * QLD + 4 * v4);
      float* d = dst_base + (int64_t)o * Kp + (int64_t)c0 * TAPS + 4 * v4;
      if (a.Z == 1) st4(d, ld4(d) + v);
      else st4(d, v);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- grouped k = 1 weight gradient
// wgrad_k1_multi: the k = 1 weight gradients of one FFT block -- QKV (768 x 256 + bias), fc
// (256 x 256) and w_2 (256 x 1024) at the decoder shapes, transformer/SubLayers.py:39-55,88 --
// in ONE launch.  Their products are tall reductions (24,576 rows, 0.2 MFLOP per output), so
// they run split-K: a 128 (o) x 128 (c) output tile over a range of rows per block, fp32
// partial tiles into split slabs, summed in split order by ONE reduce launch.  Grouping the
// three GEMMs puts 32 output tiles into the grid instead of 4-16, so the same 256 blocks need 8
// row splits instead of 21-64: a third of the slab bytes, long row loops (48 k-tiles) that
// amortise the prologue / epilogue, and 2 launches per block instead of 6.
// Block: 8 waves; wave w owns the 64 x 64 quadrant w & 3 over rows 32 (w >> 2) .. + 31 of each
// 64-row k-tile (the two row halves of a quadrant are summed through LDS at the end).  The
// k-tiles (dy [64 rows][128 o] and x [64 rows][128 c], 256-B rows, LDS-DMA through buffer
// descriptors) run through a 4-slot ring with three tiles in flight (counted vmcnt, one raw
// barrier per tile).  Transposed fragments (ds_read_b64_tr_b16) with the chunk swizzle
// (R & 7) << 1: a 32-lane read hits 16 distinct bank slots.  The bias gradient rides on the dy
// fragments of the blocks of the first c tile (an MFMA against a ones fragment).
struct K1Job {
  const u16* dy;
  int64_t ldy;
  const u16* x;
  int64_t ldx;
  float* dw;
  float* db;
  float* slab;   // [splits][Cout][Cin]
  float* bslab;  // [splits][Cout] (db != NULL)
  int64_t rps;   // rows per split (multiple of 64)
  int Cin, Cout, tiles_o, tiles_c, splits, begin;  // begin: the job's first block
};
constexpr int K1_MAXJ = 4;
struct K1Multi {
  K1Job job[K1_MAXJ];
  int n, nblocks;
  int64_t M, T;
  const int64_t* lens;
};

template <int STAGES>
__global__ __launch_bounds__(512, 1) void wgrad_k1_multi(K1Multi m) {
  constexpr int BO = 128, BC = 128, BK = 64, NT = 512;
  constexpr int IMG = BK * 128;     // one operand image: [64 rows][128] bf16 (256-B rows)
  constexpr int STAGE_E = 2 * IMG;  // dy image then x image (32 KB)
  constexpr int EPI_LD = 64 + 4;    // fp32 epilogue rows of a 64 x 64 quadrant
  constexpr int EPI_B = (4 * 64 * EPI_LD + 4 * 64) * 4;
  constexpr int SMEM_B = STAGES * STAGE_E * 2 > EPI_B ? STAGES * STAGE_E * 2 : EPI_B;
  constexpr int MAXKT = 1024;
  __shared__ __attribute__((aligned(1024))) u16 smem[SMEM_B / 2 + MAXKT + 64];
  short* ktl = reinterpret_cast<short*>(smem + SMEM_B / 2);
  int* wcnt = reinterpret_cast<int*>(smem + SMEM_B / 2 + MAXKT);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = wave & 3, half = wave >> 2;
  const int qo = (quad >> 1) * 64, qc = (quad & 1) * 64;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3, r16 = lane & 15;

  // XCD-contiguous block runs; a job's blocks are split-major, tiles fastest (an XCD's blocks
  // share the rows of dy and x)
  const int nwg = m.nblocks;
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  int jb = 0;
#pragma unroll
  for (int j = 1; j < K1_MAXJ; ++j)
    if (j < m.n && wg >= m.job[j].begin) jb = j;
  const K1Job J = m.job[jb];
  const int local = wg - J.begin, tiles = J.tiles_o * J.tiles_c;
  const int z = local / tiles, tile = local - z * tiles;
  const int to = tile / J.tiles_c, tc = tile - to * J.tiles_c;
  const int o0 = to * BO, c0 = tc * BC;
  const int64_t r_begin = (int64_t)z * J.rps;
  int64_t r_end = r_begin + J.rps;
  if (r_end > m.M) r_end = m.M;
  const int nk_all = r_end > r_begin ? (int)((r_end - r_begin + BK - 1) / BK) : 0;
  // ordered list of the split's k-tiles holding a real row
  const bool use_list = m.lens != nullptr && nk_all <= MAXKT;
  int nk = nk_all;
  if (use_list) {
    int total = 0;
    for (int cc0 = 0; cc0 < nk_all; cc0 += NT) {
      const int kt = cc0 + tid;
      bool v = false;
      if (kt < nk_all) {
        const int64_t k0 = r_begin + (int64_t)kt * BK;
        v = !rows_all_padding(m.lens, m.T, k0, k0 + BK < r_end ? k0 + BK : r_end);
      }
      const uint64_t mask = __ballot(v);
      if (lane == 0) wcnt[wave] = __popcll(mask);
      __syncthreads();
      int before = total;
      for (int w = 0; w < wave; ++w) before += wcnt[w];
      const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
      if (v) ktl[before + below] = (short)kt;
      for (int w = 0; w < 8; ++w) total += wcnt[w];
      __syncthreads();
    }
    nk = total;
  }

  // staging: a wave-instruction fills 4 image rows x 256 B; image row R = (2 wave + i) * 4 +
  // lane / 16 (i < 2), physical 16-B chunk lane & 15 holding logical chunk (lane & 15) ^ swz(R).
  // Buffer descriptors over the split's rows (the k-tile advance rides in the scalar offset);
  // chunks past the channel count and rows past the split's end select an out-of-range voffset.
  auto swz = [](int R) { return (R & 7) << 1; };
  const auto dy_rs = buf_rsrc(J.dy + r_begin * J.ldy, (r_end - r_begin) * J.ldy * 2);
  const auto x_rs = buf_rsrc(J.x + r_begin * J.ldx, (r_end - r_begin) * J.ldx * 2);
  int Rl[2];
  uint32_t a_vo[2], b_vo[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int R = (wave * 2 + i) * 4 + (lane >> 4);
    const int lc = (lane & 15) ^ swz(R);
    Rl[i] = R;
    a_vo[i] = o0 + lc * 8 < J.Cout ? (uint32_t)((R * J.ldy + o0 + lc * 8) * 2) : kOOB;
    b_vo[i] = c0 + lc * 8 < J.Cin ? (uint32_t)((R * J.ldx + c0 + lc * 8) * 2) : kOOB;
  }
  const int rows = (int)(r_end - r_begin);
  auto issue = [&](int kt, int stage) {
    u16* As = smem + stage * STAGE_E;
    u16* Bs = As + IMG;
    const int tl = __builtin_amdgcn_readfirstlane(use_list ? (int)ktl[kt] : kt);
    const int lim = rows - tl * BK;  // rows of this k-tile inside the split
    const uint32_t sa = (uint32_t)(tl * BK * J.ldy * 2), sb = (uint32_t)(tl * BK * J.ldx * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool ok = Rl[i] < lim;
      glds16_buf(dy_rs, As + (wave * 2 + i) * 4 * 128, ok ? a_vo[i] : kOOB, sa);
      glds16_buf(x_rs, Bs + (wave * 2 + i) * 4 * 128, ok ? b_vo[i] : kOOB, sb);
    }
  };

  f32x4 acc[4][4], accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bool do_bias = J.db != nullptr && tc == 0 && (quad & 1) == 0;  // wave-uniform
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  const int rbase = half * 32 + 4 * g + q, sw = swz(rbase);
  auto tr = [&](const u16* img, int col0, int hi) -> s16x4 {
    const int lc = (col0 >> 3) + (p >> 1);
    return ds_tr16(img + (rbase + 16 * hi) * 128 + ((lc ^ sw) << 3) + ((p & 1) << 2));
  };
  auto compute = [&](int stage) {
    const u16* As = smem + stage * STAGE_E;
    const u16* Bs = As + IMG;
    s16x4 ra[4][2], rb[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i][0] = tr(As, qo + i * 16, 0);
      ra[i][1] = tr(As, qo + i * 16, 1);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rb[j][0] = tr(Bs, qc + j * 16, 0);
      rb[j][1] = tr(Bs, qc + j * 16, 1);
    }
    bf16x8 fa[4];
    // c fragment j's MFMAs wait only for the reads up to it (4-bit counter: the 16th read
    // issues once the first has retired, so 6 - 2 j younger reads remain in flight)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j == 0) lgkm_wait<6>();
      else if (j == 1) lgkm_wait<4>();
      else if (j == 2) lgkm_wait<2>();
      else lgkm_wait<0>();
      if (j == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = tr16_cat(ra[i][0], ra[i][1]);
      }
      const bf16x8 fb = tr16_cat(rb[j][0], rb[j][1]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[i][j], 0, 0, 0);
    }
    if (do_bias) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], ones, accb[i], 0, 0, 0);
    }
  };

  // ring: STAGES - 1 tiles issued ahead; per tile a counted vmcnt (this tile landed, the later
  // ones stay in flight), one raw barrier (every wave's pieces landed AND every wave finished the
  // previous tile, whose slot the refill overwrites), refill, MFMAs
  for (int t = 0; t < STAGES - 1 && t < nk; ++t) issue(t, t);
  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = nk - 1 - kt < STAGES - 2 ? nk - 1 - kt : STAGES - 2;
    if (ahead >= 2 && STAGES >= 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + STAGES - 1 < nk) issue(kt + STAGES - 1, (kt + STAGES - 1) % STAGES);
    compute(kt % STAGES);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // the two row halves of each quadrant through LDS: half 1 writes, half 0 adds and stores
  float* Cs = reinterpret_cast<float*>(smem);
  float* Bp = Cs + 4 * 64 * EPI_LD;
  if (half == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          Cs[(quad * 64 + i * 16 + 4 * g + r) * EPI_LD + j * 16 + r16] = acc[i][j][r];
    if (do_bias && r16 == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) Bp[quad * 64 + i * 16 + 4 * g + r] = accb[i][r];
    }
  }
  __syncthreads();
  if (half == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          Cs[(quad * 64 + i * 16 + 4 * g + r) * EPI_LD + j * 16 + r16] += acc[i][j][r];
    if (do_bias && r16 == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) Bp[quad * 64 + i * 16 + 4 * g + r] += accb[i][r];
    }
  }
  __syncthreads();
  {
    // 128 x 128 outputs, 32 per thread: row o = tid / 4, 32 consecutive c; quadrant rows
    const int o = tid >> 2, cc = (tid & 3) * 32;
    const int qd = (o >> 6) * 2 + (cc >> 6), ro = o & 63, co = cc & 63;
    float* slab = J.slab + (int64_t)z * J.Cout * J.Cin;
    if (o0 + o < J.Cout) {
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(Cs + (qd * 64 + ro) * EPI_LD + co + 4 * v);
        if (c0 + cc + 4 * v < J.Cin)
          *reinterpret_cast<f32x4*>(slab + (int64_t)(o0 + o) * J.Cin + c0 + cc + 4 * v) = t;
      }
    }
    if (J.db != nullptr && tc == 0 && tid < BO && o0 + tid < J.Cout)
      J.bslab[(int64_t)z * J.Cout + o0 + tid] = Bp[((tid >> 6) * 2) * 64 + (tid & 63)];
  }
}

// dw_j += sum_z slab_j[z] (f32x4 units), db_j += sum_z bslab_j[z]: the splits in order (fixed:
// bitwise reproducible), eight split loads in flight per thread
struct K1Red {
  const float* slab[K1_MAXJ];
  const float* bslab[K1_MAXJ];
  float* dw[K1_MAXJ];
  float* db[K1_MAXJ];
  int64_t u_begin[K1_MAXJ + 1];  // f32x4 units of the weight gradients, per job
  int64_t b_begin[K1_MAXJ + 1];  // bias outputs, per job (after every weight unit)
  int splits[K1_MAXJ];
  int n;
};
__global__ __launch_bounds__(256) void wgrad_k1_multi_reduce(K1Red r) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < r.u_begin[r.n]) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < K1_MAXJ; ++k)
      if (k < r.n && e >= r.u_begin[k]) j = k;
    const int64_t i4 = (e - r.u_begin[j]) * 4, total = (r.u_begin[j + 1] - r.u_begin[j]) * 4;
    const float* s = r.slab[j] + i4;
    const int S = r.splits[j];
    f32x4 acc = ld4(s);
    int zz = 1;
    for (; zz + 7 < S; zz += 8) {
      f32x4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = ld4(s + (int64_t)(zz + k) * total);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; zz < S; ++zz) acc += ld4(s + (int64_t)zz * total);
    float* d = r.dw[j] + i4;
    st4(d, ld4(d) + acc);
    return;
  }
  const int64_t eb = e - r.u_begin[r.n];
  if (eb >= r.b_begin[r.n]) return;
  int j = 0;
#pragma unroll
  for (int k = 1; k < K1_MAXJ; ++k)
    if (k < r.n && eb >= r.b_begin[k]) j = k;
  const int64_t o = eb - r.b_begin[j], cout = r.b_begin[j + 1] - r.b_begin[j];
  float acc = 0.f;
  for (int zz = 0; zz < r.splits[j]; ++zz) acc += r.bslab[j][(int64_t)zz * cout + o];
  r.db[j][o] += acc;
}

// jobs: host int64 rows {dy, ldy, x, ldx, dw, db, c_in, c_out}; p = plan_wgrad_k1_multi of them
int launch_wgrad_k1_multi(const WgradPlan& p, const int64_t* jobs, int n, int64_t rows,
                          int64_t seq_len, const int64_t* lens, float* ws, hipStream_t st) {
  FS2_CHECK_ARG(n >= 1 && n <= K1_MAXJ, "fs2_conv_wgrad_k1_multi: 1..%d jobs", K1_MAXJ);
  for (int j = 0; j < n; ++j) {
    const int64_t* r = jobs + 8 * j;
    FS2_CHECK_ARG(r[6] % 8 == 0 && r[7] % 8 == 0 && r[1] % 8 == 0 && r[3] % 8 == 0 &&
                      (r[0] & 15) == 0 && (r[2] & 15) == 0 && (r[4] & 15) == 0,
                  "fs2_conv_wgrad_k1_multi: channel counts / strides must be multiples of 8, "
                  "operands 16-B aligned");
  }
  const int S = p.splits;
  int64_t rps = (rows + S - 1) / S;
  rps = (rps + 63) / 64 * 64;
  for (int j = 0; j < n; ++j) {
    const int64_t ld = jobs[8 * j + 1] > jobs[8 * j + 3] ? jobs[8 * j + 1] : jobs[8 * j + 3];
    FS2_CHECK_ARG((rps + 64) * ld * 2 < ((int64_t)1 << 31),
                  "fs2_conv_wgrad_k1_multi: a row split exceeds 32-bit buffer offsets");
  }
  K1Multi m{};
  K1Red red{};
  m.n = red.n = n;
  m.M = rows;
  m.T = seq_len;
  m.lens = lens;
  int begin = 0;
  int64_t f = 0, ub = 0, bb = 0;
  for (int j = 0; j < n; ++j) {
    const int64_t* r = jobs + 8 * j;
    K1Job& J = m.job[j];
    J.dy = (const u16*)r[0];
    J.ldy = r[1];
    J.x = (const u16*)r[2];
    J.ldx = r[3];
    J.dw = (float*)r[4];
    J.db = (float*)r[5];
    J.Cin = (int)r[6];
    J.Cout = (int)r[7];
    J.tiles_o = (J.Cout + 127) / 128;
    J.tiles_c = (J.Cin + 127) / 128;
    J.splits = S;
    J.rps = rps;
    J.begin = begin;
    begin += J.tiles_o * J.tiles_c * S;
    J.slab = ws + f;
    f += (int64_t)S * J.Cout * J.Cin;
    J.bslab = J.db ? ws + f : nullptr;
    if (J.db) f += (int64_t)S * J.Cout;
    f = (f + 3) / 4 * 4;
    red.slab[j] = J.slab;
    red.bslab[j] = J.bslab;
    red.dw[j] = J.dw;
    red.db[j] = J.db;
    red.splits[j] = S;
    red.u_begin[j] = ub;
    ub += (int64_t)J.Cout * J.Cin / 4;
    red.b_begin[j] = bb;
    bb += J.db ? J.Cout : 0;
  }
  red.u_begin[n] = ub;
  red.b_begin[n] = bb;
  m.nblocks = begin;
  if ((unsigned)begin != p.grid) return no_instance("wgrad_k1_multi (grid)");  // the plan's tiles x splits
  if (p.stages == 2) wgrad_k1_multi<2><<<p.grid, 512, 0, st>>>(m);
  else if (p.stages == 3) wgrad_k1_multi<3><<<p.grid, 512, 0, st>>>(m);
  else wgrad_k1_multi<4><<<p.grid, 512, 0, st>>>(m);
  wgrad_k1_multi_reduce<<<p.reduce_grid, 256, 0, st>>>(red);
  return FS2_OK;
}

// ---------------------------------------------------------------- wide-tile launcher
static_assert(WIDE_MAXB == kWideMaxBands, "the planner's limit of conv_wgrad_wide");

template <int TAPS>
static bool wide_try(const WgradPlan& p, const WgradWide& a, hipStream_t st) {
  if (p.taps != TAPS) return false;
  conv_wgrad_wide<TAPS, 3><<<p.grid, 512, 0, st>>>(a);
  return true;
}

// splits > 1: split slabs and bias partials in ws, summed by wgrad_k1_multi_reduce
int launch_wgrad_wide(const WgradPlan& p, const WgradCall& c, hipStream_t st) {
  const int Z = p.splits;
  const int64_t Kp = c.c_in * c.taps;
  float* bslab = (Z > 1 && c.db) ? c.ws + (int64_t)Z * c.c_out * Kp : nullptr;
  const WgradWide a{(const u16*)c.dy, c.ldy, (const u16*)c.x, c.ldx, c.dw, c.db,
                    Z > 1 ? c.ws : nullptr, bslab, c.rows, c.seq_len, (int)c.c_in, (int)c.c_out,
                    c.pad, p.tiles_o, p.tiles_k, Z, c.lens};
  const bool ok = wide_try<9>(p, a, st) || wide_try<5>(p, a, st) || wide_try<3>(p, a, st);
  if (!ok) return no_instance("conv_wgrad_wide");
  if (Z > 1) {
    K1Red red{};
    red.n = 1;
    red.slab[0] = c.ws;
    red.bslab[0] = bslab;
    red.dw[0] = c.dw;
    red.db[0] = c.db;
    red.splits[0] = Z;
    red.u_begin[0] = 0;
    red.u_begin[1] = c.c_out * Kp / 4;
    red.b_begin[0] = 0;
    red.b_begin[1] = c.db ? c.c_out : 0;
    wgrad_k1_multi_reduce<<<p.reduce_grid, 256, 0, st>>>(red);
  }
  return FS2_OK;
}

}  // namespace fs2
