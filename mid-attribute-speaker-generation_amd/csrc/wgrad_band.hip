// Conv1d weight gradient without split-K slabs: conv_wgrad_band.
//
//   dw[o, c, j] += sum_r dy[r, o] * x[r + j - pad, c]        (taps 3 / 5 / 9)
//   db[o]       += sum_r dy[r, o]
//
// Replaces the weight half of ConvolutionBackward for the FFT-block Conv1d FFN
// (transformer/SubLayers.py:85-93), the PostNet convs (transformer/Layers.py:129-137) and the
// variance-predictor convs (model/modules.py:209-250).
//
// The product is a tall reduction: 24,576 rows against a 1,024 x 2,304 output for the decoder
// FFN.  The round-3 kernel split the rows over 8 blocks per output tile and round-tripped eight
// fp32 slabs (72 MB written, 81 MB read back by a reduce launch, for a 9.4 MB result).  Here
// one block owns a 32 (o) x 32 (c) x taps output tile for ALL rows, so the grid is the output
// tiles (256 blocks for the decoder / encoder FFN and the PostNet 512 x 512 convs) and no slab
// exists: the four waves of a block each take every fourth band of rows, hold the whole tile
// in registers (taps x 2 x 2 fragments of v_mfma_f32_16x16x32_bf16), and are summed in a fixed
// order through LDS at the end ((w0 + w2) + (w1 + w3): bitwise reproducible), then added
// straight into dw / db.
//
// Bands.  A band is 32 S consecutive rows inside one utterance (T % 32 S == 0).  Its step s
// (s < S) is the 32-deep MFMA reduction over the rows s + S m (m = 0..31), so tap j of step s
// needs the input rows s + j + S m of the band's halo: halo fragment F[s + j], where F[f] are
// the halo rows f + S m (f < S + taps - 1).  Each halo fragment is read from LDS ONCE and feeds
// every (s, j) with s + j = f -- the tap-register idea of conv_gemm_tapreg applied to the
// reduction dimension (rows may be paired with MFMA k-slots in any order, as long as dy and x
// use the same one).  The dy image stores band row h at position (h mod S) * 32 + h / S and the
// x image halo row h at (h mod S) * RS + h / S, so every fragment is 32 consecutive positions.
// Positions are 64-B rows (32 bf16 columns); the 32-B halves swap at (P >> 2) & 1, which makes
// the ds_read_b64_tr_b16 fragment reads conflict-free at any starting position.
//
// Each wave stages its own bands through its own ST-slot LDS ring by LDS-DMA and waits only for
// its own loads (counted vmcnt): there is no barrier in the main loop.  Rows past an
// utterance's length (lens given) are staged from the zero line, and bands made only of them
// are not visited.  The bias gradient rides on the dy fragments of the blocks of the first c
// tile (an MFMA against a ones fragment).
#include "glds.hpp"
#include "conv_plan.hpp"

namespace fs2 {

struct WgradBand {
  const u16* dy;
  int64_t ldy;
  const u16* x;
  int64_t ldx;
  float* dw;
  float* db;
  int64_t M, T;
  int Cin, Cout, pad;
  int tiles_o, tiles_c;
  const int64_t* lens;
};

template <int TAPS, int S, int ST, int W>
__global__ __launch_bounds__(64 * W, W == 8 ? 1 : 2) void conv_wgrad_band(WgradBand a) {
  constexpr int BO = 32, BC = 32, BR = 32 * S, NT = 64 * W;
  constexpr int HR = BR + TAPS - 1, RS = (HR + S - 1) / S, NF = S + TAPS - 1;
  constexpr int PB = 64;                                     // bytes per image position
  constexpr int DPOS = BR, XPOS = (S * RS + 15) / 16 * 16;  // image positions
  constexpr int NQD = DPOS / 16, NQX = XPOS / 16, NQ = NQD + NQX;  // LDS-DMA per band
  constexpr int STAGE_B = (DPOS + XPOS) * PB;                     // bytes per ring slot
  constexpr int RING_B = W * ST * STAGE_B;
  static_assert(RING_B < 65536 + W * ST * STAGE_B, "offsets");
  constexpr int QLD = BC * TAPS + 4;  // fp32 row stride of a dW-layout partial tile
  constexpr int RED_B = (W / 2) * (BO * QLD * 4 + 2 * 64 * 16);  // W / 2 partial tiles + bias
  static_assert(TAPS * 16 * 64 <= BO * QLD, "native partial fits a region");
  constexpr int MAXB = 1024;
  // the band list sits behind the ring, inside the reduction region (used after the main loop):
  // 77 KB in all, two blocks per CU
  constexpr int LIST_B = RING_B + 4 * MAXB + 64;
  constexpr int SMEM_B = LIST_B > RED_B ? LIST_B : RED_B;
  constexpr int LOOK = 2;  // halo fragments read ahead of their MFMAs
  static_assert(NQ * (ST - 2 > 0 ? ST - 2 : 1) <= 63 && ST == 2, "vmcnt bookkeeping / the unrolled ring");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM_B];
  short* blist = reinterpret_cast<short*>(smem + RING_B);          // band index
  short* brem = reinterpret_cast<short*>(smem + RING_B + 2 * MAXB);  // its rows below the length
  int* wcnt = reinterpret_cast<int*>(smem + RING_B + 4 * MAXB);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3, r16 = lane & 15;

  // output tile: XCD-contiguous runs, c fastest (an XCD's blocks share their dy columns in L2)
  const int nwg = a.tiles_o * a.tiles_c;
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int to = wg / a.tiles_c, tc = wg - to * a.tiles_c;
  const int o0 = to * BO, c0 = tc * BC;

  // bands holding a real row, in row order, with their rows below the length (the launcher
  // admits lens only with nb_all <= MAXB).  In LDS: a global load of lens in the main loop
  // would make the compiler wait vmcnt(0) there, draining the LDS-DMA ring every band.
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
      for (int w = 0; w < W; ++w) total += wcnt[w];
      __syncthreads();
    }
    nb = total;
  }
  const int nbw = nb > wave ? (nb - wave + W - 1) / W : 0;  // this wave: bands wave + W i

  // the 32-B halves of position P swap at (P >> 2) & 1 (16-B chunk index ^ 2)
  auto swz = [](int P) { return ((P >> 2) & 1) << 1; };
  // LDS-DMA through buffer descriptors: dy from row 0, x from row -pad; the band's first row
  // rides in the scalar offset
  const auto dy_rs = buf_rsrc(a.dy, a.M * a.ldy * 2);
  const auto x_rs = buf_rsrc(a.x - (int64_t)a.pad * a.ldx, (a.M + a.pad) * a.ldx * 2);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)smem;
  unsigned char* ring = smem + wave * ST * STAGE_B;

  auto issue = [&](int i, int slot) {
    const int kk = wave + W * i;
    const int k = __builtin_amdgcn_readfirstlane(use_list ? (int)blist[kk] : kk);
    const int rem = __builtin_amdgcn_readfirstlane(use_list ? (int)brem[kk] : BR);
    const int b = k / nbu, t0 = (k - b * nbu) * BR;
    const int64_t r0 = (int64_t)b * a.T + t0;
    unsigned char* St = ring + slot * STAGE_B;
    // per-lane offsets recomputed here (an opaque lane id keeps them out of the registers
    // held across the loop)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int lpos = ln >> 2, lch = ln & 3;
#pragma unroll
    for (int qi = 0; qi < NQD; ++qi) {
      const int P = qi * 16 + lpos;
      const int h = (P & 31) * S + (P >> 5);
      const int col = o0 + ((lch ^ swz(P)) << 3);
      const bool ok = h < rem && col < a.Cout;
      glds16_buf(dy_rs, St + qi * 16 * PB, ok ? (uint32_t)((h * a.ldy + col) * 2) : kOOB,
                 (uint32_t)(r0 * a.ldy * 2));
    }
#pragma unroll
    for (int qi = 0; qi < NQX; ++qi) {
      const int P = qi * 16 + lpos;
      const int h = (P % RS) * S + P / RS;
      const int col = c0 + ((lch ^ swz(P)) << 3);
      const int t = t0 - a.pad + h;
      const bool ok = P < S * RS && h < HR && t >= 0 && t < (int)a.T && col < a.Cin;
      glds16_buf(x_rs, St + (DPOS + qi * 16) * PB, ok ? (uint32_t)((h * a.ldx + col) * 2) : kOOB,
                 (uint32_t)(r0 * a.ldx * 2));
    }
  };

  f32x4 acc[TAPS][2][2], accb[2];
#pragma unroll
  for (int j = 0; j < TAPS; ++j)
#pragma unroll
    for (int io = 0; io < 2; ++io)
#pragma unroll
      for (int ic = 0; ic < 2; ++ic) acc[j][io][ic] = f32x4{0.f, 0.f, 0.f, 0.f};
  accb[0] = accb[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = a.db != nullptr && tc == 0;  // block-uniform
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

  // per-lane fragment bases: the fragment of 32 positions from pb (rows pb + 4g + q and + 16),
  // 16 columns at col0, reads base(pb mod 8, col0) + (pb - pb mod 8) PB (+ 16 PB): the swizzle
  // of position pb + L depends on pb only through pb mod 8
  const int L = 4 * g + q;
  auto fbase = [&](int r, int col0, int img) -> uint32_t {
    const int lc = (col0 >> 3) + (p >> 1);
    return lds0 + (uint32_t)(wave * ST * STAGE_B + img + (r + L) * PB + ((lc ^ swz(r + L)) << 4) +
                             ((p & 1) << 3));
  };
  uint32_t bA0 = fbase(0, 0, 0), bA1 = fbase(0, 16, 0);
  uint32_t bF[8][2];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int ic = 0; ic < 2; ++ic) bF[r][ic] = fbase(r, ic * 16, DPOS * PB);

  auto compute = [&](auto slot_c) {
    constexpr int SO = decltype(slot_c)::value * STAGE_B;
    bf16x8 A[S][2], F[LOOK + 1][2];
    static_for<S>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      A[s][0] = tr16_cat(ds_tr16_at<SO + s * 32 * PB>(bA0), ds_tr16_at<SO + (s * 32 + 16) * PB>(bA0));
      A[s][1] = tr16_cat(ds_tr16_at<SO + s * 32 * PB>(bA1), ds_tr16_at<SO + (s * 32 + 16) * PB>(bA1));
    });
    auto rdF = [&](auto fc, bf16x8 (&dst)[2]) {
      constexpr int f = decltype(fc)::value;
      constexpr int pb = (f % S) * RS + f / S, r = pb & 7, off = SO + (pb - r) * PB;
      dst[0] = tr16_cat(ds_tr16_at<off>(bF[r][0]), ds_tr16_at<off + 16 * PB>(bF[r][0]));
      dst[1] = tr16_cat(ds_tr16_at<off>(bF[r][1]), ds_tr16_at<off + 16 * PB>(bF[r][1]));
    };
    static_for<LOOK>([&](auto fc) { rdF(fc, F[decltype(fc)::value]); });
    static_for<NF>([&](auto fc) {
      constexpr int f = decltype(fc)::value;
      if constexpr (f + LOOK < NF) rdF(std::integral_constant<int, f + LOOK>{}, F[(f + LOOK) % (LOOK + 1)]);
      constexpr int younger = (NF - 1 - f < LOOK ? NF - 1 - f : LOOK) * 4;
      lgkm_wait<younger>();
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int j = f - s;
        if (j < 0 || j >= TAPS) continue;
#pragma unroll
        for (int io = 0; io < 2; ++io)
#pragma unroll
          for (int ic = 0; ic < 2; ++ic)
            acc[j][io][ic] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[s][io], F[f % (LOOK + 1)][ic],
                                                                     acc[j][io][ic], 0, 0, 0);
        if (j == 0 && do_bias) {
#pragma unroll
          for (int io = 0; io < 2; ++io)
            accb[io] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[s][io], ones, accb[io], 0, 0, 0);
        }
      }
    });
  };

  // per-wave 2-slot ring, no barrier: wait for this wave's band i (counted vmcnt), refill the
  // other slot with band i + 1, compute band i; the fragment bases step to the other slot
  // after each band (one add per base)
  if (nbw > 0) issue(0, 0);
  int dslot = STAGE_B;
  for (int i = 0; i < nbw; ++i) {
    vm_wait_tiles<NQ>(0);
    if (i + 1 < nbw) issue(i + 1, (i + 1) & 1);
    compute(std::integral_constant<int, 0>{});
    bA0 += dslot;
    bA1 += dslot;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      bF[r][0] += dslot;
      bF[r][1] += dslot;
    }
    dslot = -dslot;
  }

  // fixed-order cross-wave sum, a tree through LDS: waves [h, 2h) write their partials, waves
  // [0, h) add them (h = W/2, ..., 2), so wave 0 holds (p0 + p4) + (p2 + p6) and wave 1 the
  // odd pairs (W = 8); both write their sums in the dw layout ([o][c][j], row stride QLD) and
  // every thread adds the two into dw / db
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float* Q = reinterpret_cast<float*>(smem);
  f32x4* QB = reinterpret_cast<f32x4*>(Q + (W / 2) * BO * QLD);  // [W / 2][2 io][64 lanes]
#pragma unroll
  for (int h = W / 2; h >= 2; h /= 2) {
    if (wave >= h && wave < 2 * h) {
      f32x4* dst = reinterpret_cast<f32x4*>(Q + (wave - h) * BO * QLD);
#pragma unroll
      for (int j = 0; j < TAPS; ++j)
#pragma unroll
        for (int io = 0; io < 2; ++io)
#pragma unroll
          for (int ic = 0; ic < 2; ++ic) dst[((j * 2 + io) * 2 + ic) * 64 + lane] = acc[j][io][ic];
      if (do_bias) {
        QB[((wave - h) * 2 + 0) * 64 + lane] = accb[0];
        QB[((wave - h) * 2 + 1) * 64 + lane] = accb[1];
      }
    }
    __syncthreads();
    if (wave < h) {
      const f32x4* src = reinterpret_cast<const f32x4*>(Q + wave * BO * QLD);
#pragma unroll
      for (int j = 0; j < TAPS; ++j)
#pragma unroll
        for (int io = 0; io < 2; ++io)
#pragma unroll
          for (int ic = 0; ic < 2; ++ic) acc[j][io][ic] += src[((j * 2 + io) * 2 + ic) * 64 + lane];
      if (do_bias) {
        accb[0] += QB[(wave * 2 + 0) * 64 + lane];
        accb[1] += QB[(wave * 2 + 1) * 64 + lane];
      }
    }
    __syncthreads();
  }
  if (wave < 2) {
    float* dst = Q + wave * BO * QLD;
#pragma unroll
    for (int j = 0; j < TAPS; ++j)
#pragma unroll
      for (int io = 0; io < 2; ++io)
#pragma unroll
        for (int ic = 0; ic < 2; ++ic)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dst[(io * 16 + 4 * g + r) * QLD + (ic * 16 + r16) * TAPS + j] = acc[j][io][ic][r];
    if (do_bias && r16 == 0) {
#pragma unroll
      for (int io = 0; io < 2; ++io)
#pragma unroll
        for (int r = 0; r < 4; ++r) QB[(wave * 2 + io) * 64 + 4 * g + r][0] = accb[io][r];
    }
  }
  __syncthreads();
  {
    constexpr int V = BC * TAPS / 4;  // f32x4 per output row of the tile
    const int64_t Kp = (int64_t)a.Cin * TAPS;
    const int ncol = (a.Cin - c0 < BC ? a.Cin - c0 : BC) * TAPS;  // valid floats per row
    for (int e = tid; e < BO * V; e += NT) {
      const int o = e / V, v4 = e - o * V;
      if (o0 + o >= a.Cout || 4 * v4 >= ncol) continue;
      const f32x4 s = ld4(Q + o * QLD + 4 * v4) + ld4(Q + BO * QLD + o * QLD + 4 * v4);
      float* d = a.dw + (int64_t)(o0 + o) * Kp + (int64_t)c0 * TAPS + 4 * v4;
      st4(d, ld4(d) + s);
    }
    if (do_bias && tid < BO && o0 + tid < a.Cout) {
      const int io = tid >> 4, gg = (tid & 15) >> 2, r = tid & 3;
      const float b = QB[(0 * 2 + io) * 64 + 4 * gg + r][0] + QB[(1 * 2 + io) * 64 + 4 * gg + r][0];
      a.db[o0 + tid] += b;
    }
  }
}

template <int TAPS>
static bool band_try(const WgradPlan& p, const WgradBand& a, hipStream_t st) {
  if (p.taps != TAPS) return false;
  conv_wgrad_band<TAPS, 2, 2, 4><<<p.grid, 256, 0, st>>>(a);
  return true;
}

int launch_wgrad_band(const WgradPlan& p, const WgradCall& c, hipStream_t st) {
  const WgradBand a{(const u16*)c.dy, c.ldy, (const u16*)c.x, c.ldx, c.dw, c.db, c.rows, c.seq_len,
                    (int)c.c_in, (int)c.c_out, c.pad, p.tiles_o, p.tiles_k, c.lens};
  const bool ok = band_try<9>(p, a, st) || band_try<5>(p, a, st) || band_try<3>(p, a, st);
  return ok ? FS2_OK : no_instance("conv_wgrad_band");
}

}  // namespace fs2
