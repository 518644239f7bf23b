#include "conv_nt.hpp"
#include "conv_plan.hpp"

namespace fs2 {

// ---------------------------------------------------------------- tap-register halo Conv1d
// conv_gemm_tapreg: the halo Conv1d (C_in % 64 == 0, taps > 1, undilated, every row tile inside
// one utterance) with each A fragment of a channel block read from LDS ONCE for all taps.
//
// A wave owns a band of 16 S rows x WC columns.  Its output fragment i (i < S) holds the band
// rows i + S m (m = 0..15), so tap j of fragment i needs the input rows i + j + S m: halo
// fragment F[i + j], where F[f] = rows f + S m of the band's halo (f < S + taps - 1).  The
// S + taps - 1 halo fragments of a channel block are each read from LDS once and held in a
// rolling register window (tap j uses F[j .. j + S - 1]: one new fragment per tap and k-half);
// per 64-channel block a 64 x 32 wave tile (S = 4, k = 9) reads 24 halo + 36 weight fragments
// for 144 MFMAs (0.42 per MFMA), the halo kernel's 128 x 32 wave tile 0.63.  Same MFMAs per output in the same (channel block, tap, k-half) order as the halo
// kernels: bitwise equal where both compute.
// LDS halo image: halo row h sits at position (h mod S) * RS + h / S, so every F[f] reads 16
// consecutive positions (chunk swizzle c ^ (h / S & 7): conflict-free ds_read_b128); the LDS-DMA
// source row of each position is fixed per block (zero line outside the utterance / length).
// Weight tiles (tap j, channel block cb) stream through a WS-slot ring, one barrier per tap;
// channel block cb + 1's halo is staged at tap 0 of block cb (two halo slots).
// Weight and halo registers rotate by k-half: after a tap's half-0 MFMAs the next tap's half-0
// weights and halo fragment (at the last tap the next block's first S halo fragments) are read
// under the half-1 MFMAs, and vice versa -- one register set of each.
// A wave whose band lies past the utterance's length stages its share but issues no MFMAs
// (those rows are masked downstream, as in conv_gemm_halo).
template <int BM, int BN, int WGM, int WGN, int S, int TAPS, int WS, int MINB>
__global__ __launch_bounds__(WGM * WGN * 64, MINB) void conv_gemm_tapreg(GldsArgs a) {
  constexpr int NW = WGM * WGN, BK = 64;
  constexpr int WR = 16 * S, WC = BN / WGN, NI = WC / 16;
  static_assert(BM == WGM * WR && WC % 16 == 0 && WGM % 2 == 0, "tile");
  constexpr int NF = S + TAPS - 1;
  constexpr int HR = BM + TAPS - 1, RS = (HR + S - 1) / S, HP = (S * RS + 7) / 8;
  constexpr int QMAX = (HP + NW - 1) / NW, BWP = BN / 8 / NW;
  static_assert(BN % (8 * NW) == 0, "weight pieces");
  constexpr int D = WS == 2 ? 2 : WS - 1;  // tile s + D is issued at step s
  static_assert(D <= 3 && TAPS >= D && (D - 2) * BWP + QMAX <= 8, "vmcnt bookkeeping");
  constexpr int A_E = HP * 8 * BK, B_E = BN * BK;
  constexpr int EPI_E = (BM / 2) * (BN + 4) * 2;
  constexpr int SMEM_E = 2 * A_E + WS * B_E > EPI_E ? 2 * A_E + WS * B_E : EPI_E;
  __shared__ __attribute__((aligned(1024))) u16 smem[SMEM_E];
  u16* As = smem;
  u16* Bs = smem + 2 * A_E;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int g = lane >> 4, r16 = lane & 15, lrow = lane >> 3;
  // block -> tile: XCD-contiguous runs, n fastest within a group (as conv_gemm_halo)
  const int nwg = a.tiles_m * a.tiles_n;
  const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int gfull = a.tiles_m * a.group;
  const int ng = wg / gfull, rem = wg - ng * gfull;
  const int gsz = a.tiles_n - ng * a.group < a.group ? a.tiles_n - ng * a.group : a.group;
  const int tm = m_interleave(rem / gsz, a.tiles_m, a.lens != nullptr);
  const int tn = ng * a.group + (rem - (rem / gsz) * gsz);
  const int64_t m0 = (int64_t)tm * BM;
  const int n0 = tn * BN;
  const bool skip = a.lens && rows_all_padding(a.lens, a.T, m0, m0 + BM < a.M ? m0 + BM : a.M);
  const int64_t u0 = (m0 / a.T) * a.T;
  const int64_t ulen = a.lens ? (a.lens[m0 / a.T] < a.T ? a.lens[m0 / a.T] : a.T) : a.T;
  const int64_t u1 = u0 + ulen < a.M ? u0 + ulen : a.M;
  const bool band_pad = m0 + wm * WR >= u1;

  // halo piece pc = wave + NW q: positions 8 pc + lrow, position P = res * RS + qq holds halo
  // row h = qq * S + res (global row m0 - pad + h)
  const auto x_rs = buf_rsrc(a.x + (m0 - a.pad) * a.ldx, (int64_t)HR * a.ldx * 2);
  const auto w_rs = buf_rsrc(a.w + (int64_t)n0 * a.K, (int64_t)BN * a.K * 2);
  uint32_t h_vo[QMAX];
  int qa = 0;
#pragma unroll
  for (int q = 0; q < QMAX; ++q) {
    const int pc = wave + NW * q, P = pc * 8 + lrow;
    const int res = P / RS, qq = P - res * RS, h = qq * S + res;
    const int64_t gr = m0 - a.pad + h;
    const int lc = (lane & 7) ^ (qq & 7);
    h_vo[q] = (pc < HP && res < S && h < HR && gr >= u0 && gr < u1)
                  ? (uint32_t)((h * a.ldx + lc * 8) * 2) : kOOB;
    qa += pc < HP ? 1 : 0;
  }
  uint32_t b_vo[BWP];
#pragma unroll
  for (int i = 0; i < BWP; ++i) {
    const int R = (wave * BWP + i) * 8 + lrow;
    b_vo[i] = n0 + R < a.N ? (uint32_t)((R * a.K + ((lane & 7) ^ (R & 7)) * 8) * 2) : kOOB;
  }
  auto issue_a = [&](int cb, int slot) {
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
      const int pc = wave + NW * q;
      if (pc < HP) glds16_buf(x_rs, As + slot * A_E + pc * 8 * BK, h_vo[q], (uint32_t)(cb * BK * 2));
    }
  };
  auto issue_b = [&](int t) {  // weight tile t = (channel block t / TAPS, tap t % TAPS)
    const int cb = t / TAPS, j = t - cb * TAPS;
    const uint32_t k0 = (uint32_t)((j * a.Cin + cb * BK) * 2);
    u16* dst = Bs + (t % WS) * B_E + wave * BWP * 8 * BK;
#pragma unroll
    for (int i = 0; i < BWP; ++i) glds16_buf(w_rs, dst + i * 8 * BK, b_vo[i], k0);
  };

  f32x4 acc[S][NI];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 F[NF][2], Bw[NI][2];
  // F[f] of this lane: position (f % S) * RS + wm * 16 + f / S + r16, swizzle key = its offset
  // within the residue class mod 8 = (r16 + f / S) & 7 -- one of (NF - 1) / S + 1 lane patterns
  // per k-half (the rest of the address is a compile-time offset)
  constexpr int NQ = (NF - 1) / S + 1;
  const u16* fa[NQ][2];
#pragma unroll
  for (int d = 0; d < NQ; ++d)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      fa[d][ks] = As + (r16 + wm * 16 + d) * BK + (((ks * 4 + g) ^ ((r16 + d) & 7)) * 8);
  const int b_row = wn * WC + r16;
  const u16* fb[2] = {Bs + b_row * BK + ((g ^ (b_row & 7)) * 8),
                      Bs + b_row * BK + (((4 + g) ^ (b_row & 7)) * 8)};
  auto rd_f = [&](int cb, int f, int ks) {
    F[f][ks] = *reinterpret_cast<const bf16x8*>(fa[f / S][ks] + (cb & 1) * A_E + (f % S) * RS * BK);
  };
  auto rd_b = [&](int t, int ks) {
    const int so = (t % WS) * B_E;
#pragma unroll
    for (int jj = 0; jj < NI; ++jj) Bw[jj][ks] = *reinterpret_cast<const bf16x8*>(fb[ks] + so + jj * 16 * BK);
  };
  auto mfma_half = [&](auto jc, int ks) {
    constexpr int J = decltype(jc)::value;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int jj = 0; jj < NI; ++jj)
        acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(F[i + J][ks], Bw[jj][ks], acc[i][jj], 0, 0, 0);
  };

  if (!skip) {
    const int ncb = a.Cin / BK, Stot = ncb * TAPS;
    // prologue: halo 0, tiles 0 .. D-1
    issue_a(0, 0);
    issue_b(0);
    int pend = 0;
#pragma unroll
    for (int d = 1; d < D; ++d)
      if (d < Stot) {
        issue_b(d);
        pend += BWP;
      }
    vm_wait_n(pend);  // halo 0 and tile 0 landed
    __builtin_amdgcn_s_barrier();
    auto run = [&](auto cc) {
      constexpr bool C = decltype(cc)::value;
      if constexpr (C) {
#pragma unroll
        for (int f = 0; f < S; ++f) {
          rd_f(0, f, 0);
          rd_f(0, f, 1);
        }
        rd_b(0, 0);
        rd_b(0, 1);
      }
      for (int cb = 0; cb < ncb; ++cb) {
        const bool more = cb + 1 < ncb;
        auto step = [&](auto jc) {
          constexpr int J = decltype(jc)::value;
          const int s = cb * TAPS + J;
          // tile s + 1 landed (this wave's pieces); later DMA may stay in flight: tiles
          // s + 2 .. s + D - 1 and the halo issued at tap 0 when that came after tile s + 1
          int n = 0;
          if (D == 3 && s + 2 < Stot) n += BWP;
          if (J >= 1 && J <= D - 1 && more) n += qa;
          vm_wait_n(n);
          if constexpr (WS == 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
          if (s + D < Stot) issue_b(s + D);
          // block cb + 1's halo into the slot block cb - 1 used (its last reads, at tap
          // TAPS - 2, were consumed by the MFMAs of tap TAPS - 1: done before this barrier)
          if (J == 0 && more) issue_a(cb + 1, (cb + 1) & 1);
          if constexpr (C) {
            // tap J uses F[J .. J + S - 1]; F[J] is dead after it, F[J + S] is new at J + 1
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              mfma_half(jc, ks);
              __builtin_amdgcn_sched_barrier(0);
              if (s + 1 < Stot) rd_b(s + 1, ks);
              if constexpr (J + 1 < TAPS) {
                rd_f(cb, J + S, ks);
              } else if (more) {
#pragma unroll
                for (int f = 0; f < S; ++f) rd_f(cb + 1, f, ks);
              }
              __builtin_amdgcn_sched_barrier(0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        };
        static_for<TAPS>(step);
      }
    };
    if (band_pad) run(std::false_type{});
    else run(std::true_type{});
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  nt_epilogue<BM, BN, false, NW, WGN, WGM, S, true>(a, acc, smem, m0, n0, skip, tid, wm, wn, g, r16);
}

template <int BN, int TAPS, int MINB>
static bool tapreg_try(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  if (p.bn != BN || p.taps != TAPS) return false;
  conv_gemm_tapreg<128, BN, 2, 2, 4, TAPS, 2, MINB><<<p.grid, 256, 0, st>>>(a);
  return true;
}

// 4-wave 128 x 128 tiles at 2 blocks per CU, 128 x 64 tiles at 3
int launch_conv_tapreg(const ConvPlan& p, const GldsArgs& a, hipStream_t st) {
  const bool ok = tapreg_try<128, 9, 2>(p, a, st) || tapreg_try<128, 5, 2>(p, a, st) ||
                  tapreg_try<64, 9, 3>(p, a, st) || tapreg_try<64, 5, 3>(p, a, st);
  return ok ? FS2_OK : no_instance("conv_gemm_tapreg");
}

}  // namespace fs2
