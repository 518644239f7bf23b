// The stage fs2_f0_yin (pitch.hip) and fs2_f0_pyin (pyin.hip) share: the cumulative-mean-
// normalised difference function d' of the PT_FPB frames a block owns, left in LDS, and the
// descent-and-parabola refinement of a lag.  The block and LDS layout are described at the top of
// pitch.hip; every fp32 operation here is the one numpy does in float32 (no contraction).
#pragma once
#include <math.h>

#include "common.hpp"

#pragma clang fp contract(off)

namespace fs2 {

constexpr int PT_W = 512, PT_FPB = 8, PT_WAVES = 4, PT_FPW = PT_FPB / PT_WAVES, PT_JB = 8;
constexpr int PT_TAU_CAP = 512;
constexpr int PT_DLEN = PT_TAU_CAP + 8;  // d(0 .. tau_max) of one frame

__host__ __device__ inline int pt_span_floats(int hop, int tl) {
  return (PT_FPB - 1) * hop + PT_W + 64 * tl + PT_JB;
}
// floats of region A: the span, later one PT_DLEN slice per frame
__host__ __device__ inline int pt_region_a(int hop, int tl) {
  const int span_n = pt_span_floats(hop, tl);
  const int a_n = span_n > PT_FPB * PT_DLEN ? span_n : PT_FPB * PT_DLEN;
  return (a_n + 3) & ~3;
}
inline size_t pt_lds_bytes(int hop, int tl) {
  return sizeof(float) * (size_t)(pt_region_a(hop, tl) + PT_FPB * PT_DLEN);
}
// lags per lane: the smallest odd TL with 64 TL >= tau_max (lanes TL dwords apart fall into
// different LDS banks)
inline int pt_lags_per_lane(int tmax) {
  int tl = (tmax + 63) / 64;
  return tl + 1 - (tl & 1);
}

// Stages the span of frames fr0 .. fr0 + PT_FPB - 1 of `row` (zeros outside [0, len)) and leaves
// d'(0 .. tmax) of block frame jf at the returned pointer + jf * PT_DLEN.  Ends on a
// __syncthreads; region A (smem .. smem + pt_region_a) is dead afterwards.
template <int TL>
FS2_DEV float* pt_dprime(float* smem, const float* row, int len, int fr0, int hop, int tmax) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // region A: the span, later the running sums of the block's frames; region D: d, then d'
  const int span_n = pt_span_floats(hop, TL);
  float* span = smem;
  float* dall = smem + pt_region_a(hop, TL);
  {
    const int p0 = fr0 * hop - (PT_W + tmax) / 2;
    for (int i = tid; i < span_n; i += 64 * PT_WAVES) {
      const int p = p0 + i;
      span[i] = p >= 0 && p < len ? row[p] : 0.f;
    }
  }
  __syncthreads();

#pragma unroll
  for (int q = 0; q < PT_FPW; ++q) {
    const int jf = wave * PT_FPW + q;  // frame within the block
    const float* seg = span + jf * hop;
    const float* mine = seg + TL * lane + 1;
    float acc[TL];
#pragma unroll
    for (int r = 0; r < TL; ++r) acc[r] = 0.f;
    for (int j0 = 0; j0 < PT_W; j0 += PT_JB) {
      float sj[PT_JB], win[TL + PT_JB - 1];
#pragma unroll
      for (int jj = 0; jj < PT_JB; ++jj) sj[jj] = seg[j0 + jj];
#pragma unroll
      for (int k = 0; k < TL + PT_JB - 1; ++k) win[k] = mine[j0 + k];
#pragma unroll
      for (int jj = 0; jj < PT_JB; ++jj)
#pragma unroll
        for (int r = 0; r < TL; ++r) {
          const float df = sj[jj] - win[jj + r];
          const float sq = df * df;
          acc[r] = acc[r] + sq;
        }
    }
    float* d = dall + jf * PT_DLEN;
#pragma unroll
    for (int r = 0; r < TL; ++r) {
      const int tau = TL * lane + 1 + r;
      if (tau <= tmax) d[tau] = acc[r];
    }
  }
  __syncthreads();  // the span is dead from here on

  float* csall = smem;
  if (lane < PT_FPW) {  // the running sum, sequential as the definition has it
    const float* d = dall + (wave * PT_FPW + lane) * PT_DLEN;
    float* cs = csall + (wave * PT_FPW + lane) * PT_DLEN;
    float run = 0.f;
    for (int tau = 1; tau <= tmax; ++tau) {
      run = run + d[tau];
      cs[tau] = run;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PT_FPW; ++q) {
    float* d = dall + (wave * PT_FPW + q) * PT_DLEN;
    const float* cs = csall + (wave * PT_FPW + q) * PT_DLEN;
    for (int tau = 1 + lane; tau <= tmax; tau += 64) {
      const float c = cs[tau];
      d[tau] = c != 0.f ? (d[tau] * (float)tau) / c : 1.f;
    }
    if (lane == 0) d[0] = 1.f;
  }
  __syncthreads();
  return dall;
}

// From the lag `tau` (1 <= tau <= tmax): down while d'(tau + 1) < d'(tau), then the parabola
// through d'(tau - 1 .. tau + 1).  Returns sr / (tau + offset); `tau` is left at the minimum.
FS2_DEV float pt_refine(const float* d, int& tau, int tmax, float sr) {
  while (tau + 1 <= tmax && d[tau + 1] < d[tau]) ++tau;
  float off = 0.f;
  if (tau < tmax) {
    const float ya = d[tau - 1], yb = d[tau], yc = d[tau + 1];
    const float den = (ya - 2.f * yb) + yc;
    if (den > 0.f) {
      off = (0.5f * (ya - yc)) / den;
      off = off < -1.f ? -1.f : off > 1.f ? 1.f : off;
    }
  }
  return sr / ((float)tau + off);
}

// the live length of row b (lens nullable = S, clamped into [0, S])
FS2_DEV int pt_row_len(const int64_t* lens, int64_t b, int64_t S) {
  int64_t len64 = lens ? lens[b] : S;
  len64 = len64 < 0 ? 0 : len64 > S ? S : len64;
  return (int)len64;
}

}  // namespace fs2
