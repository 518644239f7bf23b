// Pitch and the rest of Preprocessor.process_utterance / build_from_path
// (preprocessor/preprocessor.py:169-328) after the mel front end: the F0 contour (YIN, where the
// reference calls pyworld's DIO + StoneMask: a different estimator, no parity claimed), the
// interpolation over unvoiced frames, the phoneme-level means, the outlier filter with the
// running moments, and the normalisation with the running extrema.
//
// fs2_f0_yin (the d' stage and the lag refinement live in yin_core.hpp, which pyin.hip shares).
// A block of 4 waves owns PT_FPB = 8 consecutive frames of one utterance and stages
// their sample span ((PT_FPB - 1) hop + 512 + 64 TL + 8 floats, zeros outside [0, len)) into LDS
// once; each wave then owns two of the frames.  A lane keeps TL consecutive lags
// tau = TL lane + 1 + r in registers (TL the smallest odd number with 64 TL >= tau_max: 5 for
// the 310 lags of 22 050 Hz / 71 Hz).  Per 8 samples j it reads the 8 values s[j] (one address
// for the whole wave: a broadcast) and the TL + 7 values s[j + tau] its lags need (lane stride TL
// dwords, TL odd: no bank conflict), and makes 8 TL subtract / multiply / add triples: 20 LDS
// reads for 120 VALU instructions at TL = 5.  Each d(tau) is one lane's fp32 sum over j
// ascending of rounded squares -- floating-point contraction is off in this file, so the
// arithmetic is the one numpy does in float32 and a frame's value depends on its samples only.
// The running sum over tau is one lane's sequential chain per frame (the two frames of a wave
// side by side in lanes 0 and 1, its buffers over the span that is dead by then); d' and the
// search for the first lag under the threshold are lane-parallel again, the descent and the
// parabola wave-uniform.
//
// The four small kernels work on (batch, frames) rows of at most 15 360 frames (one row in
// LDS): one wave per utterance for the fill and for the phoneme means (whose in-place order
// is sequential by definition), one block for the moments (rows merge in order), one block per
// row for the normalisation.
#include <float.h>
#include <math.h>

#include "yin_core.hpp"  // the d' stage and the lag refinement, shared with pyin.hip

#pragma clang fp contract(off)

namespace fs2 {

constexpr int PT_ROW_CAP = 15360;  // frames of a row the small kernels hold in LDS

struct F0Yin {
  const float* wav;
  const int64_t* lens;
  int64_t S;
  int hop;
  int64_t F_max;
  int chunks;  // blocks per utterance
  int tmin, tmax;
  float sr, lo, hi, thr;
  float* f0;
  float* dip;
  int64_t* n_frames;
};

template <int TL>
__global__ __launch_bounds__(64 * PT_WAVES) void f0_yin_kernel(F0Yin a) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hop = a.hop, tmin = a.tmin, tmax = a.tmax;
  const int64_t b = blockIdx.x / a.chunks;
  const int fr0 = (int)(blockIdx.x - b * a.chunks) * PT_FPB;
  const int64_t F_max = a.F_max;
  const int len = pt_row_len(a.lens, b, a.S);
  const int nf = 1 + len / hop;
  if (fr0 == 0 && tid == 0) a.n_frames[b] = nf;
  const int fcnt = (int)(F_max - fr0 < PT_FPB ? F_max - fr0 : PT_FPB);
  float* f0_b = a.f0 + b * F_max;
  float* dip_b = a.dip + b * F_max;
  if (fr0 >= nf) {  // past the utterance: zeros (block-uniform)
    if (tid < fcnt) f0_b[fr0 + tid] = 0.f, dip_b[fr0 + tid] = 0.f;
    return;
  }
  const float* dall = pt_dprime<TL>(smem, a.wav + b * a.S, len, fr0, hop, tmax);

#pragma unroll
  for (int q = 0; q < PT_FPW; ++q) {
    const int jf = wave * PT_FPW + q, fr = fr0 + jf;
    const float* d = dall + jf * PT_DLEN;
    int first = -1;
    for (int base = tmin; base <= tmax && first < 0; base += 64) {
      const int tau = base + lane;
      const bool hit = tau <= tmax && d[tau] < a.thr;
      const unsigned long long mask = __ballot(hit);
      if (mask) first = base + __ffsll((long long)mask) - 1;
    }
    float f = 0.f, dp;
    if (first < 0) {
      float m = INFINITY;
      for (int tau = tmin + lane; tau <= tmax; tau += 64) m = fminf(m, d[tau]);
      dp = -wave_max(-m);
    } else {
      int tau = first;
      f = pt_refine(d, tau, tmax, a.sr);
      dp = d[tau];
      if (f < a.lo || f > a.hi) f = 0.f;
    }
    if (lane == 0 && fr < F_max) {
      const bool live = fr < nf;
      f0_b[fr] = live ? f : 0.f;
      dip_b[fr] = live ? dp : 0.f;
    }
  }
}

// ------------------------------------------------------------------ after the contour
FS2_DEV int row_count(const int64_t* n, int64_t b, int64_t cols) {
  int64_t v = n ? n[b] : cols;
  return (int)(v < 0 ? 0 : v > cols ? cols : v);
}

FS2_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int PT_NONE = 0x7fffffff;

__global__ __launch_bounds__(64) void pitch_fill_kernel(float* x, const int64_t* n, int64_t frames,
                                                        int32_t* ok) {
  extern __shared__ int prev[];  // the last non-zero frame at or before i, or -1
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  float* row = x + b * frames;
  const int nn = row_count(n, b, frames);
  int carry = -1, count = 0;
  for (int base = 0; base < nn; base += 64) {
    const int i = base + lane;
    const bool live = i < nn;
    const float v = live ? row[i] : 0.f;
    const bool nz = live && v != 0.f;
    int p = nz ? i : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(p, o, 64);
      if (lane >= o) p = p > t ? p : t;
    }
    p = p > carry ? p : carry;
    if (live) prev[i] = p;
    carry = __shfl(p, 63, 64);
    count += __popcll(__ballot(nz));
  }
  if (lane == 0) ok[b] = count > 1 ? 1 : 0;
  if (count <= 1) return;
  // downwards: only zero frames are written and only non-zero ones are read again
  int next = PT_NONE;
  for (int base = ((nn - 1) / 64) * 64; base >= 0; base -= 64) {
    const int i = base + lane;
    const bool live = i < nn;
    const float v = live ? row[i] : 0.f;
    const bool nz = live && v != 0.f;
    int q = nz ? i : PT_NONE;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_down(q, o, 64);
      if (lane + o < 64) q = q < t ? q : t;
    }
    q = q < next ? q : next;
    if (live && !nz) {
      const int p = prev[i];
      float out;
      if (p < 0) {
        out = row[q];
      } else if (q == PT_NONE) {
        out = row[p];
      } else {  // scipy's interp1d: slope (x_new - x_lo) + y_lo
        const double ylo = row[p], yhi = row[q];
        const double slope = (yhi - ylo) / (double)(q - p);
        out = (float)(slope * (double)(i - p) + ylo);
      }
      row[i] = out;
    }
    next = __shfl(q, 0, 64);
  }
}

__global__ __launch_bounds__(64) void segment_mean_kernel(float* x, const int64_t* n,
                                                          const int64_t* dur, int64_t frames,
                                                          int64_t phones, float* out) {
  extern __shared__ float work[];  // the row as the reference's in-place loop sees it
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  float* row = x + b * frames;
  const int nn = row_count(n, b, frames);
  for (int i = lane; i < (int)frames; i += 64) work[i] = row[i];
  __syncthreads();
  int64_t pos = 0;
  for (int64_t i = 0; i < phones; ++i) {
    int64_t d = dur[b * phones + i];
    d = d < 0 ? 0 : d > (1ll << 31) ? (1ll << 31) : d;
    float m = 0.f;
    if (d > 0) {
      const int64_t lo = pos < nn ? pos : nn, hi = pos + d < nn ? pos + d : nn;
      double s = 0.0;
      for (int64_t j = lo + lane; j < hi; j += 64) s += (double)work[j];
      s = wave_sum_f64(s);
      m = hi > lo ? (float)(s / (double)(hi - lo)) : NAN;
    }
    __syncthreads();
    if (lane == 0) {
      if (i < frames) work[i] = m;
      out[b * phones + i] = m;
    }
    __syncthreads();
    pos += d;
  }
  const int wrote = (int)(phones < frames ? phones : frames);
  for (int i = lane; i < wrote; i += 64) row[i] = work[i];
}

constexpr int PT_RED = 256;  // threads of the reducing blocks

// sum over the block, the waves' partials added in wave order; every thread gets it
FS2_DEV double block_sum_f64(double v, double* sh) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < PT_RED / 64; ++w) s += sh[w];
  return s;
}

// numpy's linear percentile of a sorted row (lib/function_base.py: _lerp)
FS2_DEV double percentile_sorted(const float* row, int nn, double q) {
  const double vi = (double)(nn - 1) * q;
  const double fl = floor(vi);
  int lo = (int)fl, hi = lo + 1;
  lo = lo < 0 ? 0 : lo > nn - 1 ? nn - 1 : lo;
  hi = hi < 0 ? 0 : hi > nn - 1 ? nn - 1 : hi;
  const double g = vi - fl, va = row[lo], vb = row[hi], diff = vb - va;
  return g >= 0.5 ? vb - diff * (1.0 - g) : va + diff * g;
}

__global__ __launch_bounds__(PT_RED) void outlier_moments_kernel(const float* sorted,
                                                                 const int64_t* n, int64_t batch,
                                                                 int64_t cols, double* state) {
  __shared__ double sh[PT_RED / 64];
  const int tid = threadIdx.x;
  for (int64_t b = 0; b < batch; ++b) {
    const int nn = row_count(n, b, cols);
    if (nn == 0) continue;  // block-uniform
    const float* row = sorted + b * cols;
    const double p25 = percentile_sorted(row, nn, 0.25), p75 = percentile_sorted(row, nn, 0.75);
    const double lower = p25 - 1.5 * (p75 - p25), upper = p75 + 1.5 * (p75 - p25);
    double c = 0.0, s = 0.0;
    for (int i = tid; i < nn; i += PT_RED) {
      const double v = row[i];
      if (v > lower && v < upper) c += 1.0, s += v;
    }
    const double cnt = block_sum_f64(c, sh);
    if (cnt == 0.0) continue;  // block-uniform: every thread holds the same sum
    const double mean = block_sum_f64(s, sh) / cnt;
    double m2 = 0.0;
    for (int i = tid; i < nn; i += PT_RED) {
      const double v = row[i];
      if (v > lower && v < upper) m2 += (v - mean) * (v - mean);
    }
    m2 = block_sum_f64(m2, sh);
    if (tid == 0) {  // Chan, Golub & LeVeque's pairwise update
      const double na = state[0];
      if (na == 0.0) {
        state[0] = cnt, state[1] = mean, state[2] = m2;
      } else {
        const double tot = na + cnt, delta = mean - state[1];
        state[1] = state[1] + delta * (cnt / tot);
        state[2] = state[2] + m2 + delta * delta * (na * cnt / tot);
        state[0] = tot;
      }
    }
  }
}

FS2_DEV void atomic_min_f64(double* p, double v) {
  unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
  unsigned long long old = *q;
  while (v < __longlong_as_double((long long)old)) {
    const unsigned long long seen = atomicCAS(q, old, (unsigned long long)__double_as_longlong(v));
    if (seen == old) break;
    old = seen;
  }
}
FS2_DEV void atomic_max_f64(double* p, double v) {
  unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
  unsigned long long old = *q;
  while (v > __longlong_as_double((long long)old)) {
    const unsigned long long seen = atomicCAS(q, old, (unsigned long long)__double_as_longlong(v));
    if (seen == old) break;
    old = seen;
  }
}

__global__ __launch_bounds__(PT_RED) void normalize_minmax_kernel(float* x, const int64_t* n,
                                                                  int64_t cols, double mean,
                                                                  double std, double* minmax) {
  __shared__ double sh[2][PT_RED / 64];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  float* row = x + b * cols;
  const int nn = row_count(n, b, cols);
  double lo = DBL_MAX, hi = -DBL_MAX;  // extrema are exact in any order
  for (int i = tid; i < nn; i += PT_RED) {
    const float v = (float)(((double)row[i] - mean) / std);
    row[i] = v;
    lo = fmin(lo, (double)v), hi = fmax(hi, (double)v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if ((tid & 63) == 0) sh[0][tid >> 6] = lo, sh[1][tid >> 6] = hi;
  __syncthreads();
  if (tid == 0 && nn > 0) {
#pragma unroll
    for (int w = 1; w < PT_RED / 64; ++w) lo = fmin(lo, sh[0][w]), hi = fmax(hi, sh[1][w]);
    atomic_min_f64(minmax, lo);
    atomic_max_f64(minmax + 1, hi);
  }
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_f0_yin(const float* wav, const int64_t* lens, int64_t batch, int64_t samples, int64_t hop,
               double sr, double f0_floor, double f0_ceil, double threshold, float* f0, float* dip,
               int64_t* n_frames, void* stream) {
  FS2_CHECK_ARG(hop >= 1 && hop <= 1024, "fs2_f0_yin: hop %lld (1..1024)", (long long)hop);
  FS2_CHECK_ARG(samples >= 1 && samples < (1ll << 30), "fs2_f0_yin: samples %lld (1..2^30 - 1)",
                (long long)samples);
  FS2_CHECK_ARG(batch >= 0, "fs2_f0_yin: batch %lld", (long long)batch);
  FS2_CHECK_ARG(sr > 0 && f0_floor > 0 && f0_ceil >= f0_floor && threshold > 0,
                "fs2_f0_yin: sr %g, f0 range %g..%g, threshold %g", sr, f0_floor, f0_ceil, threshold);
  const double tmax_d = floor(sr / f0_floor), tmin_d = ceil(sr / f0_ceil);
  FS2_CHECK_ARG(tmax_d <= PT_TAU_CAP, "fs2_f0_yin: sr / f0_floor = %g lags (at most %d are built)",
                tmax_d, PT_TAU_CAP);
  FS2_CHECK_ARG(tmin_d >= 1 && tmin_d <= tmax_d, "fs2_f0_yin: lags %g..%g", tmin_d, tmax_d);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && f0 && dip && n_frames, "fs2_f0_yin: missing operand");
  const int64_t F_max = 1 + samples / hop;
  const int64_t chunks = (F_max + PT_FPB - 1) / PT_FPB;
  FS2_CHECK_ARG(batch * chunks < (1ll << 31), "fs2_f0_yin: batch %lld x %lld frames too large",
                (long long)batch, (long long)F_max);
  const int tmax = (int)tmax_d, tmin = (int)tmin_d;
  const int tl = pt_lags_per_lane(tmax);
  F0Yin a{wav, lens, samples, (int)hop, F_max, (int)chunks, tmin, tmax, (float)sr, (float)f0_floor,
          (float)f0_ceil, (float)threshold, f0, dip, n_frames};
  const size_t lds = pt_lds_bytes((int)hop, tl);
  const dim3 grid((unsigned)(batch * chunks));
  hipStream_t st = as_stream(stream);
  switch (tl) {
    case 1: f0_yin_kernel<1><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    case 3: f0_yin_kernel<3><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    case 5: f0_yin_kernel<5><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    case 7: f0_yin_kernel<7><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    default: f0_yin_kernel<9><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
  }
  return launch_status("fs2_f0_yin");
}

int fs2_pitch_fill(float* x, const int64_t* n, int64_t batch, int64_t frames, int32_t* ok,
                   void* stream) {
  FS2_CHECK_ARG(batch >= 0 && batch < (1ll << 31), "fs2_pitch_fill: batch %lld", (long long)batch);
  FS2_CHECK_ARG(frames >= 1 && frames <= PT_ROW_CAP, "fs2_pitch_fill: frames %lld (1..%d)",
                (long long)frames, PT_ROW_CAP);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(x && ok, "fs2_pitch_fill: missing operand");
  pitch_fill_kernel<<<dim3((unsigned)batch), 64, sizeof(int) * (size_t)frames, as_stream(stream)>>>(
      x, n, frames, ok);
  return launch_status("fs2_pitch_fill");
}

int fs2_segment_mean(float* x, const int64_t* n, const int64_t* durations, int64_t batch,
                     int64_t frames, int64_t phones, float* out, void* stream) {
  FS2_CHECK_ARG(batch >= 0 && batch < (1ll << 31), "fs2_segment_mean: batch %lld", (long long)batch);
  FS2_CHECK_ARG(frames >= 1 && frames <= PT_ROW_CAP, "fs2_segment_mean: frames %lld (1..%d)",
                (long long)frames, PT_ROW_CAP);
  FS2_CHECK_ARG(phones >= 0 && phones < (1ll << 31), "fs2_segment_mean: phones %lld", (long long)phones);
  if (batch == 0 || phones == 0) return FS2_OK;
  FS2_CHECK_ARG(x && durations && out, "fs2_segment_mean: missing operand");
  segment_mean_kernel<<<dim3((unsigned)batch), 64, sizeof(float) * (size_t)frames,
                        as_stream(stream)>>>(x, n, durations, frames, phones, out);
  return launch_status("fs2_segment_mean");
}

int fs2_outlier_moments(const float* sorted, const int64_t* n, int64_t batch, int64_t cols,
                        double* state, void* stream) {
  FS2_CHECK_ARG(batch >= 0, "fs2_outlier_moments: batch %lld", (long long)batch);
  FS2_CHECK_ARG(cols >= 1 && cols < (1ll << 31), "fs2_outlier_moments: cols %lld", (long long)cols);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(sorted && state, "fs2_outlier_moments: missing operand");
  outlier_moments_kernel<<<1, PT_RED, 0, as_stream(stream)>>>(sorted, n, batch, cols, state);
  return launch_status("fs2_outlier_moments");
}

int fs2_normalize_minmax(float* x, const int64_t* n, int64_t batch, int64_t cols, double mean,
                         double std, double* minmax, void* stream) {
  FS2_CHECK_ARG(batch >= 0 && batch < (1ll << 31), "fs2_normalize_minmax: batch %lld",
                (long long)batch);
  FS2_CHECK_ARG(cols >= 1 && cols < (1ll << 31), "fs2_normalize_minmax: cols %lld", (long long)cols);
  FS2_CHECK_ARG(std != 0, "fs2_normalize_minmax: std 0");
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(x && minmax, "fs2_normalize_minmax: missing operand");
  normalize_minmax_kernel<<<dim3((unsigned)batch), PT_RED, 0, as_stream(stream)>>>(x, n, cols, mean,
                                                                                    std, minmax);
  return launch_status("fs2_normalize_minmax");
}

}  // extern "C"
