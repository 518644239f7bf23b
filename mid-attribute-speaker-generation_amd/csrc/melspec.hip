// The mel front end (preprocessor/preprocessor.py:330-336, common/layers.py:101-123 over
// common/stft.py): waveform -> |STFT| (n_fft = win = 1024, centred, reflect padded) -> mel
// filterbank -> log(clamp(., 1e-5)), and the frame energy ||mag||_2, in one launch over a ragged
// batch.  fp32 throughout (but the final log, see log_clamp), precise sqrtf, twiddles from a
// host-built fp64 table.
//
// A block of 4 waves owns STFT_FPB = 8 consecutive frames of one utterance and takes them through
// the forward transform of fft.hpp, which has the layout and its reasons.  Magnitudes go to LDS in
// bin order; lane m sums filter m over its bin range in ascending order; the energy is the lane's
// 8 squares in q order, then the fixed wave reduction.  The per-lane window and twiddle values
// and filter ranges do not depend on the frame and stay in registers; the filterbank's weights
// are staged in LDS beside the span when they fit.  A frame's arithmetic depends on its samples
// only, never on its place in the batch: results are bitwise batch invariant.
#include <math.h>

#include "common.hpp"
#include "fft.hpp"

namespace fs2 {

constexpr int MS_MELMAX = 128;
constexpr int MS_WCAP = 2048;  // filterbank weights staged in LDS when they fit (80 Slaney: 727)

struct MelSpec {
  const float* wav;
  const int64_t* lens;
  int64_t S;
  int hop, n_mels, clip, log_mag, n_weights;
  int64_t F_max;
  int chunks;  // blocks per utterance
  const float* window;
  const float* twiddle;  // (1024, 2): cos, -sin of 2 pi k / 1024
  const int32_t* fb_first;
  const int32_t* fb_count;
  const int32_t* fb_off;
  const float* fb_w;
  float* mel;
  float* energy;
  float* mag;
  int64_t* n_frames;
};

// log(clamp(v, 1e-5)).  The logarithm is taken in fp64 and rounded once, so it is the correctly
// rounded fp32 value: the device logf is within one ulp but not always the nearest, and the
// value every silent frame takes, log(1e-5f), is one it misses (-11.512927 for -11.512925),
// which would set silence one ulp apart from the host's float32 log.  80 calls per frame.
FS2_DEV float log_clamp(float v) { return (float)log((double)fmaxf(v, 1e-5f)); }
// the magnitude as stored: plain, or layers.py:120-123's log(clamp(., 1e-5))
FS2_DEV float mag_out(float v, int log_mag) { return log_mag ? log_clamp(v) : v; }

// WLDS: the filterbank's weights are staged in LDS with the span (else read from global memory
// in the filter sums: any dense (n_mels, 513) matrix is served, the usual sparse one faster)
template <bool WLDS>
__global__ __launch_bounds__(64 * STFT_WAVES) void melspec_kernel(MelSpec a) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hop = a.hop, n_mels = a.n_mels;
  const int64_t b = blockIdx.x / a.chunks;
  const int f0 = (int)(blockIdx.x - b * a.chunks) * STFT_FPB;
  const int64_t F_max = a.F_max;
  // a bad length on the device gives wrong values, never a read outside the row
  int64_t len64 = a.lens ? a.lens[b] : a.S;
  len64 = len64 < 1 ? 1 : len64 > a.S ? a.S : len64;
  const int len = (int)len64;
  const int nf = 1 + len / hop;
  if (f0 == 0 && tid == 0) a.n_frames[b] = nf;
  const int fcnt = (int)(F_max - f0 < STFT_FPB ? F_max - f0 : STFT_FPB);  // frames of this block

  float* mel_b = a.mel + b * n_mels * F_max;
  float* en_b = a.energy ? a.energy + b * F_max : nullptr;
  float* mag_b = a.mag ? a.mag + b * STFT_BINS * F_max : nullptr;

  if (f0 >= nf) {  // past the utterance: zeros (block-uniform)
    for (int i = tid; i < n_mels * fcnt; i += 64 * STFT_WAVES)
      mel_b[(int64_t)(i / fcnt) * F_max + f0 + i % fcnt] = 0.f;
    if (en_b && tid < fcnt) en_b[f0 + tid] = 0.f;
    if (mag_b)
      for (int i = tid; i < STFT_BINS * fcnt; i += 64 * STFT_WAVES)
        mag_b[(int64_t)(i / fcnt) * F_max + f0 + i % fcnt] = 0.f;
    return;
  }

  const int span_n = (STFT_FPB - 1) * hop + STFT_NFFT;
  float* span = smem;            // span_n
  float* otile = span + span_n;  // (n_mels + 1, STFT_FPB)
  float* ex_re = otile + (MS_MELMAX + 1) * STFT_FPB + wave * (2 * STFT_EX + STFT_BINS + 3);
  float* ex_im = ex_re + STFT_EX;
  float* mags = ex_im + STFT_EX;  // STFT_BINS
  float* wlds = otile + (MS_MELMAX + 1) * STFT_FPB + STFT_WAVES * (2 * STFT_EX + STFT_BINS + 3);
  if (WLDS)
    for (int i = tid; i < a.n_weights; i += 64 * STFT_WAVES) wlds[i] = a.fb_w[i];

  stage_span(span, a.wav + b * a.S, f0 * hop - STFT_NFFT / 2, span_n, len, tid, a.clip != 0);

  // frame-independent per-lane constants
  float win[16];
  load_window(win, a.window, lane);
  LaneConst lc;
  lane_consts(lc, a.twiddle, lane);
  const int m = lc.m;
  // this lane's filters (lane, lane + 64), their ranges clamped to the bins and the weights
  int fb_lo[2], fb_n[2], fb_o[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    int first = 0, cnt = 0, off = 0;
    if (c < n_mels) first = a.fb_first[c], cnt = a.fb_count[c], off = a.fb_off[c];
    first = first < 0 ? 0 : first > STFT_BINS ? STFT_BINS : first;
    off = off < 0 ? 0 : off > a.n_weights ? a.n_weights : off;
    cnt = cnt < 0 ? 0 : cnt;
    cnt = cnt > STFT_BINS - first ? STFT_BINS - first : cnt;
    cnt = cnt > a.n_weights - off ? a.n_weights - off : cnt;
    fb_lo[h] = first, fb_n[h] = cnt, fb_o[h] = off;
  }
  __syncthreads();

  for (int it = 0; it < STFT_FPB / STFT_WAVES; ++it) {
    const int jf = it * STFT_WAVES + wave;  // frame within the block
    const int f = f0 + jf;
    cpx z[8];
    load_frame(z, span + jf * hop, win, lane);
    fft512(z, ex_re, ex_im, lc.tw1, lc.tw2, lane, lc.hi, lc.lo);
    float esq = 0.f;
    float mg[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const cpx x = real_split(z, lc, lane, q);
      mg[q] = sqrtf(x.re * x.re + x.im * x.im);
      mags[64 * q + m] = mg[q];
      esq = fmaf(mg[q], mg[q], esq);
    }
    float m512 = 0.f;
    if (lane == 0) {
      m512 = fabsf(real_split_512(z));
      mags[512] = m512;
      esq = fmaf(m512, m512, esq);
    }
    const float en = sqrtf(wave_sum(esq));
    const bool live = f < nf;
    if (mag_b && f < F_max) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        mag_b[(int64_t)(64 * q + m) * F_max + f] = live ? mag_out(mg[q], a.log_mag) : 0.f;
      if (lane == 0) mag_b[(int64_t)512 * F_max + f] = live ? mag_out(m512, a.log_mag) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c >= n_mels) continue;
      const float* w = (WLDS ? wlds : a.fb_w) + fb_o[h];
      const float* g = mags + fb_lo[h];
      float acc = 0.f;
      for (int i = 0; i < fb_n[h]; ++i) acc = fmaf(w[i], g[i], acc);
      otile[c * STFT_FPB + jf] = live ? log_clamp(acc) : 0.f;
    }
    if (lane == 0) otile[n_mels * STFT_FPB + jf] = live ? en : 0.f;
    __syncthreads();
  }

  // the block's (n_mels + 1, fcnt) results, frames innermost
  for (int i = tid; i < n_mels * fcnt; i += 64 * STFT_WAVES) {
    const int c = i / fcnt, j = i - c * fcnt;
    mel_b[(int64_t)c * F_max + f0 + j] = otile[c * STFT_FPB + j];
  }
  if (en_b && tid < fcnt) en_b[f0 + tid] = otile[n_mels * STFT_FPB + tid];
}

// ------------------------------------------------------------------ backward (the mel loss)
// The adjoint of the mel output above, two launches as Griffin-Lim's step.  melspec_bwd_frames:
// the same block shape; each live frame is transformed again exactly as melspec_kernel does,
// its filter sums are formed in the same order, and the cotangent goes back through the log
// clamp, the filterbank (bin-major: bin k adds its filters in ascending order, so no two lanes
// ever add to one address), the modulus and the transform.  The transform's adjoint
//   d frame[n] = Re sum_{k=0}^{512} dX[k] e^{+2 pi i k n / 1024}
// is 512 x irfft of dX with bins 0 and 512 doubled, which is griffinlim.hip's inverse split and
// passes without their 1/512.  The windowed frames go to ws (batch, F_max, 1024).
// melspec_bwd_ola: one thread per sample sums what fft.hpp's reflect_index sends to it.
constexpr int MB_HOP_MIN = 128, MB_HOP_MAX = 512;

struct MelBwd {
  const float* wav;
  const int64_t* lens;
  int64_t S;
  int hop, n_mels, n_weights;
  int64_t F_max;
  int chunks;
  const float* window;
  const float* twiddle;
  const int32_t* fb_first;
  const int32_t* fb_count;
  const int32_t* fb_off;
  const float* fb_w;
  const float* d_mel;
  float* ws;
};

constexpr int MB_WAVE_F = 2 * STFT_EX + STFT_BINS + 3 + MS_MELMAX;  // floats of LDS per wave

template <bool WLDS>
__global__ __launch_bounds__(64 * STFT_WAVES) void melspec_bwd_frames(MelBwd a) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hop = a.hop, n_mels = a.n_mels;
  const int64_t b = blockIdx.x / a.chunks;
  const int f0 = (int)(blockIdx.x - b * a.chunks) * STFT_FPB;
  int64_t len64 = a.lens ? a.lens[b] : a.S;
  len64 = len64 < 1 ? 1 : len64 > a.S ? a.S : len64;
  const int len = (int)len64;
  const int nf = 1 + len / hop;
  if (f0 >= nf) return;  // block-uniform: no live frame, nothing is read from ws there
  const int live = nf - f0 < STFT_FPB ? nf - f0 : STFT_FPB;

  const int span_n = (STFT_FPB - 1) * hop + STFT_NFFT;
  float* span = smem;                                          // span_n
  float* dtile = span + span_n;                                // (MS_MELMAX, STFT_FPB) d_mel
  int* tab = reinterpret_cast<int*>(dtile + MS_MELMAX * STFT_FPB);  // first, count, off
  float* wv = reinterpret_cast<float*>(tab + 3 * MS_MELMAX) + wave * MB_WAVE_F;
  float* ex_re = wv;
  float* ex_im = ex_re + STFT_EX;
  float* mags = ex_im + STFT_EX;            // STFT_BINS (+ 3)
  float* dacc = mags + STFT_BINS + 3;       // MS_MELMAX
  float* wlds = reinterpret_cast<float*>(tab + 3 * MS_MELMAX) + STFT_WAVES * MB_WAVE_F;
  if (WLDS)
    for (int i = tid; i < a.n_weights; i += 64 * STFT_WAVES) wlds[i] = a.fb_w[i];
  const float* fw = WLDS ? wlds : a.fb_w;
  // the filter ranges, clamped as melspec_kernel clamps them
  for (int c = tid; c < MS_MELMAX; c += 64 * STFT_WAVES) {
    int first = 0, cnt = 0, off = 0;
    if (c < n_mels) first = a.fb_first[c], cnt = a.fb_count[c], off = a.fb_off[c];
    first = first < 0 ? 0 : first > STFT_BINS ? STFT_BINS : first;
    off = off < 0 ? 0 : off > a.n_weights ? a.n_weights : off;
    cnt = cnt < 0 ? 0 : cnt;
    cnt = cnt > STFT_BINS - first ? STFT_BINS - first : cnt;
    cnt = cnt > a.n_weights - off ? a.n_weights - off : cnt;
    tab[c] = first, tab[MS_MELMAX + c] = cnt, tab[2 * MS_MELMAX + c] = off;
  }
  for (int i = tid; i < n_mels * STFT_FPB; i += 64 * STFT_WAVES) {
    const int c = i / STFT_FPB, j = i - c * STFT_FPB;
    dtile[i] = j < live ? a.d_mel[(b * n_mels + c) * a.F_max + f0 + j] : 0.f;
  }
  stage_span(span, a.wav + b * a.S, f0 * hop - STFT_NFFT / 2, span_n, len, tid, false);

  float win[16], winv[16];
  load_window(win, a.window, lane);
  LaneConst lc;
  lane_consts(lc, a.twiddle, lane);
  const int m = lc.m;
  load_window(winv, a.window, m);  // the adjoint's output sample pairs
  __syncthreads();

  for (int it = 0; it < STFT_FPB / STFT_WAVES; ++it) {
    const int jf = it * STFT_WAVES + wave;  // frame within the block
    cpx z[8], xs[8], xp[8];
    float mg[8];
    load_frame(z, span + jf * hop, win, lane);
    fft512(z, ex_re, ex_im, lc.tw1, lc.tw2, lane, lc.hi, lc.lo);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      xs[q] = real_split(z, lc, lane, q);
      mg[q] = sqrtf(xs[q].re * xs[q].re + xs[q].im * xs[q].im);
      mags[64 * q + m] = mg[q];
    }
    float v512 = 0.f;
    if (lane == 0) {
      v512 = real_split_512(z);
      mags[512] = fabsf(v512);
    }
    __syncthreads();
    // the filter sums of the forward pass, then d/d(sum) of log(max(sum, 1e-5))
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = lane + 64 * h;
      if (c >= n_mels) continue;
      const float* w = fw + tab[2 * MS_MELMAX + c];
      const float* gm = mags + tab[c];
      const int cnt = tab[MS_MELMAX + c];
      float acc = 0.f;
      for (int i = 0; i < cnt; ++i) acc = fmaf(w[i], gm[i], acc);
      dacc[c] = acc > 1e-5f ? dtile[c * STFT_FPB + jf] / acc : 0.f;
    }
    __syncthreads();
    // filterbank adjoint, bin-major: this lane's bins 64 q + m (and 512 on lane 0)
    float dm[8], dm512 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) dm[q] = 0.f;
    for (int c = 0; c < n_mels; ++c) {
      const int first = tab[c], cnt = tab[MS_MELMAX + c];
      const float* w = fw + tab[2 * MS_MELMAX + c];
      const float dv = dacc[c];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rel = 64 * q + m - first;
        if ((unsigned)rel < (unsigned)cnt) dm[q] = fmaf(w[rel], dv, dm[q]);
      }
      if (lane == 0 && (unsigned)(512 - first) < (unsigned)cnt) dm512 = fmaf(w[512 - first], dv, dm512);
    }
    // modulus: dX = dmag X / |X| (0 where |X| = 0)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float sc = dm[q] / mg[q];
      xp[q] = mg[q] == 0.f ? cpx{0.f, 0.f} : cpx{xs[q].re * sc, xs[q].im * sc};
    }
    const float x512 = v512 > 0.f ? dm512 : v512 < 0.f ? -dm512 : 0.f;

    // the inverse split of griffinlim.hip with bins 0 and 512 doubled, conjugated for the passes
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      cpx x = xp[q];
      cpx p = {__shfl(xp[7 - q].re, lc.partner, 64), __shfl(xp[7 - q].im, lc.partner, 64)};
      if (lane == 0) {
        p = xp[(8 - q) & 7];
        if (q == 0) x = {2.f * x.re, 0.f}, p = {2.f * x512, 0.f};
      }
      const float er = 0.5f * (x.re + p.re), ei = 0.5f * (x.im - p.im);
      const float dr = 0.5f * (x.re - p.re), di = 0.5f * (x.im + p.im);
      const float o_re = dr * lc.tws[q].re + di * lc.tws[q].im;
      const float o_im = di * lc.tws[q].re - dr * lc.tws[q].im;
      z[q] = {er - o_im, -(ei + o_re)};
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      ex_re[64 * q + m] = z[q].re;
      ex_im[64 * q + m] = z[q].im;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = {ex_re[64 * j + lane], ex_im[64 * j + lane]};
    __syncthreads();
    fft512(z, ex_re, ex_im, lc.tw1, lc.tw2, lane, lc.hi, lc.lo);
    if (jf < live) {
      float* out = a.ws + (b * a.F_max + f0 + jf) * STFT_NFFT;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        *reinterpret_cast<f32x2*>(out + 2 * (64 * q + m)) =
            f32x2{z[q].re * winv[2 * q], -z[q].im * winv[2 * q + 1]};
    }
    __syncthreads();
  }
}

constexpr int MB_OLA = 1024;  // samples per block

__global__ __launch_bounds__(256) void melspec_bwd_ola(const float* ws, const int64_t* lens,
                                                       int64_t S, int64_t F_max, int hop, int tiles,
                                                       float* d_wav) {
  const int64_t b = blockIdx.x / tiles;
  const int t0 = (int)(blockIdx.x - b * tiles) * MB_OLA;
  int64_t len64 = lens ? lens[b] : S;
  len64 = len64 < 1 ? 1 : len64 > S ? S : len64;
  const int len = (int)len64;
  const int nf = 1 + len / hop;
  const float* ws_b = ws + b * F_max * STFT_NFFT;
  float* out = d_wav + b * S;
  const int half = STFT_NFFT / 2;
  const int pmax = (nf - 1) * hop + half - 1;  // the frames' raw positions span [-half, pmax]
  for (int i = threadIdx.x; i < MB_OLA; i += 256) {
    const int64_t t64 = (int64_t)t0 + i;
    if (t64 >= S) break;
    const int t = (int)t64;
    float acc = 0.f;
    if (t < len) {
      // the raw positions reflect_index maps to t: t, its mirror about 0, and the mirrors of both
      // about len - 1; at t = 0 also everything past the second mirror (the final clamp)
      int cand[4], nc = 0;
      cand[nc++] = t;
      if (t > 0) cand[nc++] = -t;
      if (t < len - 1) {
        const int P = 2 * (len - 1) - t;
        cand[nc++] = P;
        cand[nc++] = -P;
      }
      const int edge = 2 * (len - 1);
      const bool clamp0 = t == 0 && (edge < half || edge < pmax);
      int f_lo = nf, f_hi = -1;
      for (int c = 0; c < nc; ++c) {
        const int p = cand[c];
        if (p < -half || p > pmax) continue;
        const int num = p - (half - 1);  // f hop >= p + half - 1023
        const int lo = num <= 0 ? 0 : (num + hop - 1) / hop;
        int hi = (p + half) / hop;
        hi = hi > nf - 1 ? nf - 1 : hi;
        f_lo = lo < f_lo ? lo : f_lo;
        f_hi = hi > f_hi ? hi : f_hi;
      }
      if (clamp0) f_lo = 0, f_hi = nf - 1;
      for (int f = f_lo; f <= f_hi; ++f) {
        const int base = f * hop - half;
        const float* fr = ws_b + (int64_t)f * STFT_NFFT;
        for (int c = 0; c < nc; ++c) {
          const int n = cand[c] - base;
          if (n >= 0 && n < STFT_NFFT) acc += fr[n];
        }
        if (clamp0)
          for (int n = 0; n < STFT_NFFT; ++n) {
            const int p = base + n;
            if ((p < 0 ? -p : p) > edge) acc += fr[n];
          }
      }
    }
    out[t] = acc;
  }
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_melspec(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                int64_t n_fft, int64_t hop, const float* window, const float* twiddle,
                const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                const float* fb_w, int64_t n_weights, int64_t n_mels, int clip, int log_mag,
                float* mel, float* energy, float* mag, int64_t* n_frames, void* stream) {
  FS2_CHECK_ARG(n_fft == STFT_NFFT, "fs2_melspec: n_fft %lld (only n_fft = win_length = %d is built)",
                (long long)n_fft, STFT_NFFT);
  FS2_CHECK_ARG(hop >= 1 && hop <= STFT_NFFT, "fs2_melspec: hop %lld (1..%d)", (long long)hop,
                STFT_NFFT);
  FS2_CHECK_ARG(n_mels >= 1 && n_mels <= MS_MELMAX, "fs2_melspec: n_mels %lld (1..%d)",
                (long long)n_mels, MS_MELMAX);
  FS2_CHECK_ARG(samples >= 1 && samples < (1ll << 30), "fs2_melspec: samples %lld (1..2^30 - 1)",
                (long long)samples);
  FS2_CHECK_ARG(n_weights >= 0 && n_weights <= (int64_t)MS_MELMAX * STFT_BINS,
                "fs2_melspec: n_weights %lld", (long long)n_weights);
  FS2_CHECK_ARG(batch >= 0, "fs2_melspec: batch %lld", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && window && twiddle && fb_first && fb_count && fb_off && fb_w && mel && n_frames,
                "fs2_melspec: missing operand");
  const int64_t F_max = 1 + samples / hop;
  const int64_t chunks = (F_max + STFT_FPB - 1) / STFT_FPB;
  FS2_CHECK_ARG(batch * chunks < (1ll << 31), "fs2_melspec: batch %lld x %lld frames too large",
                (long long)batch, (long long)F_max);
  MelSpec a{wav, lens, samples, (int)hop, (int)n_mels, clip, log_mag, (int)n_weights, F_max, (int)chunks,
            window, twiddle, fb_first, fb_count, fb_off, fb_w, mel, energy, mag, n_frames};
  const size_t lds = sizeof(float) * ((STFT_FPB - 1) * (size_t)hop + STFT_NFFT +
                                      (MS_MELMAX + 1) * STFT_FPB +
                                      STFT_WAVES * (2 * STFT_EX + STFT_BINS + 3));
  const size_t lds_w = lds + sizeof(float) * (size_t)n_weights;
  const dim3 grid((unsigned)(batch * chunks));
  if (n_weights <= MS_WCAP && lds_w <= 64 * 1024)  // the widest hops leave no room for them
    melspec_kernel<true><<<grid, 64 * STFT_WAVES, lds_w, as_stream(stream)>>>(a);
  else
    melspec_kernel<false><<<grid, 64 * STFT_WAVES, lds, as_stream(stream)>>>(a);
  return launch_status("fs2_melspec");
}

int64_t fs2_melspec_bwd_ws_bytes(int64_t batch, int64_t samples, int64_t hop) {
  if (batch < 1 || samples < 1 || hop < 1) return 0;
  return batch * (1 + samples / hop) * STFT_NFFT * (int64_t)sizeof(float);
}

int fs2_melspec_bwd(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                    int64_t n_fft, int64_t hop, const float* window, const float* twiddle,
                    const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                    const float* fb_w, int64_t n_weights, int64_t n_mels, const float* d_mel,
                    float* d_wav, float* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(n_fft == STFT_NFFT, "fs2_melspec_bwd: n_fft %lld (only n_fft = win_length = %d is built)",
                (long long)n_fft, STFT_NFFT);
  FS2_CHECK_ARG(hop >= MB_HOP_MIN && hop <= MB_HOP_MAX, "fs2_melspec_bwd: hop %lld (%d..%d)",
                (long long)hop, MB_HOP_MIN, MB_HOP_MAX);
  FS2_CHECK_ARG(n_mels >= 1 && n_mels <= MS_MELMAX, "fs2_melspec_bwd: n_mels %lld (1..%d)",
                (long long)n_mels, MS_MELMAX);
  FS2_CHECK_ARG(samples >= 1 && samples < (1ll << 30), "fs2_melspec_bwd: samples %lld (1..2^30 - 1)",
                (long long)samples);
  FS2_CHECK_ARG(n_weights >= 0 && n_weights <= (int64_t)MS_MELMAX * STFT_BINS,
                "fs2_melspec_bwd: n_weights %lld", (long long)n_weights);
  FS2_CHECK_ARG(batch >= 0, "fs2_melspec_bwd: batch %lld", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && window && twiddle && fb_first && fb_count && fb_off && fb_w && d_mel && d_wav && ws,
                "fs2_melspec_bwd: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_melspec_bwd_ws_bytes(batch, samples, hop),
                "fs2_melspec_bwd: the workspace holds the frames' cotangents (%lld bytes)",
                (long long)fs2_melspec_bwd_ws_bytes(batch, samples, hop));
  const int64_t F_max = 1 + samples / hop;
  const int64_t chunks = (F_max + STFT_FPB - 1) / STFT_FPB;
  const int64_t tiles = (samples + MB_OLA - 1) / MB_OLA;
  FS2_CHECK_ARG(batch * chunks < (1ll << 31) && batch * tiles < (1ll << 31) &&
                    batch * F_max < (1ll << 40),
                "fs2_melspec_bwd: batch %lld x %lld frames too large", (long long)batch,
                (long long)F_max);
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  MelBwd a{wav, lens, samples, (int)hop, (int)n_mels, (int)n_weights, F_max, (int)chunks, window,
           twiddle, fb_first, fb_count, fb_off, fb_w, d_mel, ws};
  const size_t lds = sizeof(float) * ((STFT_FPB - 1) * (size_t)hop + STFT_NFFT +
                                      MS_MELMAX * STFT_FPB + 3 * MS_MELMAX +
                                      STFT_WAVES * (size_t)MB_WAVE_F);
  const size_t lds_w = lds + sizeof(float) * (size_t)n_weights;
  const dim3 grid((unsigned)(batch * chunks));
  if (n_weights <= MS_WCAP && lds_w <= 64 * 1024)
    melspec_bwd_frames<true><<<grid, 64 * STFT_WAVES, lds_w, st>>>(a);
  else
    melspec_bwd_frames<false><<<grid, 64 * STFT_WAVES, lds, st>>>(a);
  melspec_bwd_ola<<<dim3((unsigned)(batch * tiles)), 256, 0, st>>>(ws, lens, samples, F_max,
                                                                   (int)hop, (int)tiles, d_wav);
  return launch_status("fs2_melspec_bwd");
}

}  // extern "C"
