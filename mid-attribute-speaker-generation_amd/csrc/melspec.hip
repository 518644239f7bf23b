// The mel front end (preprocessor/preprocessor.py:330-336, common/layers.py:101-123 over
// common/stft.py): waveform -> |STFT| (n_fft = win = 1024, centred, reflect padded) -> mel
// filterbank -> log(clamp(., 1e-5)), and the frame energy ||mag||_2, in one launch over a ragged
// batch.  fp32 throughout (but the final log, see log_clamp), precise sqrtf, twiddles from a
// host-built fp64 table.
//
// A block of 4 waves owns MS_FPB = 8 consecutive frames of one utterance: it stages their sample
// span ((MS_FPB - 1) hop + 1024 samples, reflection resolved against the utterance's own length,
// every index clamped into [0, len - 1]) into LDS once, then each wave transforms two frames.
// A frame is the 512-point complex FFT of z[n] = x[2n] w[2n] + i x[2n + 1] w[2n + 1] followed by
// the real-input split.  512 = 8^3: three radix-8 passes in registers, 8 complex values per
// lane, decimation in frequency.  With n = 64 j + r, r = 8 a + b and k = 64 q + 8 t + s:
//   pass 1  lane r          DFT8 over j -> s, times W512^(r s)    -> LDS at 72 s + r
//   pass 2  lane (s, b)     DFT8 over a -> t, times W64^(b t)     -> LDS at 72 s + 9 t + b
//   pass 3  lane (s, t)     DFT8 over b -> q: Z[64 q + 8 t + s]
// ds_read_b32 / ds_write_b32 bank per 32-lane half and modulo 32: 72 s + r is contiguous in r;
// its readers 8 s + b (+ 8 a) cover 32 banks; 72 s + 9 t + b = 8 (s + t) + t + b (mod 32) covers
// them for writers (s, b) and readers (s, t) alike.  The split pairs Z[k] with Z[512 - k], which
// sits in one fixed partner lane (register 7 - q), so it is a lane shuffle, not an LDS round
// trip; lane 0 (k = 64 q) pairs with itself and owns bins 0 and 512.  Magnitudes go to LDS in
// bin order; lane m sums filter m over its bin range in ascending order; the energy is the lane's
// 8 squares in q order, then the fixed wave reduction.  The per-lane window and twiddle values
// and filter ranges do not depend on the frame and stay in registers; the filterbank's weights
// are staged in LDS beside the span when they fit.  A frame's arithmetic depends on its samples
// only, never on its place in the batch: results are bitwise batch invariant.
#include <math.h>

#include "common.hpp"
#include "fft.hpp"  // cpx, cmul, dft8

namespace fs2 {

constexpr int MS_NFFT = 1024, MS_BINS = 513, MS_FPB = 8, MS_WAVES = 4, MS_EX = 576;
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
__global__ __launch_bounds__(64 * MS_WAVES) void melspec_kernel(MelSpec a) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hop = a.hop, n_mels = a.n_mels;
  const int64_t b = blockIdx.x / a.chunks;
  const int f0 = (int)(blockIdx.x - b * a.chunks) * MS_FPB;
  const int64_t F_max = a.F_max;
  // a bad length on the device gives wrong values, never a read outside the row
  int64_t len64 = a.lens ? a.lens[b] : a.S;
  len64 = len64 < 1 ? 1 : len64 > a.S ? a.S : len64;
  const int len = (int)len64;
  const int nf = 1 + len / hop;
  if (f0 == 0 && tid == 0) a.n_frames[b] = nf;
  const int fcnt = (int)(F_max - f0 < MS_FPB ? F_max - f0 : MS_FPB);  // frames of this block

  float* mel_b = a.mel + b * n_mels * F_max;
  float* en_b = a.energy ? a.energy + b * F_max : nullptr;
  float* mag_b = a.mag ? a.mag + b * MS_BINS * F_max : nullptr;

  if (f0 >= nf) {  // past the utterance: zeros (block-uniform)
    for (int i = tid; i < n_mels * fcnt; i += 64 * MS_WAVES)
      mel_b[(int64_t)(i / fcnt) * F_max + f0 + i % fcnt] = 0.f;
    if (en_b && tid < fcnt) en_b[f0 + tid] = 0.f;
    if (mag_b)
      for (int i = tid; i < MS_BINS * fcnt; i += 64 * MS_WAVES)
        mag_b[(int64_t)(i / fcnt) * F_max + f0 + i % fcnt] = 0.f;
    return;
  }

  const int span_n = (MS_FPB - 1) * hop + MS_NFFT;
  float* span = smem;                                  // span_n
  float* otile = span + span_n;                        // (n_mels + 1, MS_FPB)
  float* ex_re = otile + (MS_MELMAX + 1) * MS_FPB + wave * (2 * MS_EX + MS_BINS + 3);
  float* ex_im = ex_re + MS_EX;
  float* mags = ex_im + MS_EX;                         // MS_BINS
  float* wlds = otile + (MS_MELMAX + 1) * MS_FPB + MS_WAVES * (2 * MS_EX + MS_BINS + 3);
  if (WLDS)
    for (int i = tid; i < a.n_weights; i += 64 * MS_WAVES) wlds[i] = a.fb_w[i];

  {
    const float* row = a.wav + b * a.S;
    const int p0 = f0 * hop - MS_NFFT / 2;
    for (int i = tid; i < span_n; i += 64 * MS_WAVES) {
      int p = p0 + i;
      p = p < 0 ? -p : p;
      p = p > len - 1 ? 2 * (len - 1) - p : p;
      p = p < 0 ? 0 : p > len - 1 ? len - 1 : p;
      float v = row[p];
      if (a.clip) v = fminf(fmaxf(v, -1.f), 1.f);
      span[i] = v;
    }
  }

  // frame-independent per-lane constants
  float win[16];
  cpx tw1[8], tw2[8], tws[8];
  const int hi = lane >> 3, lo = lane & 7;  // (s, b) in pass 2, (s, t) in pass 3
  const int m = 8 * lo + hi;                // low bin index of this lane after pass 3
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    win[2 * j] = a.window[128 * j + 2 * lane];
    win[2 * j + 1] = a.window[128 * j + 2 * lane + 1];
    const int i1 = 2 * lane * j, i2 = 16 * lo * j, i3 = 64 * j + m;
    tw1[j] = {a.twiddle[2 * i1], a.twiddle[2 * i1 + 1]};
    tw2[j] = {a.twiddle[2 * i2], a.twiddle[2 * i2 + 1]};
    tws[j] = {a.twiddle[2 * i3], a.twiddle[2 * i3 + 1]};
  }
  const int mp = (64 - m) & 63;
  const int partner = ((mp & 7) << 3) | (mp >> 3);
  // this lane's filters (lane, lane + 64), their ranges clamped to the bins and the weights
  int fb_lo[2], fb_n[2], fb_o[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    int first = 0, cnt = 0, off = 0;
    if (c < n_mels) first = a.fb_first[c], cnt = a.fb_count[c], off = a.fb_off[c];
    first = first < 0 ? 0 : first > MS_BINS ? MS_BINS : first;
    off = off < 0 ? 0 : off > a.n_weights ? a.n_weights : off;
    cnt = cnt < 0 ? 0 : cnt;
    cnt = cnt > MS_BINS - first ? MS_BINS - first : cnt;
    cnt = cnt > a.n_weights - off ? a.n_weights - off : cnt;
    fb_lo[h] = first, fb_n[h] = cnt, fb_o[h] = off;
  }
  __syncthreads();

  for (int it = 0; it < MS_FPB / MS_WAVES; ++it) {
    const int jf = it * MS_WAVES + wave;  // frame within the block
    const int f = f0 + jf;
    const float* fr = span + jf * hop;
    cpx z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n2 = 128 * j + 2 * lane;
      z[j] = {fr[n2] * win[2 * j], fr[n2 + 1] * win[2 * j + 1]};
    }
    dft8(z);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const cpx y = s ? cmul(z[s], tw1[s]) : z[s];
      ex_re[72 * s + lane] = y.re;
      ex_im[72 * s + lane] = y.im;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = {ex_re[72 * hi + 8 * q + lo], ex_im[72 * hi + 8 * q + lo]};
    __syncthreads();
    dft8(z);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const cpx y = t ? cmul(z[t], tw2[t]) : z[t];
      ex_re[72 * hi + 9 * t + lo] = y.re;
      ex_im[72 * hi + 9 * t + lo] = y.im;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = {ex_re[72 * hi + 9 * lo + q], ex_im[72 * hi + 9 * lo + q]};
    dft8(z);
    // real-input split: X[k] = E + W1024^k O, E = (Z[k] + conj Z[512 - k]) / 2,
    // O = -i (Z[k] - conj Z[512 - k]) / 2
    float esq = 0.f;
    float mg[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      cpx p = {__shfl(z[7 - q].re, partner, 64), __shfl(z[7 - q].im, partner, 64)};
      if (lane == 0) p = z[(8 - q) & 7];
      const float er = 0.5f * (z[q].re + p.re), ei = 0.5f * (z[q].im - p.im);
      const float orr = 0.5f * (z[q].im + p.im), oi = -0.5f * (z[q].re - p.re);
      const float xr = er + (tws[q].re * orr - tws[q].im * oi);
      const float xi = ei + (tws[q].re * oi + tws[q].im * orr);
      mg[q] = sqrtf(xr * xr + xi * xi);
      mags[64 * q + m] = mg[q];
      esq = fmaf(mg[q], mg[q], esq);
    }
    float m512 = 0.f;
    if (lane == 0) {  // bin 512 = Re Z[0] - Im Z[0]
      m512 = fabsf(z[0].re - z[0].im);
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
      otile[c * MS_FPB + jf] = live ? log_clamp(acc) : 0.f;
    }
    if (lane == 0) otile[n_mels * MS_FPB + jf] = live ? en : 0.f;
    __syncthreads();
  }

  // the block's (n_mels + 1, fcnt) results, frames innermost
  for (int i = tid; i < n_mels * fcnt; i += 64 * MS_WAVES) {
    const int c = i / fcnt, j = i - c * fcnt;
    mel_b[(int64_t)c * F_max + f0 + j] = otile[c * MS_FPB + j];
  }
  if (en_b && tid < fcnt) en_b[f0 + tid] = otile[n_mels * MS_FPB + tid];
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_melspec(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                int64_t n_fft, int64_t hop, const float* window, const float* twiddle,
                const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                const float* fb_w, int64_t n_weights, int64_t n_mels, int clip, int log_mag,
                float* mel, float* energy, float* mag, int64_t* n_frames, void* stream) {
  FS2_CHECK_ARG(n_fft == MS_NFFT, "fs2_melspec: n_fft %lld (only n_fft = win_length = %d is built)",
                (long long)n_fft, MS_NFFT);
  FS2_CHECK_ARG(hop >= 1 && hop <= MS_NFFT, "fs2_melspec: hop %lld (1..%d)", (long long)hop, MS_NFFT);
  FS2_CHECK_ARG(n_mels >= 1 && n_mels <= MS_MELMAX, "fs2_melspec: n_mels %lld (1..%d)",
                (long long)n_mels, MS_MELMAX);
  FS2_CHECK_ARG(samples >= 1 && samples < (1ll << 30), "fs2_melspec: samples %lld (1..2^30 - 1)",
                (long long)samples);
  FS2_CHECK_ARG(n_weights >= 0 && n_weights <= (int64_t)MS_MELMAX * MS_BINS,
                "fs2_melspec: n_weights %lld", (long long)n_weights);
  FS2_CHECK_ARG(batch >= 0, "fs2_melspec: batch %lld", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && window && twiddle && fb_first && fb_count && fb_off && fb_w && mel && n_frames,
                "fs2_melspec: missing operand");
  const int64_t F_max = 1 + samples / hop;
  const int64_t chunks = (F_max + MS_FPB - 1) / MS_FPB;
  FS2_CHECK_ARG(batch * chunks < (1ll << 31), "fs2_melspec: batch %lld x %lld frames too large",
                (long long)batch, (long long)F_max);
  MelSpec a{wav, lens, samples, (int)hop, (int)n_mels, clip, log_mag, (int)n_weights, F_max, (int)chunks,
            window, twiddle, fb_first, fb_count, fb_off, fb_w, mel, energy, mag, n_frames};
  const size_t lds = sizeof(float) * ((MS_FPB - 1) * (size_t)hop + MS_NFFT + (MS_MELMAX + 1) * MS_FPB +
                                      MS_WAVES * (2 * MS_EX + MS_BINS + 3));
  const size_t lds_w = lds + sizeof(float) * (size_t)n_weights;
  const dim3 grid((unsigned)(batch * chunks));
  if (n_weights <= MS_WCAP && lds_w <= 64 * 1024)  // the widest hops leave no room for them
    melspec_kernel<true><<<grid, 64 * MS_WAVES, lds_w, as_stream(stream)>>>(a);
  else
    melspec_kernel<false><<<grid, 64 * MS_WAVES, lds, as_stream(stream)>>>(a);
  return launch_status("fs2_melspec");
}

}  // extern "C"
