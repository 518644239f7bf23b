// Griffin-Lim (common/audio_processing.py:86-102; STFT.inverse, common/stft.py:107-137;
// TacotronSTFT._mel_to_linear, common/layers.py:125-131): the inverse half of melspec.hip's
// transform pair, n_fft = win = 1024, 128 <= hop <= 512, fp32 throughout.
//
// One iteration is two launches.  gl_frames_kernel: a block of 4 waves owns STFT_FPB = 8
// consecutive frames of one row, as melspec_kernel does.  It stages their sample span (fft.hpp's
// index rule, reflection against the row's own L = hop (F - 1)) and the (513, 8) tile of their
// target magnitudes in LDS -- the global reads of the tile run along frames -- then each wave
// takes two frames through
//   the forward transform of fft.hpp (window, 512-point complex FFT, real-input split) -> X[k]
//   X'[k] = mag[k] X[k] / |X[k]|   ((mag[k], 0) where |X[k]| = 0; no atan2 / sincos)
//   inverse split  Z'[k] = E' + i O',  E' = (X'[k] + conj X'[512 - k]) / 2,
//                  O' = W1024^-k (X'[k] - conj X'[512 - k]) / 2   (bins 0 and 512: real parts only)
//   inverse FFT as the same three passes on conj Z' (one LDS transpose from the passes' output
//   order 64 q + 8 t + s back to their input order 64 j + r), conjugated, / 512, times the window
// and writes the windowed inverse frame to the workspace (batch, frames, 1024).  The partner
// bin 512 - k sits in the same fixed partner lane as in the forward split, so both splits are
// lane shuffles.  fs2_istft runs the same kernel with an inverse-only prologue: the tile holds
// mag (cos, sin) phase instead (the one place sincosf is used), no span, no forward transform.
// gl_ola_kernel then streams the waveform: sample t sums its <= ceil(1024 / hop) frames at
// position t + 512 in ascending frame order and divides by the sum of w^2 taken in that order.
// No atomics and no order depends on the batch: results are bitwise batch invariant.
#include <math.h>

#include "common.hpp"
#include "fft.hpp"

namespace fs2 {

constexpr int GL_TS = STFT_FPB + 1;  // tile stride: bin k of frame j at 9 k + j (odd: spreads banks)
constexpr int GL_TILE = STFT_BINS * GL_TS;
constexpr int GL_HOP_MIN = 128, GL_HOP_MAX = 512;
constexpr int GL_MELMAX = 128, GL_MFR = 64;  // fs2_mel_to_linear: frames per block
constexpr int GL_MKP = 8;                    // ... and the blocks (grid y) that share its bins
constexpr int GL_OLA = 1024;                 // samples per block of gl_ola_kernel

struct GlFrames {
  const float* wav_in;  // STEP only
  const float* mag;
  const float* phase;  // inverse only, nullable
  const int64_t* n_frames;
  int64_t frames, S;
  int hop, chunks;  // blocks per row
  const float* window;
  const float* twiddle;  // (1024, 2): cos, -sin of 2 pi k / 1024
  float* ws;
};

FS2_DEV int live_frames(const int64_t* n_frames, int64_t b, int64_t frames) {
  int64_t nf = n_frames ? n_frames[b] : frames;
  nf = nf < 0 ? 0 : nf > frames ? frames : nf;
  return (int)nf;
}

// STEP: one Griffin-Lim pass from wav_in (else: the inverse of (mag, phase) alone)
template <bool STEP>
__global__ __launch_bounds__(64 * STFT_WAVES) void gl_frames_kernel(GlFrames a) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hop = a.hop;
  const int64_t b = blockIdx.x / a.chunks;
  const int f0 = (int)(blockIdx.x - b * a.chunks) * STFT_FPB;
  const int nf = live_frames(a.n_frames, b, a.frames);
  // a row of fewer than two frames has no sample, and no frame past nf is ever summed
  if (nf < 2 || f0 >= nf) return;  // block-uniform
  const int len = hop * (nf - 1);
  const int live = nf - f0 < STFT_FPB ? nf - f0 : STFT_FPB;
  const int span_n = (STFT_FPB - 1) * hop + STFT_NFFT;

  float* tile_a = smem;              // STEP: target magnitudes; else Re X'
  float* tile_b = tile_a + GL_TILE;  // STEP: the sample span; else Im X'
  float* ex_re = tile_b + (STEP ? span_n : GL_TILE) + wave * 2 * STFT_EX;
  float* ex_im = ex_re + STFT_EX;

  {
    const int64_t row = b * STFT_BINS * a.frames + f0;
    for (int i = tid; i < STFT_BINS * STFT_FPB; i += 64 * STFT_WAVES) {
      const int k = i >> 3, j = i & 7;
      float re = 0.f, im = 0.f;
      if (j < live) {  // the frames past nf hold anything: not read
        const int64_t at = row + (int64_t)k * a.frames + j;
        const float mg = a.mag[at];
        if (STEP) {
          re = mg;
        } else {
          float sn = 0.f, cs = 1.f;
          if (a.phase) sincosf(a.phase[at], &sn, &cs);
          re = mg * cs, im = mg * sn;
        }
      }
      tile_a[k * GL_TS + j] = re;
      if (!STEP) tile_b[k * GL_TS + j] = im;
    }
  }
  if (STEP) stage_span(tile_b, a.wav_in + b * a.S, f0 * hop - STFT_NFFT / 2, span_n, len, tid, false);

  // frame-independent per-lane constants
  float win[16], winv[16];
  LaneConst lc;
  lane_consts(lc, a.twiddle, lane);
  const int m = lc.m;
  if (STEP) load_window(win, a.window, lane);
  load_window(winv, a.window, m);  // the inverse's output sample pairs
#pragma unroll
  for (int j = 0; j < 16; ++j) winv[j] *= 1.f / 512.f;  // exact
  __syncthreads();

  for (int it = 0; it < STFT_FPB / STFT_WAVES; ++it) {
    const int jf = it * STFT_WAVES + wave;  // frame within the block
    cpx z[8], xp[8];
    float x512;  // X'[512] (lane 0)
    if (STEP) {
      load_frame(z, tile_b + jf * hop, win, lane);
      fft512(z, ex_re, ex_im, lc.tw1, lc.tw2, lane, lc.hi, lc.lo);
      // the target magnitude on X's direction
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const cpx x = real_split(z, lc, lane, q);
        const float tg = tile_a[(64 * q + m) * GL_TS + jf];
        const float mg = sqrtf(x.re * x.re + x.im * x.im);
        const float sc = tg / mg;
        xp[q] = mg == 0.f ? cpx{tg, 0.f} : cpx{x.re * sc, x.im * sc};
      }
      // bin 512 is real: its direction is its sign
      const float v512 = real_split_512(z), tg512 = tile_a[512 * GL_TS + jf];
      x512 = v512 < 0.f ? -tg512 : tg512;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        xp[q] = {tile_a[(64 * q + m) * GL_TS + jf], tile_b[(64 * q + m) * GL_TS + jf]};
      x512 = tile_a[512 * GL_TS + jf];
    }

    // inverse split, conjugated for the forward passes
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      cpx x = xp[q];
      cpx p = {__shfl(xp[7 - q].re, lc.partner, 64), __shfl(xp[7 - q].im, lc.partner, 64)};
      if (lane == 0) {
        p = xp[(8 - q) & 7];
        if (q == 0) x.im = 0.f, p = {x512, 0.f};  // bins 0 and 512: their real parts only
      }
      const float er = 0.5f * (x.re + p.re), ei = 0.5f * (x.im - p.im);
      const float dr = 0.5f * (x.re - p.re), di = 0.5f * (x.im + p.im);
      const float o_re = dr * lc.tws[q].re + di * lc.tws[q].im;  // (dr + i di) conj W1024^k
      const float o_im = di * lc.tws[q].re - dr * lc.tws[q].im;
      z[q] = {er - o_im, -(ei + o_re)};  // conj(E' + i O')
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
      float* out = a.ws + (b * a.frames + f0 + jf) * STFT_NFFT;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        *reinterpret_cast<f32x2*>(out + 2 * (64 * q + m)) =
            f32x2{z[q].re * winv[2 * q], -z[q].im * winv[2 * q + 1]};
    }
    __syncthreads();
  }
}

struct GlOla {
  const float* ws;
  const int64_t* n_frames;
  int64_t frames, S;
  int hop, tiles;  // blocks per row
  const float* window;
  float* wav;
};

__global__ __launch_bounds__(256) void gl_ola_kernel(GlOla a) {
  __shared__ float w2[STFT_NFFT];
  for (int i = threadIdx.x; i < STFT_NFFT; i += 256) {
    const float w = a.window[i];
    w2[i] = w * w;
  }
  __syncthreads();
  const int64_t b = blockIdx.x / a.tiles;
  const int t0 = (int)(blockIdx.x - b * a.tiles) * GL_OLA;
  const int hop = a.hop;
  const int nf = live_frames(a.n_frames, b, a.frames);
  const int len = nf < 2 ? 0 : hop * (nf - 1);
  const float* ws_b = a.ws + b * a.frames * STFT_NFFT;
  float* out = a.wav + b * a.S;
  for (int i = threadIdx.x; i < GL_OLA; i += 256) {
    const int t = t0 + i;
    if (t >= a.S) break;
    float v = 0.f;
    if (t < len) {
      const int p = t + STFT_NFFT / 2;
      const int f_lo = p < STFT_NFFT ? 0 : (p - (STFT_NFFT - 1) + hop - 1) / hop;
      const int f_hi = p / hop < nf - 1 ? p / hop : nf - 1;
      float acc = 0.f, den = 0.f;
      for (int f = f_lo; f <= f_hi; ++f) {
        const int o = p - f * hop;  // 0 .. 1023
        acc += ws_b[(int64_t)f * STFT_NFFT + o];
        den += w2[o];
      }
      v = acc / den;
    }
    out[t] = v;
  }
}

__global__ __launch_bounds__(256) void mel_to_linear_kernel(const float* mel, const int64_t* n_frames,
                                                            int n_mels, int64_t frames, int tiles,
                                                            const float* inv_basis, float* mag) {
  extern __shared__ float e[];  // (n_mels, GL_MFR): exp(mel) of the block's frames
  const int tid = threadIdx.x, fj = tid & 63, kq = tid >> 6;
  const int64_t b = blockIdx.x / tiles;
  const int64_t f0 = (int64_t)(blockIdx.x - b * tiles) * GL_MFR;
  const int nf = live_frames(n_frames, b, frames);
  const float* mel_b = mel + b * n_mels * frames;
  for (int i = tid; i < n_mels * GL_MFR; i += 256) {
    const int c = i >> 6;
    const int64_t f = f0 + (i & 63);
    e[i] = f < nf ? expf(mel_b[c * frames + f]) : 0.f;
  }
  __syncthreads();
  const int64_t f = f0 + fj;
  if (f >= frames) return;
  float* mag_b = mag + b * STFT_BINS * frames + f;
  // k is wave-uniform: the basis row is broadcast
  for (int k = 4 * blockIdx.y + kq; k < STFT_BINS; k += 4 * GL_MKP) {
    const float* pk = inv_basis + k * n_mels;
    float acc = 0.f;
    for (int c = 0; c < n_mels; ++c) acc = fmaf(pk[c], e[c * GL_MFR + fj], acc);
    mag_b[(int64_t)k * frames] = f < nf ? fmaxf(acc, 1e-10f) : 0.f;
  }
}

// the argument checks fs2_istft and fs2_griffin_lim_step share
static int gl_check(const char* fn, int64_t batch, int64_t frames, int64_t n_fft, int64_t hop) {
  FS2_CHECK_ARG(n_fft == STFT_NFFT, "%s: n_fft %lld (only n_fft = win_length = %d is built)", fn,
                (long long)n_fft, STFT_NFFT);
  FS2_CHECK_ARG(hop >= GL_HOP_MIN && hop <= GL_HOP_MAX, "%s: hop %lld (%d..%d)", fn, (long long)hop,
                GL_HOP_MIN, GL_HOP_MAX);
  FS2_CHECK_ARG(batch >= 0, "%s: batch %lld", fn, (long long)batch);
  FS2_CHECK_ARG(frames >= 1 && hop * (frames - 1) < (1ll << 30), "%s: frames %lld (1.., samples < 2^30)",
                fn, (long long)frames);
  const int64_t chunks = (frames + STFT_FPB - 1) / STFT_FPB;
  FS2_CHECK_ARG(batch * chunks < (1ll << 31) && batch * frames < (1ll << 40),
                "%s: batch %lld x %lld frames too large", fn, (long long)batch, (long long)frames);
  return FS2_OK;
}

static int gl_launch(const char* fn, bool step, const float* wav_in, const float* mag,
                     const float* phase, const int64_t* n_frames, int64_t batch, int64_t frames,
                     int64_t hop, const float* window, const float* twiddle, float* wav, float* ws,
                     int64_t ws_bytes, hipStream_t st) {
  const int64_t S = hop * (frames - 1);
  FS2_CHECK_ARG(mag && window && twiddle && (wav || S == 0) && (!step || wav_in || S == 0),
                "%s: missing operand", fn);
  FS2_CHECK_ARG(ws && ws_bytes >= fs2_griffin_lim_ws_bytes(batch, frames),
                "%s: the workspace holds the inverse frames (%lld bytes)", fn,
                (long long)fs2_griffin_lim_ws_bytes(batch, frames));
  if (S == 0) return FS2_OK;  // one frame: no sample
  poison(ws, ws_bytes, st);
  const int64_t chunks = (frames + STFT_FPB - 1) / STFT_FPB;
  GlFrames a{wav_in, mag, phase, n_frames, frames, S, (int)hop, (int)chunks, window, twiddle, ws};
  const dim3 grid((unsigned)(batch * chunks));
  const size_t ex = sizeof(float) * STFT_WAVES * 2 * STFT_EX;
  if (step)
    gl_frames_kernel<true><<<grid, 64 * STFT_WAVES,
                             sizeof(float) * (GL_TILE + (STFT_FPB - 1) * (size_t)hop + STFT_NFFT) + ex,
                             st>>>(a);
  else
    gl_frames_kernel<false><<<grid, 64 * STFT_WAVES, sizeof(float) * 2 * GL_TILE + ex, st>>>(a);
  const int64_t tiles = (S + GL_OLA - 1) / GL_OLA;
  GlOla o{ws, n_frames, frames, S, (int)hop, (int)tiles, window, wav};
  gl_ola_kernel<<<dim3((unsigned)(batch * tiles)), 256, 0, st>>>(o);
  return launch_status(fn);
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_mel_to_linear(const float* mel, const int64_t* n_frames, int64_t batch, int64_t n_mels,
                      int64_t frames, const float* inv_basis, float* mag, void* stream) {
  FS2_CHECK_ARG(n_mels >= 1 && n_mels <= GL_MELMAX, "fs2_mel_to_linear: n_mels %lld (1..%d)",
                (long long)n_mels, GL_MELMAX);
  FS2_CHECK_ARG(batch >= 0 && frames >= 1, "fs2_mel_to_linear: batch %lld, frames %lld",
                (long long)batch, (long long)frames);
  const int64_t tiles = (frames + GL_MFR - 1) / GL_MFR;
  FS2_CHECK_ARG(batch * tiles < (1ll << 31) && batch * frames < (1ll << 40),
                "fs2_mel_to_linear: batch %lld x %lld frames too large", (long long)batch,
                (long long)frames);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(mel && inv_basis && mag, "fs2_mel_to_linear: missing operand");
  mel_to_linear_kernel<<<dim3((unsigned)(batch * tiles), GL_MKP), 256, sizeof(float) * n_mels * GL_MFR,
                         as_stream(stream)>>>(mel, n_frames, (int)n_mels, frames, (int)tiles,
                                              inv_basis, mag);
  return launch_status("fs2_mel_to_linear");
}

int64_t fs2_griffin_lim_ws_bytes(int64_t batch, int64_t frames) {
  if (batch < 1 || frames < 1) return 0;
  return batch * frames * STFT_NFFT * (int64_t)sizeof(float);
}

int fs2_istft(const float* mag, const float* phase, const int64_t* n_frames, int64_t batch,
              int64_t frames, int64_t n_fft, int64_t hop, const float* window,
              const float* twiddle, float* wav, float* ws, int64_t ws_bytes, void* stream) {
  if (const int rc = gl_check("fs2_istft", batch, frames, n_fft, hop)) return rc;
  if (batch == 0) return FS2_OK;
  return gl_launch("fs2_istft", false, nullptr, mag, phase, n_frames, batch, frames, hop, window,
                   twiddle, wav, ws, ws_bytes, as_stream(stream));
}

int fs2_griffin_lim_step(const float* wav_in, const float* mag, const int64_t* n_frames,
                         int64_t batch, int64_t frames, int64_t n_fft, int64_t hop,
                         const float* window, const float* twiddle, float* wav_out, float* ws,
                         int64_t ws_bytes, void* stream) {
  if (const int rc = gl_check("fs2_griffin_lim_step", batch, frames, n_fft, hop)) return rc;
  if (batch == 0) return FS2_OK;
  const int64_t n = batch * hop * (frames - 1);
  FS2_CHECK_ARG(!wav_in || !wav_out || wav_out + n <= wav_in || wav_in + n <= wav_out,
                "fs2_griffin_lim_step: wav_out overlaps wav_in");
  return gl_launch("fs2_griffin_lim_step", true, wav_in, mag, nullptr, n_frames, batch, frames, hop,
                   window, twiddle, wav_out, ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
