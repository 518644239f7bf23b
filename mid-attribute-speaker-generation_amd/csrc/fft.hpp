// The 1024-point real STFT as a wave computes it: the one forward transform of the mel front end
// (melspec.hip) and of Griffin-Lim (griffinlim.hip, which runs its inverse through the same
// passes); the silence split (vad.hip) takes the index rule alone.
//
// A block of STFT_WAVES = 4 waves owns STFT_FPB = 8 consecutive frames of one row: it stages their
// sample span ((STFT_FPB - 1) hop + 1024 samples, reflection resolved against the row's own
// length, every index clamped into [0, len - 1]) into LDS once, then each wave transforms two
// frames.  A frame is the 512-point complex FFT of z[n] = x[2n] w[2n] + i x[2n + 1] w[2n + 1]
// followed by the real-input split.  512 = 8^3: three radix-8 passes in registers, 8 complex
// values per lane, decimation in frequency.  With n = 64 j + r, r = 8 a + b and k = 64 q + 8 t + s:
//   pass 1  lane r          DFT8 over j -> s, times W512^(r s)    -> LDS at 72 s + r
//   pass 2  lane (s, b)     DFT8 over a -> t, times W64^(b t)     -> LDS at 72 s + 9 t + b
//   pass 3  lane (s, t)     DFT8 over b -> q: Z[64 q + 8 t + s]
// ds_read_b32 / ds_write_b32 bank per 32-lane half and modulo 32: 72 s + r is contiguous in r;
// its readers 8 s + b (+ 8 a) cover 32 banks; 72 s + 9 t + b = 8 (s + t) + t + b (mod 32) covers
// them for writers (s, b) and readers (s, t) alike.  The split pairs Z[k] with Z[512 - k], which
// sits in one fixed partner lane (register 7 - q), so it is a lane shuffle, not an LDS round
// trip; lane 0 (k = 64 q) pairs with itself and owns bins 0 and 512.  The per-lane window and
// twiddle values do not depend on the frame and stay in registers.
#pragma once
#include "common.hpp"

namespace fs2 {

// n_fft, bins, frames per block, waves per block, exchange floats per wave (re and im each)
constexpr int STFT_NFFT = 1024, STFT_BINS = 513, STFT_FPB = 8, STFT_WAVES = 4, STFT_EX = 576;

struct cpx {
  float re, im;
};
// a w.  The imaginary part names the product that is rounded on its own: contraction of a sum of
// two products picks one by the operand order the optimiser happens to leave, which changes with
// the code around the call, and results must not.  (A difference contracts its first product.)
FS2_DEV cpx cmul(cpx a, cpx w) {
  return {a.re * w.re - a.im * w.im, fmaf(a.im, w.re, a.re * w.im)};
}

// 8-point forward DFT in place, natural order in and out (decimation in frequency)
FS2_DEV void dft8(cpx* v) {
  constexpr float H = 0.70710678118654752440f;
  cpx a[4], b[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = {v[j].re + v[j + 4].re, v[j].im + v[j + 4].im};
    b[j] = {v[j].re - v[j + 4].re, v[j].im - v[j + 4].im};
  }
  b[1] = {(b[1].re + b[1].im) * H, (b[1].im - b[1].re) * H};   // W8^1 = (1 - i) / sqrt 2
  b[2] = {b[2].im, -b[2].re};                                  // W8^2 = -i
  b[3] = {(b[3].im - b[3].re) * H, (-b[3].im - b[3].re) * H};  // W8^3 = (-1 - i) / sqrt 2
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const cpx* c = h ? b : a;
    const cpx t0 = {c[0].re + c[2].re, c[0].im + c[2].im};
    const cpx t1 = {c[0].re - c[2].re, c[0].im - c[2].im};
    const cpx t2 = {c[1].re + c[3].re, c[1].im + c[3].im};
    const cpx t3 = {c[1].im - c[3].im, c[3].re - c[1].re};  // (c1 - c3) (-i)
    v[h + 0] = {t0.re + t2.re, t0.im + t2.im};
    v[h + 4] = {t0.re - t2.re, t0.im - t2.im};
    v[h + 2] = {t1.re + t3.re, t1.im + t3.im};
    v[h + 6] = {t1.re - t3.re, t1.im - t3.im};
  }
}

// sample p of a centred frame read from a row of len >= 1 samples: reflected once at each end,
// then clamped into [0, len - 1] (rows shorter than the padding)
FS2_DEV int reflect_index(int p, int len) {
  p = p < 0 ? -p : p;
  p = p > len - 1 ? 2 * (len - 1) - p : p;
  return p < 0 ? 0 : p > len - 1 ? len - 1 : p;
}

// the block stages span[i] = row[reflect_index(p0 + i, len)], i < span_n, clipped to [-1, 1] on
// request
FS2_DEV void stage_span(float* span, const float* row, int p0, int span_n, int len, int tid,
                        bool clip) {
  for (int i = tid; i < span_n; i += 64 * STFT_WAVES) {
    float v = row[reflect_index(p0 + i, len)];
    if (clip) v = fminf(fmaxf(v, -1.f), 1.f);
    span[i] = v;
  }
}

// frame-independent per-lane constants
struct LaneConst {
  cpx tw1[8], tw2[8], tws[8];  // pass 1, pass 2 and split twiddles
  int hi, lo;                  // lane = 8 hi + lo: (s, b) in pass 2, (s, t) in pass 3
  int m;                       // low bin index of this lane after pass 3
  int partner;                 // the lane that holds bins 512 - k
};
// twiddle: (1024, 2), cos and -sin of 2 pi k / 1024
FS2_DEV void lane_consts(LaneConst& c, const float* twiddle, int lane) {
  c.hi = lane >> 3, c.lo = lane & 7;
  c.m = 8 * c.lo + c.hi;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i1 = 2 * lane * j, i2 = 16 * c.lo * j, i3 = 64 * j + c.m;
    c.tw1[j] = {twiddle[2 * i1], twiddle[2 * i1 + 1]};
    c.tw2[j] = {twiddle[2 * i2], twiddle[2 * i2 + 1]};
    c.tws[j] = {twiddle[2 * i3], twiddle[2 * i3 + 1]};
  }
  const int mp = (64 - c.m) & 63;
  c.partner = ((mp & 7) << 3) | (mp >> 3);
}

// the window at the sample pairs 2 n, 2 n + 1 with n = 64 j + r: r = lane for the forward
// transform's input, r = m for the inverse's output
FS2_DEV void load_window(float* win, const float* window, int r) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    win[2 * j] = window[128 * j + 2 * r];
    win[2 * j + 1] = window[128 * j + 2 * r + 1];
  }
}

// z[j] = the windowed sample pair 64 j + lane of the frame at fr
FS2_DEV void load_frame(cpx* z, const float* fr, const float* win, int lane) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int n2 = 128 * j + 2 * lane;
    z[j] = {fr[n2] * win[2 * j], fr[n2 + 1] * win[2 * j + 1]};
  }
}

// Forward 512-point FFT of one wave: in z[j] = x[64 j + lane], out z[q] = X[64 q + 8 lo + hi]
// with lane = 8 hi + lo.  ex_re / ex_im are the wave's own STFT_EX floats; the barriers are block
// wide, so every wave of the block calls this together.
FS2_DEV void fft512(cpx* z, float* ex_re, float* ex_im, const cpx* tw1, const cpx* tw2, int lane,
                    int hi, int lo) {
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
}

// Real-input split of fft512's output z, one bin per call so that a kernel consumes each X as it
// comes: X[64 q + m], q = 0..7, where X[k] = E + W1024^k O, E = (Z[k] + conj Z[512 - k]) / 2,
// O = -i (Z[k] - conj Z[512 - k]) / 2.  Every lane of the wave calls it (a shuffle).
FS2_DEV cpx real_split(const cpx* z, const LaneConst& c, int lane, int q) {
  cpx p = {__shfl(z[7 - q].re, c.partner, 64), __shfl(z[7 - q].im, c.partner, 64)};
  if (lane == 0) p = z[(8 - q) & 7];
  const float er = 0.5f * (z[q].re + p.re), ei = 0.5f * (z[q].im - p.im);
  const float orr = 0.5f * (z[q].im + p.im), oi = -0.5f * (z[q].re - p.re);
  const float xr = er + (c.tws[q].re * orr - c.tws[q].im * oi);
  const float xi = ei + (c.tws[q].re * oi + c.tws[q].im * orr);
  return {xr, xi};
}
// ... and X[512] = Re Z[0] - Im Z[0], real, which lane 0 holds
FS2_DEV float real_split_512(const cpx* z) { return z[0].re - z[0].im; }

}  // namespace fs2
