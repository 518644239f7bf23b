// Complex arithmetic and the radix-8 butterfly shared by the FFT kernels (melspec.hip,
// griffinlim.hip): 512 = 8^3, so a 512-point complex transform is three dft8 passes per wave
// with 8 complex values per lane.
#pragma once
#include "common.hpp"

namespace fs2 {

struct cpx {
  float re, im;
};
FS2_DEV cpx cmul(cpx a, cpx w) { return {a.re * w.re - a.im * w.im, a.re * w.im + a.im * w.re}; }

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

}  // namespace fs2
