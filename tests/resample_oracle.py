"""Oracles of the resampler (``fs2_resample`` as ``include/fs2hip.h`` defines it).

``design`` is the filter: a Kaiser-windowed sinc with the design numbers of resampy's
``kaiser_best`` (what ``librosa == 0.7.2`` uses in ``load``), evaluated in float64 exactly at the
offsets a rational ratio needs.  resampy instead interpolates a 512-point table of the same
window, and neither it nor soxr is installed, so nothing here is compared with them.

``oracle64`` is the definition in float64, a direct sum per output; ``ref32`` does it in float32
in the kernel's documented order: one accumulator per output, samples ascending, each product
rounded before it is added.  Their difference on a row is the rounding error of the float32
formulation there, which the GPU tests scale their tolerance from.
"""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492


def ratio(sr_in, sr_out):
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def design(sr_in, sr_out, zeros=ZEROS):
    """``(h float64 (2 half + 1), L, M, half)``; the kernel's table is ``float32(L * h)``."""
    L, M = ratio(sr_in, sr_out)
    big = max(L, M)
    half = int(math.ceil(zeros * big / ROLLOFF))
    t = np.arange(-half, half + 1, dtype=np.float64)
    window = np.i0(BETA * np.sqrt(np.maximum(1.0 - (t / half) ** 2, 0.0))) / np.i0(BETA)
    h = (ROLLOFF / big) * np.sinc(ROLLOFF * t / big) * window
    return h, L, M, half


def table32(sr_in, sr_out, zeros=ZEROS):
    h, L, M, half = design(sr_in, sr_out, zeros)
    return (L * h).astype(np.float32), L, M, half


def n_out(length, L, M):
    return (int(length) * L + M - 1) // M


def oracle64(x, sr_in, sr_out, table=None):
    """The definition in float64 over all of ``x``; ``table`` defaults to the float32 table the
    kernel reads (so the comparison isolates the arithmetic on samples), pass ``L * h`` for the
    unrounded filter."""
    tab, L, M, half = table32(sr_in, sr_out)
    tab = np.asarray(tab if table is None else table, np.float64)
    x = np.asarray(x, np.float64)
    y = np.zeros(n_out(len(x), L, M), np.float64)
    for n in range(len(y)):
        c = n * M + half
        j_lo = max(0, -((2 * half - c) // L))  # ceil((c - 2 half) / L)
        j_hi = min(len(x) - 1, c // L)
        if j_hi >= j_lo:
            j = np.arange(j_lo, j_hi + 1)
            y[n] = np.dot(tab[c - j * L], x[j])
    return y


def ref32(x, sr_in, sr_out):
    """float32, the kernel's order, vectorised over the outputs: tap step k from K - 1 down to 0
    is sample ``floor((n M + half) / L) - k``, ascending in j."""
    tab, L, M, half = table32(sr_in, sr_out)
    x = np.asarray(x, np.float32)
    n = np.arange(n_out(len(x), L, M), dtype=np.int64)
    c = n * M + half
    jt, r = c // L, c % L
    acc = np.zeros(len(n), np.float32)
    for k in range(2 * half // L, -1, -1):
        i, j = r + k * L, jt - k
        ok = (i <= 2 * half) & (j >= 0) & (j < len(x))
        t = np.where(ok, tab[np.minimum(i, 2 * half)], np.float32(0))
        s = np.where(ok, x[np.clip(j, 0, len(x) - 1)], np.float32(0))
        acc = acc + (t * s).astype(np.float32)
    return acc


def rule(ref, want):
    """The project's tolerance rule per value: max(4 x max|ref32 - oracle64| on that row,
    4 fp32 ulps of the value)."""
    want = np.asarray(want, np.float64)
    spread = 4.0 * float(np.abs(np.asarray(ref, np.float64) - want).max()) if want.size else 0.0
    ulps = 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return np.maximum(spread, ulps)
