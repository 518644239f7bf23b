"""Oracles of the pitch path.

The F0 estimator is YIN (de Cheveigne & Kawahara 2002) as ``include/fs2hip.h`` defines it at
``fs2_f0_yin``; the reference calls pyworld (preprocessor/preprocessor.py:196-201), which is not
installed, so nothing here is compared with it.  ``oracle64`` is the definition in float64;
``ref32`` does every step in float32 with d(tau) accumulated left to right, as one lane of the
kernel does.  Their difference on an input is the rounding error of the float32 formulation
there, which is what the GPU tests scale their tolerance from.

Everything after the contour is transliterated from the reference, each function citing its
lines; nothing is copied.
"""
import math

import numpy as np

SR, HOP, W = 22050, 256, 512
F0_FLOOR, F0_CEIL, THRESHOLD = 71.0, 800.0, 0.15


def lag_range(sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    return int(math.ceil(sr / f0_ceil)), int(math.floor(sr / f0_floor))


def n_frames(length, hop):
    return 1 + length // hop


def yin(x, n, dtype, hop=HOP, sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, threshold=THRESHOLD):
    """The first ``n`` samples of ``x`` -> ``(f0, dip, margin)``, one value per frame, every step
    in ``dtype``.  ``margin`` is the smallest absolute difference in any comparison the frame's
    decision made: d'(tau) against the threshold up to and including the first crossing (over
    the whole range for an unvoiced frame) and d'(tau + 1) against d'(tau) on the descent."""
    T = dtype
    tmin, tmax = lag_range(sr, f0_floor, f0_ceil)
    L = W + tmax
    x = np.asarray(x)[:n].astype(T)
    nf = n_frames(n, hop)
    thr, lo, hi, srt = T(threshold), T(f0_floor), T(f0_ceil), T(sr)
    f0, dip, margin = np.zeros(nf, T), np.zeros(nf, T), np.zeros(nf, np.float64)
    lagged = np.arange(1, tmax + 1)[:, None] + np.arange(W)[None, :]
    for k in range(nf):
        seg = np.zeros(L, T)
        start = k * hop - L // 2
        a, b = max(start, 0), min(start + L, n)
        if b > a:
            seg[a - start:b - start] = x[a:b]
        d = np.zeros(tmax + 1, T)
        diff = seg[None, :W] - seg[lagged]
        d[1:] = np.cumsum(diff * diff, axis=1, dtype=T)[:, -1]  # each lag left to right
        cs = np.cumsum(d[1:], dtype=T)
        dp = np.ones(tmax + 1, T)
        for tau in range(1, tmax + 1):
            c = cs[tau - 1]
            dp[tau] = (d[tau] * T(tau)) / c if c != 0 else T(1)
        rng = np.arange(tmin, tmax + 1)
        under = np.flatnonzero(dp[rng] < thr)
        if under.size == 0:
            dip[k] = dp[rng].min()
            margin[k] = np.abs(dp[rng].astype(np.float64) - float(thr)).min()
            continue
        tau = int(rng[under[0]])
        m = np.abs(dp[tmin:tau + 1].astype(np.float64) - float(thr)).min()
        while tau + 1 <= tmax:
            m = min(m, abs(float(dp[tau + 1]) - float(dp[tau])))
            if not dp[tau + 1] < dp[tau]:
                break
            tau += 1
        margin[k] = m
        dip[k] = dp[tau]
        off = T(0)
        if tau < tmax:
            ya, yb, yc = dp[tau - 1], dp[tau], dp[tau + 1]
            den = (ya - T(2) * yb) + yc
            if den > 0:
                off = min(max((T(0.5) * (ya - yc)) / den, T(-1)), T(1))
        f = srt / (T(tau) + off)
        f0[k] = f if lo <= f <= hi else T(0)
    return f0, dip, margin


def oracle64(x, n=None, **kw):
    return yin(x, len(x) if n is None else n, np.float64, **kw)


def ref32(x, n=None, **kw):
    return yin(x, len(x) if n is None else n, np.float32, **kw)


def rule(ref, want, got_like):
    """The project's tolerance rule per value: max(4 x max|ref32 - oracle64| on that input,
    4 fp32 ulps of the value)."""
    want = np.asarray(want, np.float64)
    spread = 4.0 * float(np.abs(np.asarray(ref, np.float64) - want).max()) if want.size else 0.0
    ulps = 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return np.maximum(spread, ulps) + 0.0 * np.asarray(got_like, np.float64)


def voice(n, f_a, f_b, seed, snr_db=30.0, gaps=()):
    """Six harmonics (amplitudes 1, .6, .4, .3, .2, .1, random phases) on a linear F0 glide from
    ``f_a`` to ``f_b`` Hz, peak 0.2, white noise at ``snr_db``, zeroed ``gaps`` [(a, b), ...];
    float32."""
    rng = np.random.default_rng(seed)
    f = np.linspace(f_a, f_b, n)
    phase = 2.0 * np.pi * np.cumsum(f) / SR
    x = sum(a * np.sin(h * phase + 2.0 * np.pi * rng.random())
            for h, a in zip(range(1, 7), (1.0, 0.6, 0.4, 0.3, 0.2, 0.1)))
    x = 0.2 * x / np.abs(x).max()
    x = x + rng.standard_normal(n) * np.sqrt(np.mean(x * x) / 10.0 ** (snr_db / 10.0))
    for a, b in gaps:
        x[a:b] = 0.0
    return x.astype(np.float32)


# ------------------------------------------------------------------ after the contour
def fill(pitch):
    """preprocessor.py:204, 213-221: ``None`` with at most one non-zero frame, else the linear
    interpolation over the zero frames, the first value held before and the last after
    (scipy's interp1d: slope * (x - x_lo) + y_lo, in the array's dtype)."""
    pitch = np.asarray(pitch)
    if np.sum(pitch != 0) <= 1:
        return None
    ids = np.where(pitch != 0)[0]
    out = pitch.copy()
    for i in range(len(pitch)):
        if pitch[i] != 0:
            continue
        if i < ids[0]:
            out[i] = pitch[ids[0]]
        elif i > ids[-1]:
            out[i] = pitch[ids[-1]]
        else:
            hi = int(np.searchsorted(ids, i))
            p, q = ids[hi - 1], ids[hi]
            slope = (pitch[q] - pitch[p]) / pitch.dtype.type(q - p)
            out[i] = slope * pitch.dtype.type(i - p) + pitch[p]
    return out


def segment_mean(values, duration):
    """preprocessor.py:223-231 (and 234-242): the in-place loop, writes and all."""
    values = np.array(values)
    pos = 0
    for i, d in enumerate(duration):
        if d > 0:
            values[i] = np.mean(values[pos:pos + d])
        else:
            values[i] = 0
        pos += d
    return values[:len(duration)]


def remove_outlier(values):
    """preprocessor.py:307-315."""
    values = np.array(values)
    p25 = np.percentile(values, 25)
    p75 = np.percentile(values, 75)
    lower = p25 - 1.5 * (p75 - p25)
    upper = p75 + 1.5 * (p75 - p25)
    return values[np.logical_and(values > lower, values < upper)]


class Moments:
    """StandardScaler.partial_fit as preprocessor.py:94-97 uses it: the incremental count, mean
    and sum of squared deviations (Chan, Golub & LeVeque), ``scale_`` with sklearn's zero rule."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0.0, 0.0, 0.0

    def partial_fit(self, values):
        v = np.asarray(values, np.float64)
        if v.size == 0:
            return self
        cnt, mean = float(v.size), float(v.mean())
        m2 = float(((v - mean) ** 2).sum())
        if self.n == 0:
            self.n, self.mean, self.m2 = cnt, mean, m2
        else:
            tot, delta = self.n + cnt, mean - self.mean
            self.mean += delta * (cnt / tot)
            self.m2 += m2 + delta * delta * (self.n * cnt / tot)
            self.n = tot
        return self

    @property
    def scale(self):
        std = math.sqrt(self.m2 / self.n)
        return std if std > 0 else 1.0


def normalize(rows, mean, std):
    """preprocessor.py:317-328 over arrays instead of files: the normalised rows (stored as
    float32, as the package keeps them) and the extrema of what was stored."""
    max_value, min_value = np.finfo(np.float64).min, np.finfo(np.float64).max
    out = []
    for values in rows:
        values = ((np.asarray(values, np.float64) - mean) / std).astype(np.float32)
        out.append(values)
        if len(values):
            max_value = max(max_value, float(max(values)))
            min_value = min(min_value, float(min(values)))
    return out, min_value, max_value


def get_alignment(intervals, sr=SR, hop=HOP):
    """preprocessor.py:267-305 over (start, end, text) tuples."""
    sil_phones = ["sil", "sp", "spn", "silB", "silE", ""]
    phones, durations = [], []
    start_time, end_time, end_idx = 0, 0, 0
    for s, e, p in intervals:
        if phones == []:
            if p in sil_phones:
                continue
            else:
                start_time = s
        if p not in sil_phones:
            phones.append(p)
            end_time = e
            end_idx = len(phones)
        else:
            phones.append("sp")
        durations.append(int(np.round(e * sr / hop) - np.round(s * sr / hop)))
    phones = phones[:end_idx]
    durations = durations[:end_idx]
    assert len(phones) == len(durations)
    return phones, durations, start_time, end_time


# ------------------------------------------------------------------ shared fixtures
def fill_rows():
    """(B = 6, F = 37) rows and their live counts: all voiced; leading and trailing zeros;
    interior gaps of 1 and 9 frames; one non-zero frame; none; n = 1."""
    rng = np.random.default_rng(11)
    x = (100.0 + 150.0 * rng.random((6, 37))).astype(np.float32)
    n = [37, 30, 33, 21, 12, 1]
    x[1, :4] = 0
    x[1, 25:30] = 0
    x[2, 7] = 0
    x[2, 15:24] = 0
    x[3] = 0
    x[3, 9] = 181.25
    x[4] = 0
    for b, k in enumerate(n):  # what follows a row is not zeros
        x[b, k:] = 55.5
    return x, n


def segment_rows():
    """Values (3, 9), live frames and durations: the overwritten-read quirk, plain, and a
    trailing zero duration (one live frame more than the durations cover, or the reference's
    write of ``pitch[5]`` would be out of bounds)."""
    rng = np.random.default_rng(12)
    x = (1.0 + 9.0 * rng.random((3, 9))).astype(np.float32)
    durs = [[0, 0, 3, 1, 0, 2], [2, 2, 2], [1] * 5 + [0]]
    return x, [6, 7, 6], durs


def moment_rows():
    """Rows of 1, 2, 5, 64, 257 values and one of 40 equal values (IQR 0: every value is
    removed), as float32."""
    rng = np.random.default_rng(13)
    rows = [(150.0 + 40.0 * rng.standard_normal(k)).astype(np.float32) for k in (1, 2, 5, 64, 257)]
    rows[3][5], rows[4][100], rows[4][7] = 900.0, -300.0, 1200.0  # outliers to remove
    rows.append(np.full(40, 123.5, np.float32))
    return rows


def corpus_rows():
    """Three utterances' phoneme-level values for CorpusStats."""
    rng = np.random.default_rng(14)
    rows = [(200.0 + 30.0 * rng.standard_normal(k)).astype(np.float32) for k in (23, 9, 41)]
    rows[0][3], rows[2][17] = 700.0, 20.0
    return rows
