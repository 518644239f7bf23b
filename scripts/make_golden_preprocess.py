"""Expected outputs of the post-contour preprocessing fixtures of ``tests/pitch_oracle.py``, made by
the libraries the reference itself calls (preprocessor/preprocessor.py): ``scipy.interpolate.
interp1d`` (213-221), ``np.percentile`` (307-315) and ``sklearn.preprocessing.StandardScaler``
(94-97), in float64 as the reference holds its pitch.  Run where scipy and sklearn are installed
(``python scripts/make_golden_preprocess.py``); no test calls it and only data leaves it, so
neither the CPU nor the GPU tests need sklearn.

  tests/golden/g16_preprocess.npz
    fill, fill_ok       (6, 37) interpolated rows (untouched where ok = 0) and the flags
    seg                 (3, 6) phoneme means of the in-place loop (223-231), zero padded
    mom                 [n_samples_seen_, mean_, var_ * n, scale_] after the six rows
    mom_min, mom_max    extrema of the rows normalised with them (317-328), stored as float32
    corpus_stats        stats.json's [min, max, mean, std] (126-141) of the three-utterance corpus
"""
import os
import sys

import numpy as np
from scipy.interpolate import interp1d
from sklearn.preprocessing import StandardScaler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import pitch_oracle as O  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g16_preprocess.npz")


def fill(pitch):
    nonzero_ids = np.where(pitch != 0)[0]
    interp_fn = interp1d(nonzero_ids, pitch[nonzero_ids],
                         fill_value=(pitch[nonzero_ids[0]], pitch[nonzero_ids[-1]]),
                         bounds_error=False)
    return interp_fn(np.arange(0, len(pitch)))


def remove_outlier(values):
    values = np.array(values)
    p25, p75 = np.percentile(values, 25), np.percentile(values, 75)
    lower, upper = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
    return values[np.logical_and(values > lower, values < upper)]


def fit(rows):
    scaler = StandardScaler()
    for r in rows:
        kept = remove_outlier(r.astype(np.float64))
        if len(kept) > 0:
            scaler.partial_fit(kept.reshape((-1, 1)))
    return scaler


def extrema(rows, mean, std):
    hi, lo = np.finfo(np.float64).min, np.finfo(np.float64).max
    for r in rows:
        values = ((r.astype(np.float64) - mean) / std).astype(np.float32)
        hi, lo = max(hi, max(values)), min(lo, min(values))
    return float(lo), float(hi)


def main():
    x, n = O.fill_rows()
    filled, ok = x.astype(np.float64), np.zeros(len(n), np.int32)
    for b, k in enumerate(n):
        if np.sum(x[b, :k] != 0) > 1:
            filled[b, :k], ok[b] = fill(x[b, :k].astype(np.float64)), 1

    v, live, durs = O.segment_rows()
    seg = np.zeros((len(durs), max(len(d) for d in durs)))
    for b, d in enumerate(durs):
        pitch, pos = v[b, :live[b]].astype(np.float64), 0
        for i, dd in enumerate(d):
            pitch[i] = np.mean(pitch[pos:pos + dd]) if dd > 0 else 0
            pos += dd
        seg[b, :len(d)] = pitch[:len(d)]

    rows = O.moment_rows()
    sc = fit(rows)
    mom = np.array([sc.n_samples_seen_, sc.mean_[0], sc.var_[0] * sc.n_samples_seen_, sc.scale_[0]],
                   np.float64)
    mom_min, mom_max = extrema(rows, sc.mean_[0], sc.scale_[0])

    corpus = O.corpus_rows()
    cs = fit(corpus)
    lo, hi = extrema(corpus, cs.mean_[0], cs.scale_[0])
    np.savez(OUT, fill=filled, fill_ok=ok, seg=seg, mom=mom, mom_min=np.float64(mom_min),
             mom_max=np.float64(mom_max),
             corpus_stats=np.array([lo, hi, cs.mean_[0], cs.scale_[0]], np.float64))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
