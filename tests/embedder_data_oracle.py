"""numpy restatements for the speaker encoder's data path and EER test, and the self-describing
synthetic corpus of fixture g15 (``scripts/make_golden_embedder_data.py``).

Corpus: element ``[u, c, f]`` of file ``k`` (index in sorted-name order) is
``float32(((k * 8 + u) * 128 + c) * 256 + f)`` -- exact below 2^24 -- so a gathered value says
which file, utterance, channel and frame it came from.
"""
import os

import numpy as np

NMELS = 80
# (name, utterances, frames): three files per language, utterance counts below and above M = 3,
# one file with more than tisv_frame = 150 frames; names are in sorted order
FILES = (("jvs_001_M_japanese.npy", 2, 150), ("jvs_002_F_japanese.npy", 5, 163),
         ("jvs_003_M_japanese.npy", 3, 150), ("vctk_p225_F_english.npy", 7, 150),
         ("vctk_p226_M_english.npy", 2, 150), ("vctk_p227_M_english.npy", 4, 150))
NAMES = tuple(f[0] for f in FILES)


def file_array(k):
    _, u, t = FILES[k]
    a = ((k * 8 + np.arange(u)[:, None, None]) * 128 + np.arange(NMELS)[None, :, None]) * 256 \
        + np.arange(t)[None, None, :]
    assert a.max() < 2 ** 24
    return a.astype(np.float32)


def write_corpus(path):
    """Writes the six files; returns their names (sorted)."""
    for k, (name, _, _) in enumerate(FILES):
        np.save(os.path.join(path, name), file_array(k))
    return list(NAMES)


def decode(v):
    """value(s) -> (file k, utterance u, channel c, frame f)."""
    v = np.asarray(v).astype(np.int64)
    return v >> 18, (v >> 15) & 7, (v >> 8) & 127, v & 255


def gather(store, row_off, row_stride, row_start, n_mels, length):
    """fs2_mel_crop_gather by numpy indexing: (rows, length, n_mels)."""
    out = np.empty((len(row_off), length, n_mels), np.float32)
    for r, (o, s, p) in enumerate(zip(row_off, row_stride, row_start)):
        src = store[int(o):int(o) + n_mels * int(s)].reshape(n_mels, int(s))
        out[r] = src[:, int(p):int(p) + length].T
    return out


def cossim(enroll, verify):
    """get_cossim(verify, get_centroids(enroll)) (utils.py:169-236) in float64: (N, M_v, N); the
    k = j entries against the verification utterances' exclude-self centroid; + 1e-6."""
    e, v = np.asarray(enroll, np.float64), np.asarray(verify, np.float64)
    n, mv, _ = v.shape
    cent = e.mean(1)
    excl = (v.sum(1, keepdims=True) - v) / (mv - 1)

    def cos(a, b):
        return (a * b).sum(-1) / (np.maximum(np.linalg.norm(a, axis=-1), 1e-8) *
                                  np.maximum(np.linalg.norm(b, axis=-1), 1e-8))

    sim = cos(v[:, :, None, :], cent[None, None, :, :])
    idx = np.arange(n)
    sim[idx, :, idx] = cos(v, excl)
    return sim + 1e-6


def thresholds():
    return np.array([np.float32(0.01 * i + 0.5) for i in range(50)], np.float32)


def eer_sweep(sim):
    """The threshold sweep of test() (train_speech_embedder.py:433-450) on sim (N, M, N):
    table (50, 2) = FAR, FRR and result (4) = EER, threshold, FAR, FRR, in float32 from integer
    counts with the reference's order of divisions."""
    sim = np.asarray(sim, np.float32)
    n, m, _ = sim.shape
    f = np.float32
    own = np.eye(n, dtype=bool)[:, None, :].repeat(m, 1)
    table = np.zeros((50, 2), np.float32)
    result = np.zeros(4, np.float32)
    best = f(1)
    for i, thr in enumerate(thresholds()):
        on = sim > thr
        accepted, same = int(on.sum()), int((on & own).sum())
        far = f(accepted - same) / f(n - 1) / f(m) / f(n)
        frr = f(n * m - same) / f(m) / f(n)
        table[i] = far, frr
        if best > abs(far - frr):
            best = abs(far - frr)
            result[:] = (far + frr) / f(2), thr, far, frr
    return table, result


def threshold_gap(sim):
    """Smallest distance of any sim entry to any threshold."""
    return float(np.abs(np.asarray(sim, np.float64)[..., None] -
                        thresholds().astype(np.float64)).min())
