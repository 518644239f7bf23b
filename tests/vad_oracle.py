"""Oracles of the silence split and the tisv windows (``fs2_nonsilent_split`` and
``fs2_tisv_windows`` as ``include/fs2hip.h`` defines them), in numpy float64.

``split`` is ``librosa.effects.split`` as librosa 0.7.2 writes it (``pad="reflect"``: its
``rms`` frames a reflect-padded signal) and as librosa >= 0.10 does (``pad="zero"``): the mean
square of each centred frame, ``10 log10(max(1e-10, p)) - 10 log10(max(1e-10, p_max)) >
-top_db``, the edges of the runs times ``hop``, clipped to the length.  The rule was read from
librosa's source; librosa is not installed where this was written and nothing here was compared
with it.  Rows of ``frame_length / 2`` samples or fewer, where numpy's reflect needs more than
one reflection, use the kernel's stated index rule instead (-k is k, len - 1 + k is len - 1 - k,
then clamped); an empty row has no interval.

``windows`` is the window rule in integers, ``windows_float`` the reference's loop
(data_preprocess.py:63-66) as written.
"""
import numpy as np


def padded(y, frame_length, pad):
    y = np.asarray(y, np.float64)
    n, half = len(y), frame_length // 2
    p = np.arange(-half, n + half)
    if pad == "zero":
        ok = (p >= 0) & (p < n)
        return np.where(ok, y[np.clip(p, 0, n - 1)], 0.0)
    if pad != "reflect":
        raise ValueError(pad)
    p = np.abs(p)
    p = np.where(p > n - 1, 2 * (n - 1) - p, p)
    return y[np.clip(p, 0, n - 1)]


def frame_power(y, frame_length=2048, hop=512, pad="reflect"):
    """The mean square of each of the ``1 + len // hop`` frames (none for an empty row)."""
    n = len(y)
    if n == 0:
        return np.zeros(0)
    yp = padded(y, frame_length, pad)
    return np.array([np.mean(yp[f * hop:f * hop + frame_length] ** 2) for f in range(1 + n // hop)])


def rel_db(power):
    """Each frame's level against the loudest, in dB, with librosa's floor of 1e-10."""
    power = np.asarray(power, np.float64)
    return 10.0 * np.log10(np.maximum(1e-10, power)) - 10.0 * np.log10(max(1e-10, power.max()))


def split(y, top_db=60.0, frame_length=2048, hop=512, pad="reflect"):
    """``(intervals (n, 2) int64, rel_db per frame)``."""
    n = len(y)
    if n == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0)
    db = rel_db(frame_power(y, frame_length, hop, pad))
    ns = db > -top_db
    edges = [np.flatnonzero(np.diff(ns.astype(int))) + 1]
    if ns[0]:
        edges.insert(0, [0])
    if ns[-1]:
        edges.append([len(ns)])
    edges = np.minimum(np.concatenate(edges).astype(np.int64) * hop, n).reshape(-1, 2)
    return edges, db


def margin(db, top_db):
    """The smallest distance of a frame from the threshold, in dB (inf without frames)."""
    return float(np.abs(np.asarray(db) + top_db).min()) if len(db) else float("inf")


def windows(frames, tisv):
    """First frames of the windows of ``tisv`` frames: ``tisv j // 2`` while
    ``2 frames >= tisv (j + 2)``."""
    out, j = [], 0
    while 2 * frames >= tisv * (j + 2):
        out.append(tisv * j // 2)
        j += 1
    return out


def windows_float(frames, tisv):
    """data_preprocess.py:63-66: ``(start, stop)`` of each slice the reference takes."""
    out, i = [], 0
    while frames >= tisv * (i + 1):
        out.append((int(tisv * i), int(tisv * (i + 1))))
        i += 0.5
    return out


def signal(n, loud, seed=0, level=0.5, floor=1e-6):
    """Random signs at ``floor``, at ``level`` inside the ``(lo, hi)`` spans of ``loud``: a
    frame's power depends only on how many loud samples it covers."""
    rng = np.random.default_rng(seed)
    a = np.full(n, floor)
    for lo, hi in loud:
        a[lo:hi] = level
    return (rng.choice([-1.0, 1.0], n) * a).astype(np.float32)
