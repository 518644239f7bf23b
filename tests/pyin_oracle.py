"""Oracle of the pYIN path (Mauch & Dixon 2014) as ``include/fs2hip.h`` defines it at
``fs2_f0_pyin``: every threshold of a Beta(2, 18) prior votes for the pick plain YIN makes at that
threshold, the votes become per-frame observations over (pitch bin, voiced / unvoiced) states, and
a Viterbi pass in the probability domain picks the track.

``oracle64`` does the YIN stage (d', the picks, the parabola) in float64, ``ref32`` in float32 with
d(tau) accumulated left to right as one lane of the kernel does; everything after the candidate
f0 (bins, masses, observations, Viterbi) is float64 in both, with the operations and their order
spelled out so that the kernel can reproduce the bits.  Nothing is compared with librosa's or the
authors' implementation: neither is installed.
"""
import math

import numpy as np

from pitch_oracle import (F0_CEIL, F0_FLOOR, HOP, SR, W, fill, lag_range,  # noqa: F401
                          n_frames, rule, segment_mean, voice)

N_THRESH, BINS_PER_SEMITONE = 100, 5
P_ABSENT, OBS_FLOOR, P_STAY, P_SWITCH = 0.01, 1e-9, 0.99, 0.01
STEP = 12 * BINS_PER_SEMITONE  # bins per octave


# ------------------------------------------------------------------ host tables
def beta_cdf(x):
    """The Beta(2, 18) CDF in closed form (integer parameters)."""
    return 1.0 - (1.0 - x) ** 19 - 19.0 * x * (1.0 - x) ** 18


def thresholds():
    """theta_0 = 0 and theta_i = float32(i / 100), i = 1..100, as float64."""
    return np.array([float(np.float32(i / 100.0)) for i in range(N_THRESH + 1)])


def beta_weights():
    """w_i = I(theta_i) - I(theta_{i - 1}), i = 1..100 (index i - 1), Python floats throughout."""
    th = thresholds().tolist()
    return np.array([beta_cdf(th[i]) - beta_cdf(th[i - 1]) for i in range(1, N_THRESH + 1)])


def bin_count(f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    return int(math.floor(STEP * math.log2(f0_ceil / f0_floor))) + 1


def reach(hop=HOP, sr=SR):
    """R: the widest jump, in bins, between two frames (35.92 octaves per second)."""
    return int(round(35.92 * STEP * hop / sr))


def tri_table(R):
    """tri(0..R) = (R + 1 - delta) / (R + 1)^2."""
    return np.array([(R + 1 - d) / float((R + 1) ** 2) for d in range(R + 1)])


def bin_centres(n_bins, f0_floor=F0_FLOOR):
    return np.array([f0_floor * 2.0 ** (b / float(STEP)) for b in range(n_bins)]).astype(np.float32)


def transition(n_bins, tri):
    """P[s, s'] over s = v * n_bins + b (voiced first): tri(|b' - b|) * (0.99 | 0.01), each entry
    one float64 product; zero outside the reach."""
    R = len(tri) - 1
    delta = np.abs(np.arange(n_bins)[:, None] - np.arange(n_bins)[None, :])
    band = np.where(delta <= R, np.asarray(tri, np.float64)[np.minimum(delta, R)], 0.0)
    stay, move = band * P_STAY, band * P_SWITCH
    return np.block([[stay, move], [move, stay]])


# ------------------------------------------------------------------ Viterbi
def observations(mass, voiced):
    """mass (F, n_bins), voiced (F) = min(sum_b mass, 1) -> obs (F, 2 n_bins)."""
    mass = np.asarray(mass, np.float64)
    nb = mass.shape[1]
    un = (1.0 - np.asarray(voiced, np.float64)) / float(nb) + OBS_FLOOR
    return np.concatenate([mass + OBS_FLOOR, np.repeat(un[:, None], nb, axis=1)], axis=1)


def viterbi(obs, P):
    """The state path of obs (F, S) under P (S, S): products, one division by the frame's maximum
    per frame, first index on ties (numpy argmax)."""
    obs = np.asarray(obs, np.float64)
    F, S = obs.shape
    if F == 0:
        return np.zeros(0, np.int64)
    d = obs[0] / float(S)
    d = d / d.max()
    bp = np.zeros((F, S), np.int64)
    cols = np.arange(S)
    for k in range(1, F):
        cand = d[:, None] * P
        bp[k] = cand.argmax(axis=0)
        d = cand[bp[k], cols] * obs[k]
        d = d / d.max()
    path = np.zeros(F, np.int64)
    path[-1] = int(d.argmax())
    for k in range(F - 1, 0, -1):
        path[k - 1] = bp[k, path[k]]
    return path


def viterbi_brute(obs, P):
    """Every path enumerated (tiny HMMs only): the same recursion's value of a whole path is the
    product along it; the best path, ties to the path the recursion's rule prefers, which is the
    lexicographically smallest when read from the last frame backwards."""
    import itertools
    obs = np.asarray(obs, np.float64)
    F, S = obs.shape
    best, best_path = -1.0, None
    for path in itertools.product(range(S), repeat=F):
        p = obs[0, path[0]] / float(S)
        for k in range(1, F):
            p = p * P[path[k - 1], path[k]] * obs[k, path[k]]
        key = path[::-1]
        if p > best or (p == best and key < best_path[::-1]):
            best, best_path = p, path
    return np.asarray(best_path, np.int64)


# ------------------------------------------------------------------ candidates
def _dprime(x, n, T, hop, tmin, tmax):
    """d'(0..tau_max) of every frame, as ``pitch_oracle.yin`` computes it."""
    L = W + tmax
    nf = n_frames(n, hop)
    lagged = np.arange(1, tmax + 1)[:, None] + np.arange(W)[None, :]
    for k in range(nf):
        seg = np.zeros(L, T)
        start = k * hop - L // 2
        a, b = max(start, 0), min(start + L, n)
        if b > a:
            seg[a - start:b - start] = x[a:b]
        d = np.zeros(tmax + 1, T)
        diff = seg[None, :W] - seg[lagged]
        d[1:] = np.cumsum(diff * diff, axis=1, dtype=T)[:, -1]
        cs = np.cumsum(d[1:], dtype=T)
        dp = np.ones(tmax + 1, T)
        for tau in range(1, tmax + 1):
            c = cs[tau - 1]
            dp[tau] = (d[tau] * T(tau)) / c if c != 0 else T(1)
        yield dp


def _refine(dp, tau, tmax, T, srt):
    """The descent and the parabola of ``fs2_f0_yin`` from a starting lag."""
    while tau + 1 <= tmax and dp[tau + 1] < dp[tau]:
        tau += 1
    off = T(0)
    if tau < tmax:
        ya, yb, yc = dp[tau - 1], dp[tau], dp[tau + 1]
        den = (ya - T(2) * yb) + yc
        if den > 0:
            off = min(max((T(0.5) * (ya - yc)) / den, T(-1)), T(1))
    return srt / (T(tau) + off)


def candidates(x, n, dtype, hop=HOP, sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    """-> ``(mass (F, n_bins) f64, cand_f0 (F, n_bins) dtype, voiced (F) f64)``: per frame and bin
    the summed prior mass of the thresholds whose pick falls there (ascending i), the f0 of the
    lowest such i, and min(sum_b mass, 1) with b ascending."""
    T = dtype
    tmin, tmax = lag_range(sr, f0_floor, f0_ceil)
    nb = bin_count(f0_floor, f0_ceil)
    x = np.asarray(x)[:n].astype(T)
    nf = n_frames(n, hop)
    lo, hi, srt = T(f0_floor), T(f0_ceil), T(sr)
    th = [T(np.float32(i / 100.0)) for i in range(N_THRESH + 1)]
    w = beta_weights().tolist()
    mass, cf0, voiced = np.zeros((nf, nb)), np.zeros((nf, nb), T), np.zeros(nf)
    rng = np.arange(tmin, tmax + 1)
    for k, dp in enumerate(_dprime(x, n, T, hop, tmin, tmax)):
        seen = np.zeros(nb, bool)
        cache = {}
        for i in range(1, N_THRESH + 1):
            under = np.flatnonzero(dp[rng] < th[i])
            if under.size:
                start, m = int(rng[under[0]]), w[i - 1]
            else:
                start, m = int(rng[int(np.argmin(dp[rng]))]), w[i - 1] * P_ABSENT
                if not dp[start] < 1:  # d' is 1 by convention where there is no energy: no vote
                    continue
            if start not in cache:
                cache[start] = _refine(dp, start, tmax, T, srt)
            f = cache[start]
            if not lo <= f <= hi:
                continue
            b = int(np.rint(float(STEP) * np.log2(np.float64(f) / np.float64(lo))))
            b = min(max(b, 0), nb - 1)
            if not seen[b]:
                seen[b], cf0[k, b] = True, f
            mass[k, b] = mass[k, b] + m
        voiced[k] = min(float(np.cumsum(mass[k])[-1]), 1.0)  # b ascending, one accumulator
    return mass, cf0, voiced


def pyin(x, n, dtype, hop=HOP, sr=SR, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    """-> a dict: ``f0`` (F) float32-valued contour (0 = unvoiced), ``unvoiced`` (F) = 1 - v,
    ``states`` (F), and the stage results ``mass``, ``cand_f0``, ``voiced``."""
    mass, cf0, voiced = candidates(x, n, dtype, hop, sr, f0_floor, f0_ceil)
    nb = mass.shape[1]
    tri = tri_table(reach(hop, sr))
    states = viterbi(observations(mass, voiced), transition(nb, tri))
    centres = bin_centres(nb, f0_floor)
    f0 = np.zeros(len(states), dtype)
    for k, s in enumerate(states):
        if s < nb:
            f0[k] = cf0[k, s] if cf0[k, s] != 0 else dtype(centres[s])
    return {"f0": f0, "unvoiced": 1.0 - voiced, "states": states, "mass": mass, "cand_f0": cf0,
            "voiced": voiced}


def oracle64(x, n=None, **kw):
    return pyin(x, len(x) if n is None else n, np.float64, **kw)


def ref32(x, n=None, **kw):
    return pyin(x, len(x) if n is None else n, np.float32, **kw)


# ------------------------------------------------------------------ shared fixtures
def cases():
    """``(tag, x, kwargs)`` of every waveform the GPU tests put through the kernels: the inputs of
    test_gpu_pitch.py's table (the four utterances at both hops, the edge cases, the floors that
    select the other kernel instances) and the longest utterance again at 3 dB SNR."""
    import test_gpu_pitch as T
    out = []
    for hop in (256, 200):
        for n, x in zip(T.LENS, T._utts()):
            out.append((f"len {n} hop {hop}", x, dict(hop=hop)))
        out.append((f"len 8192 at 3 dB hop {hop}", noisy(), dict(hop=hop)))
    out += [(kind, make(), {}) for kind, make in T.EDGES.items()]
    low, high = voice(4100, 110.0, 180.0, 3), voice(4100, 500.0, 600.0, 9)
    for x, floor in ((low, 44.0), (low, 50.0), (low, 120.0), (high, 350.0)):
        out.append((f"floor {floor}", x, dict(f0_floor=floor, f0_ceil=700.0)))
    return out


def noisy():
    return voice(8192, 150.0, 220.0, 4, snr_db=3.0)


_WANT = {}


def want(tag, x, **kw):
    """``(oracle64, ref32)`` of one case, computed once per session and not to be modified."""
    if tag not in _WANT:
        _WANT[tag] = (oracle64(x, **kw), ref32(x, **kw))
    return _WANT[tag]
