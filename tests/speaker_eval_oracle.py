"""numpy oracle of the generated-speaker metrics (csrc/speaker_eval.hip, speaker_eval.py).

The neighbour search mirrors the kernel's arithmetic contract: per pair three fp64 sums (dot,
|a|^2, |b|^2), each over d = 0 .. D-1 in that order by an explicit loop vectorised over the pairs
(a product of two fp32 values is exact in fp64, so there is nothing for a fused multiply-add to
change), den = sqrt(|a|^2) sqrt(|b|^2), c = den > 0 ? dot / den : 0, dist = float32(1 - c); then a
stable argsort, so ties go to the lower index.  The summary's median is numpy.median of the finite
entries in fp64, its mean a running fp64 sum in index order.  The Frechet distance goes by
numpy.linalg.eigh with the kernel's clipping; ``frechet_sqrtm`` is the textbook
scipy.linalg.sqrtm formulation it is checked against.

``Ops`` gives ``speaker_eval.table`` these functions on CPU tensors, so the table's bookkeeping
runs without the library.
"""
import numpy as np


def cosine_dist(a, b):
    """(Na, Nb) float32 cosine distances by the contract above."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    na, nb = a.shape[0], b.shape[0]
    dot = np.zeros((na, nb))
    a2 = np.zeros(na)
    b2 = np.zeros(nb)
    for d in range(a.shape[1]):
        dot = dot + a[:, d][:, None] * b[:, d][None, :]
        a2 = a2 + a[:, d] * a[:, d]
        b2 = b2 + b[:, d] * b[:, d]
    den = np.sqrt(a2)[:, None] * np.sqrt(b2)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(den > 0, dot / den, 0.0)
    return (1.0 - c).astype(np.float32)


def nearest(a, b, k=1, group_a=None, group_b=None, same=False):
    """(dist (Na, k) float32, index (Na, k) int64); +inf / -1 where a row runs out of candidates."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = a.shape[0], b.shape[0]
    dist = np.full((na, k), np.inf, np.float32)
    index = np.full((na, k), -1, np.int64)
    if nb == 0:
        return dist, index
    full = cosine_dist(a, b)
    keep = np.ones((na, nb), bool)
    if group_a is not None:
        eq = np.asarray(group_a)[:, None] == np.asarray(group_b)[None, :]
        keep = eq if same else ~eq
    for i in range(na):
        cand = np.flatnonzero(keep[i])
        order = cand[np.argsort(full[i, cand], kind="stable")][:k]
        dist[i, :len(order)] = full[i, order]
        index[i, :len(order)] = order
    return dist, index


def summary_array(x):
    """float64[5]: count, median, mean, min, max of the finite entries."""
    x = np.asarray(x, np.float32).reshape(-1)
    f = x[np.isfinite(x)].astype(np.float64)
    if f.size == 0:
        return np.array([0.0, np.nan, np.nan, np.nan, np.nan])
    s = 0.0
    for v in f.tolist():  # index order
        s += v
    return np.array([float(f.size), float(np.median(f)), s / f.size, f.min(), f.max()])


FIELDS = ("count", "median", "mean", "min", "max")


def summary(x):
    r = summary_array(x)
    return {"count": int(r[0]), **{k: float(v) for k, v in zip(FIELDS[1:], r[1:])}}


def moments(x):
    x = np.asarray(x, np.float32).astype(np.float64)
    return x.mean(axis=0), np.atleast_2d(np.cov(x, rowvar=False))


def frechet_parts(mean_a, cov_a, mean_b, cov_b):
    """[distance, |dmu|^2, tr a + tr b, sum sqrt(eig)] by numpy.linalg.eigh."""
    lam, V = np.linalg.eigh(0.5 * (cov_a + cov_a.T))
    S = (V * np.sqrt(np.maximum(lam, 0.0))) @ V.T
    M = S @ cov_b @ S
    mu = np.linalg.eigvalsh(0.5 * (M + M.T))
    rt = float(np.sqrt(np.maximum(mu, 0.0)).sum())
    dm = float(((mean_a - mean_b) ** 2).sum())
    tr = float(np.trace(cov_a) + np.trace(cov_b))
    return np.array([dm + tr - 2.0 * rt, dm, tr, rt])


def frechet(a, b):
    return float(frechet_parts(*moments(a), *moments(b))[0])


def frechet_sqrtm(a, b):
    """The same distance as tr(sqrtm(cov_a cov_b)) (scipy)."""
    from scipy.linalg import sqrtm
    (ma, ca), (mb, cb) = moments(a), moments(b)
    root = sqrtm(ca @ cb)
    return float(((ma - mb) ** 2).sum() + np.trace(ca) + np.trace(cb) - 2.0 * np.trace(root).real)


def centroids(dvecs, seg_start):
    """Per-segment mean row scaled to unit length, float32."""
    x = np.asarray(dvecs, np.float32).astype(np.float64)
    out = []
    for lo, hi in zip(seg_start[:-1], seg_start[1:]):
        m = x[lo:hi].mean(axis=0)
        out.append(m / np.linalg.norm(m))
    return np.asarray(out, np.float32).reshape(len(seg_start) - 1, x.shape[1])


def attribute_vote(points, ref_points, ref_labels, k=5):
    _, idx = nearest(points, ref_points, k)
    lab = np.asarray(ref_labels)
    return np.array([np.mean(lab[r[r >= 0]] == 1) if (r >= 0).any() else np.nan for r in idx])


class Ops:
    """The device operations ``speaker_eval.table`` needs, on CPU tensors through numpy."""

    @staticmethod
    def _t(x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x))

    @staticmethod
    def _n(x):
        return None if x is None else x.detach().cpu().numpy()

    @classmethod
    def nearest(cls, a, b, k=1, group_a=None, group_b=None, same=False):
        d, i = nearest(cls._n(a), cls._n(b), k, cls._n(group_a), cls._n(group_b), same)
        return cls._t(d), cls._t(i)

    @classmethod
    def summary(cls, x):
        return summary(cls._n(x))

    @classmethod
    def centroids(cls, dvecs, seg_start):
        return cls._t(centroids(cls._n(dvecs), [int(s) for s in seg_start]))

    @classmethod
    def frechet(cls, a, b):
        return frechet(cls._n(a), cls._n(b))
