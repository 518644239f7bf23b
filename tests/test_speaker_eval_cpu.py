"""Generated-speaker metrics without a GPU: the numpy oracle against scipy, the bookkeeping of
``speaker_eval.table`` on hand-made points, and the host-side argument checks of the entry points.
"""
import importlib

import numpy as np
import pytest
import torch

import speaker_eval_oracle as O

PKG = "mid-attribute-speaker-generation_amd"
NEW = ("fs2_cosine_nn", "fs2_cosine_nn_ws_bytes", "fs2_finite_summary",
       "fs2_finite_summary_ws_bytes", "fs2_gauss_moments", "fs2_frechet")


def _unit(rng, n, d):
    x = rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def test_oracle_distances_against_scipy():
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(0)
    for na, nb, d in ((37, 101, 64), (5, 300, 255), (20, 20, 1)):
        a, b = _unit(rng, na, d), 3.0 * _unit(rng, nb, d)  # b is not of unit length
        got = O.cosine_dist(a, b)
        want = cdist(a.astype(np.float64), b.astype(np.float64), "cosine")
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"({na}, {nb}, {d}): oracle against cdist {err:.2e}")
        # only the float32 rounding of a value in [0, 2] can differ: half an ulp of 2 is 2^-23
        assert got.dtype == np.float32 and err <= 2.0 ** -22
    z = np.zeros((1, 4), np.float32)
    assert O.cosine_dist(z, _unit(rng, 3, 4)).tolist() == [[1.0, 1.0, 1.0]]


def test_oracle_nearest_ties_and_groups():
    b = np.array([[1, 0], [0, 1], [2, 0], [-1, 0]], np.float32)
    a = np.array([[1, 0]], np.float32)
    d, i = O.nearest(a, b, 3)
    assert i.tolist() == [[0, 2, 1]] and d.tolist() == [[0.0, 0.0, 1.0]]  # the tie: lower index
    d, i = O.nearest(a, b, 2, np.array([7]), np.array([7, 1, 1, 7]))
    assert i.tolist() == [[2, 1]]
    d, i = O.nearest(a, b, 3, np.array([7]), np.array([7, 1, 1, 7]), same=True)
    assert i.tolist() == [[0, 3, -1]] and d[0, 2] == np.inf and d[0, 1] == 2.0
    d, i = O.nearest(a, b[:0], 2)
    assert i.tolist() == [[-1, -1]] and np.isinf(d).all()


def test_oracle_summary():
    x = np.array([3.0, np.inf, 1.0, np.nan, 2.0, -np.inf, 10.0], np.float32)
    assert O.summary(x) == {"count": 4, "median": 2.5, "mean": 4.0, "min": 1.0, "max": 10.0}
    r = O.summary(np.array([np.nan, np.inf], np.float32))
    assert r["count"] == 0 and all(np.isnan(r[k]) for k in O.FIELDS[1:])


def _sets(rng, na, nb, d):
    a = (rng.standard_normal((na, d)) / np.sqrt(d)).astype(np.float32)
    b = (rng.standard_normal((nb, d)) * 1.3 / np.sqrt(d) + 0.05).astype(np.float32)
    return a, b


FULL_RANK = ((200, 300, 64), (50, 50, 8), (30, 40, 1))


def test_oracle_frechet_against_sqrtm():
    rng = np.random.default_rng(1)
    for na, nb, d in FULL_RANK:
        a, b = _sets(rng, na, nb, d)
        for x, y in ((a, b), (a, a)):
            parts = O.frechet_parts(*O.moments(x), *O.moments(y))
            scale = parts[1] + parts[2]
            got, want = O.frechet(x, y), O.frechet_sqrtm(x, y)
            print(f"({na}, {nb}, {d}) eigh {got:.17g} sqrtm {want:.17g} diff {abs(got - want):.2e} "
                  f"scale {scale:.3g}")
            # the bound the device result is held to as well: D eps for the backward error of
            # either eigensolver, D for summing D square roots
            tol = d * d * 2.0 ** -52 * scale
            assert abs(got - want) <= tol
            if x is y:
                assert abs(got) <= tol  # a set against itself: 0 up to that rounding


# ------------------------------------------------------------------ the table on hand-made points
def _set(SE, speakers):
    rows = [r for s in speakers for r in s]
    seg = np.concatenate([[0], np.cumsum([len(s) for s in speakers])])
    return SE.SpeakerSet(torch.tensor(rows, dtype=torch.float32), seg.tolist())


def _rec(values):
    v = np.asarray(values, np.float64)
    return {"count": len(v), "median": float(np.median(v)), "mean": float(v.mean()),
            "min": float(v.min()), "max": float(v.max())}


def _same(got, want):
    assert got["count"] == want["count"]
    for k in O.FIELDS[1:]:
        assert got[k] == pytest.approx(want[k], abs=1e-6), (k, got, want)


def test_table_bookkeeping():
    SE = importlib.import_module(PKG + ".speaker_eval")
    # unit vectors (0.6, 0.8 are 3-4-5 legs): every cosine distance below is 1 - a dot product
    train = _set(SE, [[(1, 0), (1, 0)],            # T0 at (1, 0)
                      [(0.6, 0.8), (-0.6, 0.8)],   # T1: mean (0, 0.8) -> (0, 1); each row 0.2 off
                      [(-1, 0)]])                  # T2 at (-1, 0)
    gen = _set(SE, [[(0.8, 0.6)],                  # G0: T0 0.2, T1 0.4, T2 1.8
                    [(0, -1), (0, -2)]])           # G1: T0 1, T1 2, T2 1 (the tie goes to T0)
    truth = _set(SE, [[(1, 0)], [(0.8, 0.6)], [(-1, 0)]])
    t = SE.table(O.Ops, train, gen, truth)
    _same(t["t2t"], _rec([1, 1, 1]))               # T0-T1 1, T0-T2 2, T1-T2 1
    _same(t["g2g"], _rec([1.6, 1.6]))              # 1 - (0.8, 0.6) . (0, -1)
    _same(t["g2t"], _rec([0.2, 1]))
    _same(t["t2g"], _rec([0.2, 0.4, 1]))
    _same(t["t_within"], _rec([0, 0, 0.2, 0.2, 0]))
    _same(t["g_within"], _rec([0, 0, 0]))
    _same(t["s2s"], _rec([0.2, 0.2, 1.8]))         # S0-S1 0.2, S0-S2 2, S1-S2 1.8
    _same(t["s2t"], _rec([0, 0.2, 0]))             # S1 is nearest to T0
    _same(t["s2t_same"], _rec([0, 0.4, 0]))        # ... and 0.4 from its own T1
    tr, ge = train.dvecs.numpy(), gen.dvecs.numpy()
    assert t["fd_g_t"] == O.frechet(ge, tr)
    assert t["fd_t_t"] == O.frechet(tr[[0, 1, 4]], tr[[2, 3]])  # speakers 0 and 2 against 1
    assert set(SE.table(O.Ops, train, gen)) == {"t2t", "g2g", "g2t", "t2g", "t_within", "g_within",
                                                "fd_g_t", "fd_t_t"}
    # one speaker: no other to be near, and too few rows for a covariance
    one = _set(SE, [[(1, 0)]])
    t1 = SE.table(O.Ops, one, one)
    assert t1["t2t"]["count"] == 0 and np.isnan(t1["t2t"]["median"])
    assert np.isnan(t1["fd_g_t"]) and np.isnan(t1["fd_t_t"]) and t1["g2t"]["max"] == 0.0
    with pytest.raises(ValueError):
        SE.SpeakerSet(torch.zeros(3, 2), [0, 2])
    with pytest.raises(ValueError):
        SE.table(O.Ops, train, gen, gen)           # truth must list the training speakers


def test_attribute_vote_oracle():
    ref = np.array([[1, 0], [0.9, 0.1], [0, 1], [0.1, 0.9], [-1, 0]], np.float32)
    labels = [1, 1, 0, 0, 0]
    pts = np.array([[1, 0.05], [0, 1], [1, 1]], np.float32)
    v = O.attribute_vote(pts, ref, labels, k=2)
    assert v[:2].tolist() == [1.0, 0.0] and v[2] == 0.5


def test_speaker_labels(tmp_path):
    import json
    SE = importlib.import_module(PKG + ".speaker_eval")
    meta = {"gender": {"M": 0, "F": 1}, "language": {"ja": 0, "en": 1}}
    (tmp_path / "speakers.json").write_text(json.dumps(
        {"a": [1, "F", "ja"], "b": [0, "M", "en"], "c": [2, "F", "en"]}))
    assert SE.speaker_labels(str(tmp_path), meta, "gender") == [0, 1, 1]
    assert SE.speaker_labels(str(tmp_path), meta, "language") == [1, 0, 1]
    (tmp_path / "speakers.json").write_text(json.dumps({"a": 0}))
    with pytest.raises(ValueError):
        SE.speaker_labels(str(tmp_path), meta, "gender")


# ------------------------------------------------------------------ the entry points, host side
def test_symbols_and_argument_checks():
    L = importlib.import_module(PKG + "._lib")
    assert set(NEW) <= set(L.lib.symbols())
    L.lib.load()
    lib, p, big = L.lib, 16, 1 << 40  # p: a non-null placeholder, never dereferenced

    def raises(call, word):
        with pytest.raises(L.KernelError) as e:
            call()
        assert word in str(e.value), str(e.value)

    # cosine_nn(a, b, na, nb, dim, k, group_a, group_b, mode, dist, index, ws, ws_bytes, stream)
    raises(lambda: lib.fs2_cosine_nn(p, p, 4, 4, 0, 1, None, None, 0, p, p, p, big, 0), "dim")
    raises(lambda: lib.fs2_cosine_nn(p, p, 4, 4, 257, 1, None, None, 0, p, p, p, big, 0), "dim")
    raises(lambda: lib.fs2_cosine_nn(p, p, 4, 4, 64, 0, None, None, 0, p, p, p, big, 0), "k ")
    raises(lambda: lib.fs2_cosine_nn(p, p, 4, 4, 64, 17, None, None, 0, p, p, p, big, 0), "k ")
    raises(lambda: lib.fs2_cosine_nn(p, p, 4, 4, 64, 1, None, None, 2, p, p, p, big, 0), "mode")
    raises(lambda: lib.fs2_cosine_nn(p, p, 4, 4, 64, 1, p, None, 0, p, p, p, big, 0), "pair")
    raises(lambda: lib.fs2_cosine_nn(p, p, -1, 4, 64, 1, None, None, 0, p, p, p, big, 0), "na")
    raises(lambda: lib.fs2_cosine_nn(None, p, 4, 4, 64, 1, None, None, 0, p, p, p, big, 0),
           "missing")
    need = lib.fs2_cosine_nn_ws_bytes(4, 5000, 3)
    assert need == 5 * 4 * 3 * 8 and lib.fs2_cosine_nn_ws_bytes(4, 1024, 3) == 0
    raises(lambda: lib.fs2_cosine_nn(p, p, 4, 5000, 64, 3, None, None, 0, p, p, p, need - 1, 0),
           "workspace")
    assert lib.fs2_cosine_nn(None, None, 0, 4, 64, 1, None, None, 0, None, None, None, 0, 0) == 0

    assert lib.fs2_finite_summary_ws_bytes(1000) == 4000
    raises(lambda: lib.fs2_finite_summary(p, (1 << 20) + 1, p, p, big, 0), "n ")
    raises(lambda: lib.fs2_finite_summary(p, 8, p, p, 31, 0), "workspace")
    raises(lambda: lib.fs2_finite_summary(p, 8, None, p, big, 0), "missing")

    raises(lambda: lib.fs2_gauss_moments(p, 1, 8, p, p, 0), "at least 2")
    raises(lambda: lib.fs2_gauss_moments(p, 10, 65, p, p, 0), "dim")
    raises(lambda: lib.fs2_gauss_moments(p, 10, 8, None, p, 0), "missing")

    raises(lambda: lib.fs2_frechet(p, p, p, p, 1, 65, p, 0), "dim")
    raises(lambda: lib.fs2_frechet(p, p, p, p, 1, 0, p, 0), "dim")
    raises(lambda: lib.fs2_frechet(p, p, None, p, 1, 8, p, 0), "missing")
    assert lib.fs2_frechet(None, None, None, None, 0, 8, None, 0) == 0


def test_wrappers_raise_off_the_gpu():
    K = importlib.import_module(PKG + ".kernels")
    x = torch.zeros(4, 8)
    for call in (lambda: K.cosine_nn(x, x), lambda: K.finite_summary(x),
                 lambda: K.gauss_moments(x),
                 lambda: K.frechet(x[0].double(), torch.eye(8).double(), x[0].double(),
                                   torch.eye(8).double())):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
