"""Exact t-SNE on the GPU (csrc/tsne.hip, embedding_map.py) against the numpy oracle
(tsne_oracle.py, itself checked against scikit-learn in test_tsne_cpu.py) and fixture g17.

Tolerances of the fp32 descent (KL, one step, the short run) follow one rule: the fixture records
how far the same computation in numpy float32 lies from float64 (max error over max magnitude);
the kernels may deviate up to 8 times that, for their different summation order and reciprocal.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from conftest import load_golden
import tsne_oracle as O

NAME = "mid-attribute-speaker-generation_amd"
pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# n_per, groups, D, seed, perplexity: a, b, c are the fixture's sets
SETS = {"a": (35, 2, 3, 1, 5.0), "b": (32, 3, 64, 2, 10.0), "c": (80, 3, 256, 3, 50.0),
        "d": (65, 2, 64, 5, 30.0), "two": (48, 2, 64, 4, 10.0), "wide": (20, 3, 300, 6, 10.0),
        "dmax": (14, 3, 1024, 7, 10.0), "nmax": (1024, 4, 8, 8, 50.0)}


def _mod(name):
    return importlib.import_module(f"{NAME}.{name}")


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def points(name):
    n_per, groups, D, seed, _ = SETS[name]
    x = O.make_points(n_per, groups, D, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle_p(name):
    P, beta, ent = O.joint_probabilities(points(name), SETS[name][4])
    P.setflags(write=False)
    return P, beta, ent


def tsne(name, **kw):
    return _mod("embedding_map").TSNE(perplexity=SETS[name][4], **kw)


def rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


# ------------------------------------------------------------------ 1. points
def test_points_are_capped_segment_means():
    K = _mod("kernels")
    rng = np.random.default_rng(0)
    counts, cap, D = [3, 4, 7, 1, 12], 4, 300  # shorter than, equal to and longer than the cap
    x = rng.standard_normal((sum(counts), D)).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    got = _np(K.tsne_points(_dev(x), _dev(seg, np.int64), cap))
    for s, c in enumerate(counts):
        rows = x[seg[s]:seg[s] + min(c, cap)].astype(np.float64)
        n = len(rows)
        tol = n * U * np.abs(rows).sum(0) / n  # a few ulp of the sum, carried to the mean
        assert (np.abs(got[s] - rows.mean(0)) <= tol).all(), s


# ------------------------------------------------------------------ 2. PCA initialisation
@pytest.mark.parametrize("name", ["b", "wide", "dmax"])
def test_pca_init_equals_the_svd(name):
    want, S = O.pca_init(points(name))
    assert (S[2] / S[1]) ** 2 <= 0.9  # a clear gap after the second component
    got = _np(tsne(name).pca_init(_dev(points(name))))
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"pca {name}: singular values {S[:4]}, max err / max {err:.2e}")
    assert err <= 1e-6


@pytest.mark.parametrize("name", ["two", "a"])
def test_pca_init_with_a_nearly_degenerate_second_component(name):
    """Two groups: one dominant component, the second and third close.  Asked: the first column
    matches, the columns are uncorrelated (1e-5: their fp32 rounding is 6e-8 per element), and
    the call returns."""
    want, S = O.pca_init(points(name))
    got = _np(tsne(name).pca_init(_dev(points(name)))).astype(np.float64)
    err = np.abs(got[:, 0] - want[:, 0]).max() / np.abs(want[:, 0]).max()
    corr = np.corrcoef(got[:, 0], got[:, 1])[0, 1]
    print(f"pca {name}: singular values {S[:4]}, first column err {err:.2e}, corr {corr:.2e}")
    assert np.isfinite(got).all() and err <= 1e-6 and abs(corr) <= 1e-5


# ------------------------------------------------------------------ 3. affinities
@pytest.mark.parametrize("name", ["a", "d", "b"])
def test_affinities_equal_the_oracle(name):
    perp = SETS[name][4]
    want, beta, _ = oracle_p(name)
    P, got_beta, P64 = (_np(t) for t in tsne(name).affinities(_dev(points(name)), want64=True))
    n = len(want)
    np.testing.assert_allclose(got_beta, beta, rtol=1e-12)
    big = want > 1e-6 * want.max(1, keepdims=True)
    worst = np.abs(P64[big] / want[big] - 1).max()
    print(f"affinities {name}: max rel err {worst:.2e} over {big.sum()} of {n * n} entries")
    assert worst <= 1e-9
    # the rows' entropies at the kernel's beta
    d = O.sq_distances(points(name)).astype(np.float64)
    p = np.exp(-d * got_beta[:, None])
    np.fill_diagonal(p, 0.0)
    s = p.sum(1)
    ent = np.log(s) + got_beta * (d * p).sum(1) / s
    assert np.abs(ent - np.log(perp)).max() <= 1e-5 + 1e-9
    assert (P64 == P64.T).all() and abs(P64.sum() - 1.0) <= 1e-6 and (np.diag(P64) == 0).all()
    assert (P == P64.astype(np.float32)).all()


def test_the_largest_problem():
    """N = 4096, the limit: a whole row of distances in LDS, 16 per thread in the search, 64 per
    lane in the descent.  The oracle's search is too slow here, so the properties are checked:
    every row's entropy at the kernel's beta, symmetry, the sum, and a short finite descent."""
    X, perp = points("nmax"), SETS["nmax"][4]
    assert X.shape == (4096, 8)
    t = tsne("nmax", exploration_iter=1, max_iter=2)
    P, beta, P64 = t.affinities(_dev(X), want64=True)
    beta = _np(beta)
    d = np.zeros((4096, 4096))
    for k in range(X.shape[1]):  # the direct form, one coordinate at a time
        d += np.subtract.outer(X[:, k].astype(np.float64), X[:, k].astype(np.float64)) ** 2
    d = d.astype(np.float32).astype(np.float64)
    p = np.exp(-d * beta[:, None])
    np.fill_diagonal(p, 0.0)
    s = p.sum(1)
    ent = np.log(s) + beta * (d * p).sum(1) / s
    assert np.abs(ent - np.log(perp)).max() <= 1e-5 + 1e-9
    assert torch.equal(P64, P64.T) and abs(P64.sum().item() - 1.0) <= 1e-6
    assert torch.equal(P, P64.float()) and (P64.diagonal() == 0).all()
    Y = t.fit_transform(_dev(X))
    assert t.n_iter_ == 1 and t.stage2_start_ == 1 and np.isfinite(t.kl_divergence_)
    assert torch.isfinite(Y).all() and 0 < t.kl(Y, P) < np.inf


# ------------------------------------------------------------------ 4. the objective
@pytest.mark.parametrize("name", ["a", "b"])
def test_kl_equals_the_oracle(name):
    g = load_golden("g17_tsne.npz")
    Y, P = g[f"{name}_Y"].astype(np.float32), g[f"{name}_P"]
    want, _ = O.kl_grad(Y, P)
    got = tsne(name).kl(_dev(Y), _dev(P))
    dev32 = float(g[f"{name}_kl_dev32"])
    print(f"kl {name}: {got!r} against {want!r}, rel {abs(got - want) / want:.2e}, "
          f"numpy float32 {dev32:.2e}")
    assert abs(got - want) <= 8 * dev32 * abs(want)


# ------------------------------------------------------------------ 5. one step
def test_one_step_from_the_recorded_state():
    g = load_golden("g17_tsne.npz")
    P, _, _ = oracle_p("b")
    lr = O.auto_lr(len(P))
    state = [g[f"b_state_{k}"] for k in ("Y", "update", "gains")]
    Y1, upd1, gains1, kl, gn, ug = O.step(*state, P, 12.0, 0.5, lr)
    Y, upd, gains = (_dev(a) for a in state)
    got_Y, got_kl, got_gn = tsne("b").step(Y, upd, gains, _dev(P), 12.0, 0.5)
    dY, dU, dKL, dGN = g["b_step_dev32"]
    fig = (rel(_np(got_Y), Y1), rel(_np(upd), upd1), abs(got_kl.item() - kl) / kl,
           abs(got_gn.item() - gn) / gn)
    print("step: Y' {:.2e} update' {:.2e} kl {:.2e} norm {:.2e}; numpy float32 {}".format(
        *fig, g["b_step_dev32"]))
    assert fig[0] <= 8 * dY and fig[1] <= 8 * dU and fig[2] <= 8 * dKL and fig[3] <= 8 * dGN
    sure = np.abs(ug) >= 1e-6 * np.abs(ug).max()  # elsewhere the sign of update * grad is noise
    assert (~sure).mean() <= 0.01
    # the oracle's float64 decisions, applied to the float32 gains in float32 as the kernel does
    g32 = state[2].astype(np.float32)
    want_gains = np.maximum(np.where(ug < 0, g32 + np.float32(0.2), g32 * np.float32(0.8)),
                            np.float32(0.01))
    assert want_gains.dtype == np.float32 and np.abs(want_gains - gains1).max() <= 4 * U * gains1.max()
    assert (_np(gains)[sure] == want_gains[sure]).all()


# ------------------------------------------------------------------ 6. short runs, every switch
def test_short_run_with_every_switch():
    """20 iterations, 10 of them exaggerated, from the PCA initialisation: both stages, the
    reset of update and gains, both last-iteration evaluations, the record read once."""
    g = load_golden("g17_tsne.npz")
    P, _, _ = oracle_p("b")
    Y0, _ = O.pca_init(points("b"))
    kw = dict(exploration_iter=10, max_iter=20)
    want_Y, want_kl, want_it = O.run(Y0, P, O.auto_lr(len(P)), **kw)
    t = tsne("b", **kw)
    Y = _np(t.fit_transform(_dev(points("b"))))
    dY, dKL = g["b_short_dev32"]
    print(f"short run: Y {rel(Y, want_Y):.2e} kl {abs(t.kl_divergence_ - want_kl) / want_kl:.2e}; "
          f"numpy float32 {dY:.2e} {dKL:.2e}")
    assert t.n_iter_ == want_it == 19 and t.stage2_start_ == 10
    assert rel(Y, want_Y) <= 8 * dY
    assert abs(t.kl_divergence_ - want_kl) <= 8 * dKL * want_kl


def test_norm_stop_ends_stage_one_at_its_first_check():
    """min_grad_norm = 1e3 ends stage 1 at iteration 49, so stage 2 runs from 50 and, with
    max_iter = 60, to 59: n_iter_ is 59 as the oracle's and scikit-learn's rules give it (49 is
    stage 1's last iteration).  After 60 iterations numpy float32 itself lies 1.5 (Y) and 0.24
    (KL) from float64 -- the descent amplifies rounding by about 1.5 per iteration -- so on this
    run the 8x rule bounds the coordinates only loosely; the switches are what it checks."""
    g = load_golden("g17_tsne.npz")
    P, _, _ = oracle_p("b")
    Y0, _ = O.pca_init(points("b"))
    kw = dict(max_iter=60, min_grad_norm=1e3)
    want_Y, want_kl, want_it = O.run(Y0, P, O.auto_lr(len(P)), **kw)
    t = tsne("b", **kw)
    Y = _np(t.fit_transform(_dev(points("b"))))
    dY, dKL = g["b_norm_dev32"]
    print(f"norm run: Y {rel(Y, want_Y):.2e} kl {abs(t.kl_divergence_ - want_kl) / want_kl:.2e}; "
          f"numpy float32 {dY:.2e} {dKL:.2e}")
    assert t.stage2_start_ == 50 and t.n_iter_ == want_it == int(g["b_norm_n_iter"]) == 59
    assert np.isfinite(Y).all() and rel(Y, want_Y) <= 8 * dY
    assert abs(t.kl_divergence_ - want_kl) <= 8 * dKL * want_kl


# ------------------------------------------------------------------ 7. full fits
@pytest.mark.parametrize("name", ["b", "c"])
def test_full_fit_reaches_the_recorded_objective(name):
    """The KL of the returned map, recomputed under the oracle's P in float64, is at most the
    largest recorded KL (scikit-learn at four seeds, the oracle in float32, float64 and from six
    perturbed starts) plus one spread of that set; two calls agree bitwise."""
    recorded = load_golden("g17_tsne.npz")[f"{name}_final_kl"]
    P, _, _ = oracle_p(name)
    X = _dev(points(name))
    t = tsne(name)
    Y = t.fit_transform(X).clone()
    kl, _ = O.kl_grad(_np(Y), P)
    print(f"full fit {name}: KL {kl:.4f} (reported {t.kl_divergence_:.4f}, n_iter {t.n_iter_}); "
          f"recorded {recorded.min():.4f} .. {recorded.max():.4f}")
    assert np.isfinite(_np(Y)).all() and t.n_iter_ <= 999
    assert kl <= recorded.max() + (recorded.max() - recorded.min())
    assert torch.equal(tsne(name).fit_transform(X), Y)


def _fake_speakers(n, per, seed=0):
    """{file name: (per, 64) embeddings} of n speakers, alternating jp / en, around two centres."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((2, 64))
    out = {}
    for k in range(n):
        lang = ("jp", "en")[k % 2]
        e = centres[k % 2] + 0.4 * rng.standard_normal((1, 64)) + \
            0.1 * rng.standard_normal((per, 64))
        out[f"corpus_s{k:03d}_m_{lang}.npy"] = _dev(e)
    return out


def test_speaker_map_coordinates_fill_the_unit_square():
    import random
    m = _mod("embedding_map").speaker_map(_fake_speakers(70, 3), emb_per_spkr=2, perplexity=10,
                                          rng=random.Random(0), exploration_iter=10, max_iter=20)
    c = _np(m["coords"])
    assert c.shape == (70, 2) and (c >= 0).all() and (c <= 1).all()
    assert (c.min(0) == 0).all() and (c.max(0) == 1).all()
    assert m["n_iter"] == 19 and np.isfinite(m["kl"])
    assert sorted(m["names"]) == sorted(_fake_speakers(70, 3))


# ------------------------------------------------------------------ 8. the trainer's method
def test_trainer_visualize_embeddings(tmp_path):
    import random
    embedder = _mod("ge2e").SpeechEmbedder(device="cuda", weight_grads=True)
    trainer = _mod("embedder_train").EmbedderTrainer(embedder, _mod("ge2e").GE2ELoss("cuda"))
    spk = _fake_speakers(12, 5)
    kw = dict(perplexity=3, rng=random.Random(0))
    m = trainer.visualize_embeddings(spk, **kw)
    assert m["lang2code"] == {"en": 0, "jp": 1} and len(m["names"]) == 12
    assert m["codes"] == [m["lang2code"][n[:-4].split("_")[3]] for n in m["names"]]
    assert _np(m["coords"]).shape == (12, 2)
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return  # no figure without matplotlib; everything else above has run
    path = tmp_path / "map.png"
    trainer.visualize_embeddings(spk, path=str(path), **kw)
    assert path.stat().st_size > 0
