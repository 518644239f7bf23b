"""Exact t-SNE, the parts that need no GPU: the numpy oracle against scikit-learn's own joint
probabilities, objective and gradient (fixture g17, written by scripts/make_golden_tsne.py), the
speaker selection of visualize_embeddings against a transcription, the oracle's control rules
against scripted error and norm sequences, and the argument checks of the new entries."""
import importlib
import random
import sys

import numpy as np
import pytest

from conftest import load_golden
import tsne_oracle as O

PKG = "mid-attribute-speaker-generation_amd"
NEW = ("fs2_tsne_points", "fs2_tsne_pca_ws_bytes", "fs2_tsne_pca_init",
       "fs2_tsne_affinities_ws_bytes", "fs2_tsne_affinities", "fs2_tsne_state_init",
       "fs2_tsne_rowsum", "fs2_tsne_update", "fs2_tsne_control", "fs2_tsne_step", "fs2_tsne_kl",
       "fs2_tsne_finish")
SETS = {"a": (35, 2, 3, 1, 5.0), "b": (32, 3, 64, 2, 10.0)}  # n_per, groups, D, seed, perplexity


@pytest.mark.parametrize("name", sorted(SETS))
def test_oracle_equals_sklearn(name):
    g = load_golden("g17_tsne.npz")
    n_per, groups, D, seed, perp = SETS[name]
    P, _, ent = O.joint_probabilities(O.make_points(n_per, groups, D, seed), perp)
    np.testing.assert_allclose(P, g[f"{name}_P"], rtol=1e-12, atol=0)
    assert np.abs(ent - np.log(perp)).max() <= 1e-5 + 1e-9
    kl, grad = O.kl_grad(g[f"{name}_Y"], g[f"{name}_P"])
    np.testing.assert_allclose(kl, g[f"{name}_kl"], rtol=1e-12)
    np.testing.assert_allclose(grad, g[f"{name}_grad"], rtol=1e-12,
                               atol=1e-12 * np.abs(g[f"{name}_grad"]).max())


def test_select_speakers_is_the_reference_selection():
    M = importlib.import_module(PKG + ".embedding_map")
    names = [f"jvs_s{k:02d}_m_jp.npy" for k in range(5)] + \
            [f"vctk_p{k:02d}_f_en.npy" for k in range(3)] + \
            ["x/jvs_s77_f_jp.npy", "aishell_a01_m_zh.npy", "vctk_p09_m_en.npy"]
    got = M.select_speakers(names, "language", 4, random.Random(0))

    rng = random.Random(0)  # train_speech_embedder.py:336-355, written out
    lang2indices = {}
    for index, name in enumerate(names):
        lang = name.split("/")[-1][:-4].split("_")[3]
        if lang not in lang2indices:
            lang2indices[lang] = []
        lang2indices[lang].append(index)
    for lang, v in lang2indices.items():
        lang2indices[lang] = rng.sample(v, min(4, len(v)))
    langs = []
    for lang, idx in lang2indices.items():
        langs.extend([lang] * len(idx))
    lang2code = {k: i for i, k in enumerate(sorted(set(langs)))}
    indices = [i for item in lang2indices.items() for i in item[1]]

    assert got == (indices, langs, lang2code)
    assert list(lang2indices) == ["jp", "en", "zh"] and lang2code == {"en": 0, "jp": 1, "zh": 2}
    assert len(indices) == 4 + 4 + 1  # jp has 6 > 4 speakers, en exactly 4, zh appears late
    two = M.select_speakers(names[:8], "language", 300, random.Random(1))
    assert sorted(two[0]) == list(range(8)) and two[2] == {"en": 0, "jp": 1}
    assert M.select_speakers(names, "gender", 300, random.Random(2))[2] == {"f": 0, "m": 1}


def _drive(errors, norms, **kw):
    """The oracle's record driven over scripted (error, norm) per iteration: the events."""
    c = O.Control(**kw)
    events = []
    for i in range(max(c.max_iter, c.exploration_iter)):
        stage, evaluate = c.stage, c.begin(i)[2]
        c.end(i, errors(i), norms(i))
        if evaluate:
            events.append(("eval", i))
        if c.stage != stage:
            events.append(("stage2", c.start))
        if c.done:
            events.append(("done", i))
            break
    return c, events


def _expected(errors, norms, max_iter, explore, window2, min_norm):
    """_gradient_descent twice, as TSNE._tsne calls it: ten lines of Python."""
    def descent(it, last, window):
        best, best_iter, error, i = np.finfo(float).max, it, None, it
        for i in range(it, last):
            if (i + 1) % 50 == 0 or i == last - 1:
                error = errors(i)
            if (i + 1) % 50 == 0:
                if error < best:
                    best, best_iter = error, i
                elif i - best_iter > window:
                    break
                if norms(i) <= min_norm:
                    break
        return error, i
    _, it = descent(0, explore, explore)
    error, n_iter = descent(it + 1, max_iter, window2)
    return it + 1, error, n_iter


CASES = {
    # stage 1 runs out, stage 2 makes a new best at every check and runs out at max_iter - 1
    "full": (lambda i: 5.0 - 1e-3 * i, lambda i: 1.0, 1000, 250, 300, 1e-7),
    # no progress after iteration 349: stage 2 stops at the first check past the window
    "no_progress": (lambda i: 5.0 - 1e-3 * min(i, 349), lambda i: 1.0, 1000, 250, 100, 1e-7),
    # the norm ends stage 1 at its first check and stage 2 at its first check
    "norm": (lambda i: 5.0 - 1e-3 * i, lambda i: 1e-9, 1000, 250, 300, 1e-7),
    # an exploration that is no multiple of 50 and a last iteration that is no check
    "odd": (lambda i: 5.0 - 1e-3 * i, lambda i: 1.0, 133, 70, 300, 1e-7),
    # no progress inside stage 1: the window there is exploration_iter
    "stage1_window": (lambda i: 5.0 + 1e-3 * i, lambda i: 1.0, 400, 120, 300, 1e-7),
    # max_iter below the exploration: the norm ends stage 1 at 49, stage 2 runs from 50 to 59
    "short_max": (lambda i: 5.0 - 1e-3 * i, lambda i: 1e-9, 60, 250, 300, 1e-7),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_control_rules(case):
    errors, norms, max_iter, explore, window2, min_norm = CASES[case]
    c, events = _drive(errors, norms, max_iter=max_iter, exploration_iter=explore,
                       n_iter_without_progress=window2, min_grad_norm=min_norm)
    start, error, n_iter = _expected(errors, norms, max_iter, explore, window2, min_norm)
    assert (c.start, c.error, c.n_iter, c.done) == (start, error, n_iter, True)
    assert ("stage2", start) in events and events[-1] == ("done", n_iter)
    where = {"full": (250, 999), "no_progress": (250, 499), "norm": (50, 99), "odd": (70, 132),
             "stage1_window": (120, 399), "short_max": (50, 59)}[case]
    assert (start, n_iter) == where
    if case == "full":
        assert (c.best_iter, c.best) == (999, errors(999))  # a new best at every check
        assert [i for k, i in events if k == "eval"] == list(range(49, 1000, 50))
    if case == "odd":  # evaluated at both stages' last iterations although neither is a check
        assert [i for k, i in events if k == "eval"] == [49, 69, 99, 132]
    if case == "no_progress":  # best at 349; 449 - 349 = 100 is inside the window, 499 is past
        assert c.best_iter == 349
    if case == "stage1_window":  # the error only rises: 99 - 49 <= 120 keeps stage 1 going, and
        assert c.best_iter == 149  # stage 2's best is its first check, 399 - 149 <= 300


def test_entries_validate_arguments_before_any_launch():
    L = importlib.import_module(PKG + "._lib")
    assert set(NEW) <= set(L.lib.symbols())
    lib, p, big = L.lib, 16, 1 << 40  # p: a non-null placeholder, never dereferenced
    assert lib.fs2_abi_version() == 1
    bad = [
        lambda: lib.fs2_tsne_points(p, p, 4, 1025, 400, p, 0),
        lambda: lib.fs2_tsne_points(p, p, 4, 64, 0, p, 0),
        lambda: lib.fs2_tsne_points(None, p, 4, 64, 400, p, 0),
        lambda: lib.fs2_tsne_pca_init(p, 4097, 64, p, p, big, 0),
        lambda: lib.fs2_tsne_pca_init(p, 96, 1025, p, p, big, 0),
        lambda: lib.fs2_tsne_pca_init(p, 96, 64, None, p, big, 0),
        lambda: lib.fs2_tsne_pca_init(p, 96, 64, p, p, lib.fs2_tsne_pca_ws_bytes(96, 64) - 8, 0),
        lambda: lib.fs2_tsne_affinities(p, 4097, 64, 50.0, p, None, None, p, big, 0),
        lambda: lib.fs2_tsne_affinities(p, 96, 1025, 50.0, p, None, None, p, big, 0),
        lambda: lib.fs2_tsne_affinities(p, 96, 0, 50.0, p, None, None, p, big, 0),
        lambda: lib.fs2_tsne_affinities(p, 50, 64, 50.0, p, None, None, p, big, 0),
        lambda: lib.fs2_tsne_affinities(p, 30, 64, 50.0, p, None, None, p, big, 0),
        lambda: lib.fs2_tsne_affinities(p, 96, 64, 10.0, None, None, None, p, big, 0),
        lambda: lib.fs2_tsne_affinities(p, 96, 64, 10.0, p, None, None, p,
                                        lib.fs2_tsne_affinities_ws_bytes(96) - 8, 0),
        lambda: lib.fs2_tsne_state_init(p, 4097, 50.0, 1000, 250, 300, 12.0, 50.0, 1e-7, 0),
        lambda: lib.fs2_tsne_state_init(p, 50, 50.0, 1000, 250, 300, 12.0, 50.0, 1e-7, 0),
        lambda: lib.fs2_tsne_state_init(p, 96, 10.0, 0, 250, 300, 12.0, 50.0, 1e-7, 0),
        lambda: lib.fs2_tsne_state_init(None, 96, 10.0, 1000, 250, 300, 12.0, 50.0, 1e-7, 0),
        lambda: lib.fs2_tsne_rowsum(p, 4097, p, p, 0),
        lambda: lib.fs2_tsne_rowsum(p, 96, p, None, 0),
        lambda: lib.fs2_tsne_update(p, p, p + 8, p, p, 4097, 0, p, p, p, p, 0),
        lambda: lib.fs2_tsne_update(p, p, p, p, p, 96, 0, p, p, p, p, 0),     # Y_out is Y
        lambda: lib.fs2_tsne_update(p, p, p + 8, p, p, 96, 0, None, p, p, p, 0),
        lambda: lib.fs2_tsne_update(p, p, p + 8, p, p, 96, -1, p, p, p, p, 0),
        lambda: lib.fs2_tsne_step(p, p, p + 8, p, p, 4097, 12.0, 0.5, 50.0, p, p, p, 0),
        lambda: lib.fs2_tsne_step(p, p, p + 8, p, p, 96, 12.0, 0.5, 50.0, p, None, p, 0),
        lambda: lib.fs2_tsne_kl(p, p, 4097, 1.0, p, p, p, 0),
        lambda: lib.fs2_tsne_kl(p, None, 96, 1.0, p, p, p, 0),
        lambda: lib.fs2_tsne_control(p, 4097, 49, p, p, 0),
        lambda: lib.fs2_tsne_control(None, 96, 49, p, p, 0),
        lambda: lib.fs2_tsne_finish(p, 4097, p, 0),
        lambda: lib.fs2_tsne_finish(p, 96, None, 0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(L.KernelError):
            call()
            pytest.fail(f"call {k} was accepted")
    # n = 0 launches nothing and needs no operand
    assert lib.fs2_tsne_points(None, None, 0, 64, 400, None, 0) == 0
    assert lib.fs2_tsne_pca_init(None, 0, 64, None, None, 0, 0) == 0
    assert lib.fs2_tsne_affinities(None, 0, 64, 50.0, None, None, None, None, 0, 0) == 0
    assert lib.fs2_tsne_rowsum(None, 0, None, None, 0) == 0
    assert lib.fs2_tsne_update(None, None, None, None, None, 0, 0, None, None, None, None, 0) == 0
    assert lib.fs2_tsne_finish(None, 0, None, 0) == 0
    assert lib.fs2_tsne_pca_ws_bytes(96, 64) == (3 * 64 + 2 * 96 + 64 * 64) * 8
    assert lib.fs2_tsne_affinities_ws_bytes(96) == (96 * 96 + 96) * 8


def test_tsne_rejects_bad_settings_without_a_device():
    M = importlib.import_module(PKG + ".embedding_map")
    with pytest.raises(ValueError):
        M.TSNE(max_iter=0, device="cpu")
    t = M.TSNE(perplexity=50.0, device="cpu")
    with pytest.raises(ValueError):
        t._x(np.zeros((50, 8), np.float32))
    assert t.lr(240) == 50.0 and t.lr(4800) == 100.0
    assert M.TSNE(learning_rate=200.0, device="cpu").lr(240) == 200.0


def test_embedding_map_imports_without_matplotlib(monkeypatch):
    for name in [m for m in sys.modules if m == "matplotlib" or m.startswith("matplotlib.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "matplotlib", None)  # import matplotlib now raises
    monkeypatch.delitem(sys.modules, PKG + ".embedding_map", raising=False)
    M = importlib.import_module(PKG + ".embedding_map")
    assert callable(M.speaker_map) and callable(M.plot_speaker_map)
    with pytest.raises(ImportError):
        M.plot_speaker_map({}, "unused.png")
