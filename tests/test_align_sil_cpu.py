"""Optional positions in the aligner, the parts that need no GPU: the oracle
(``align_sil_oracle``) against independent references -- the forward-sum with skippable labels
against ``-logsumexp`` over the kept subsets of ``torch.nn.functional.ctc_loss``, the search
against enumeration of every kept subset and every split -- the all-zero mask against
``align_oracle``, ``parse_phn`` with ``|``, the argument checks of the two new entry points, and
the premise of the GPU convergence test.

The premise, measured with ``python tests/align_sil_oracle.py`` (the torch model on the CPU, 100
Adam steps of batches of 8, temperature 0.05, the prior off, ``synth_corpus_sil`` of seeds 0..4):

  trained agreement with the mask      0.921 0.933 0.826 0.807 0.831   mean 0.864, spread (sample
                                                                       standard deviation) 0.059
  its pause accuracy                   0.958 0.940 0.899 0.897 0.950   mean 0.929, spread 0.029
  untrained agreement / pause accuracy 0.095 0.081 0.093 0.124 0.106 / 0.50 0.48 0.45 0.42 0.63
  trained and aligned without          0.769 0.778 0.781 0.759 0.784   mean 0.774
  positions for the pauses
  masked minus unmasked                0.152 0.155 0.045 0.048 0.047

The mask is ahead on every seed, but by more than the seed-to-seed spread of 0.059 only on seeds
0 and 1; on seeds 2-4 the gap is inside it.  What all five support, and what the test asserts on
its seed, is masked > unmasked, not a margin.

Two things had to be changed to get there, both measured on the same seeds.  With the prior on
(omega = 1) and every pause optional the trained model omitted nearly every optional position on
all five seeds (pause accuracy 0.30, 0.29, 0.32, 0.29, 0.30; agreement 0.69, 0.61, 0.66, 0.57,
0.64): the prior is a pmf over the positions, it costs every label log N or more against the blank,
and the blank then explains the silent frames.  With the prior off it learned the pauses on seeds
0, 2, 4 (pause accuracy 0.72, 0.92, 0.92) and not on 1 and 3 (0.29, 0.30).  With 30 % of the
pauses that are there written out in the transcription (``explicit``) it learns them on all five
seeds, prior off (above) or on (agreement 0.898, 0.879, 0.832, 0.830, 0.900, pause accuracy 0.958,
0.905, 0.881, 0.846, 0.901).  The corpus was changed, not the claim.
"""
import importlib

import numpy as np
import pytest
import torch

import align_oracle as O
import align_sil_oracle as S

PKG = "mid-attribute-speaker-generation_amd"


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


# (N, M, mask): both ends marked, N = 1, M below N but at or above the unmarked count, one mark
SHAPES = [(1, 1, [0]), (1, 4, [0]), (2, 2, [1, 0]), (2, 1, [1, 0]), (2, 3, [0, 1]),
          (3, 2, [1, 0, 1]), (3, 1, [1, 0, 1]), (3, 5, [1, 0, 1]), (4, 6, [1, 0, 1, 0]),
          (5, 5, [0, 1, 0, 1, 0]), (5, 3, [1, 0, 1, 0, 1]), (5, 2, [1, 0, 1, 0, 1]),
          (5, 7, [1, 0, 1, 0, 1]), (4, 5, [0, 0, 0, 1]), (6, 4, [0, 1, 0, 0, 1, 0]),
          (4, 5, [0, 0, 0, 0])]


# ------------------------------------------------------------------ forward-sum
@pytest.mark.parametrize("N,M,mask", SHAPES)
def test_oracle_forward_sum_opt_is_the_sum_over_kept_subsets(N, M, mask):
    rng = np.random.default_rng(100 * N + M)
    lp = torch.from_numpy(rng.standard_normal((M + 2, N + 1)) * 2.0 - 3.0).requires_grad_()
    want = S.forward_sum_opt_brute(lp, N, M, mask)
    assert torch.isfinite(want)
    want.backward()
    got, grad = S.forward_sum_opt(lp.detach().numpy(), N, M, mask)
    assert abs(got - float(want.detach())) <= 1e-9 * max(1.0, abs(got))
    g = lp.grad.numpy()
    np.testing.assert_allclose(grad, g[:M, :N], rtol=0, atol=1e-9)
    assert not g[M:].any() and not g[:, N:].any()
    # the differentiable recursion: the same loss and, through autograd, the same gradient
    lp2 = lp.detach().clone().requires_grad_()
    pad = np.asarray([list(mask) + [1]], np.uint8)  # a mark past N is not read
    nll = S.forward_sum_opt_torch(lp2[None], [N], [M], pad)
    nll.sum().backward()
    assert abs(float(nll.detach()[0]) - got) <= 1e-9 * max(1.0, abs(got))
    np.testing.assert_allclose(lp2.grad.numpy(), g, rtol=0, atol=1e-9)


@pytest.mark.parametrize("N,M,mask", [(3, 1, [0, 1, 0]), (5, 2, [0, 1, 0, 1, 0]), (2, 1, [0, 0]),
                                      (4, 1, [1, 0, 0, 1])])
def test_oracle_forward_sum_opt_without_a_path(N, M, mask):
    lp = np.random.default_rng(3).standard_normal((M, N))
    assert torch.isinf(S.forward_sum_opt_brute(torch.from_numpy(lp), N, M, mask))
    nll, grad = S.forward_sum_opt(lp, N, M, mask)
    assert nll == np.inf and grad.shape == (M, N) and not grad.any()


def test_zero_mask_is_the_plain_oracle():
    rng = np.random.default_rng(5)
    for N, M in ((1, 1), (1, 6), (4, 4), (5, 9), (12, 30), (40, 90), (3, 2)):
        lp = (rng.standard_normal((M, N)) * 2.0 - 3.0).astype(np.float32)
        zero = np.zeros(N, np.uint8)
        a, b = S.forward_sum_opt(lp, N, M, zero), O.forward_sum(lp, N, M)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])  # exactly: a closed edge adds exp(-inf)
        if M >= N:
            assert np.array_equal(S.mas_opt(lp, N, M, zero), O.mas(lp, N, M))
        else:
            assert not S.mas_opt(lp, N, M, zero).any()


# ------------------------------------------------------------------ MAS
def _random_mask(rng, N, p=0.5):
    m = (rng.random(N) < p).astype(np.uint8)
    for s in range(1, N):
        if m[s] and m[s - 1]:
            m[s] = 0
    if m.all():
        m[0] = 0
    return m


def test_oracle_mas_opt_is_brute_force_on_floats():
    """Random floats: the fp32 recursion's path scores what the fp64 enumeration's best does, to
    the rounding of M fp32 adds; durations sum to M and are 0 only at marked positions."""
    rng = np.random.default_rng(21)
    paths = 0
    for trial in range(120):
        N, M = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        mask = _random_mask(rng, N)
        x = (rng.standard_normal((M, N)) * 2.0 - 3.0).astype(np.float32)
        dur = S.mas_opt(x, N, M, mask)
        best, want = S.mas_opt_brute(x, N, M, mask)
        if best == -np.inf:
            assert not dur.any() and M < N - int(mask.sum())
            continue
        paths += 1
        assert dur.sum() == M and not (dur[mask == 0] == 0).any()
        zeros = np.flatnonzero(dur == 0)
        assert not (np.diff(zeros) == 1).any()  # never two neighbours omitted
        score = float(x.astype(np.float64)[np.arange(M), O.path_of(dur)].sum())
        assert abs(score - best) <= 2 * M * 2.0 ** -24 * np.abs(x).sum(), (N, M, mask)
    assert paths >= 80


def test_oracle_mas_opt_tie_rules_on_integers():
    """Small integers: sums are exact, ties are exact, and the rules decide: the end N - 1 unless
    N - 2 is strictly better, the diagonal on a tie with staying, the skip only when strictly
    better than both."""
    rng = np.random.default_rng(22)
    ties = 0
    for trial in range(400):
        N, M = int(rng.integers(1, 6)), int(rng.integers(1, 8))
        mask = _random_mask(rng, N)
        x = rng.integers(-2 if trial % 2 else -1, 1, (M, N)).astype(np.float32)
        if trial % 10 == 0:
            x[:] = 0.0  # every path ties
        dur = S.mas_opt(x, N, M, mask)
        best, want = S.mas_opt_brute(x, N, M, mask)
        assert np.array_equal(dur, want), (N, M, mask, x, dur, want)
        ties += best != -np.inf
    assert ties >= 300
    # all ties: nothing is strictly better, so no position is omitted while frames last ...
    assert S.mas_opt(np.zeros((6, 5), np.float32), 5, 6, [1, 0, 1, 0, 1]).tolist() == [2, 1, 1, 1, 1]
    # ... and with fewer frames than positions the path must skip
    assert S.mas_opt(np.zeros((3, 5), np.float32), 5, 3, [1, 0, 1, 0, 1]).sum() == 3


# ------------------------------------------------------------------ .phn parsing
def test_phn_parsing_with_optional_silences(tmp_path):
    A = _mod("align")
    table = {s: i for i, s in enumerate(_mod("dataset").symbol_table())}
    p = str(tmp_path / "u.phn")
    for line, with_edges, without in S.PARSE:
        for edges, want in ((True, with_edges), (False, without)):
            with open(p, "w", encoding="utf-8") as f:
                f.write(line + "\n")
            if want is None:
                with pytest.raises(ValueError, match="u.phn"):
                    A.parse_phn(p, table, "sp", edges)
                continue
            phones, ids, optional = A.parse_phn(p, table, "sp", edges)
            assert (phones, list(optional)) == want, (line, edges)
            assert ids == [table[s] for s in phones]
            assert not any(a and b for a, b in zip(optional, optional[1:])) and not all(optional)
    # without optional_sil: the 2-tuple and the error on '|', as before
    with open(p, "w", encoding="utf-8") as f:
        f.write("a k | o\n")
    with pytest.raises(ValueError, match=r"unknown symbol '\|'"):
        A.parse_phn(p)
    with pytest.raises(ValueError, match=r"unknown symbol '\|'"):
        A.parse_phn(p, table)
    with open(p, "w", encoding="utf-8") as f:
        f.write("a k sp o\n")
    assert A.parse_phn(p) == (["a", "k", "sp", "o"], [table[s] for s in ("a", "k", "sp", "o")])
    with pytest.raises(ValueError, match="optional_sil"):
        A.parse_phn(p, table, "no-such-symbol")
    with pytest.raises(ValueError, match="missing.phn"):
        A.parse_phn(str(tmp_path / "missing.phn"), table, "sp")


# ------------------------------------------------------------------ the C entry points
def test_new_entries_validate_arguments_before_any_launch():
    L = _mod("_lib")
    assert {"fs2_forward_sum_opt", "fs2_mas_opt"} <= set(L.lib.symbols())
    lib, p, big = L.lib, 16, 1 << 40  # p: a non-null placeholder, never dereferenced
    bad = [
        lambda: lib.fs2_forward_sum_opt(p, p, p, None, p, 2, 50, 9, p, p, p, big, 0),  # no mask
        lambda: lib.fs2_forward_sum_opt(p, p, p, p, None, 2, 50, 9, p, p, p, big, 0),
        lambda: lib.fs2_forward_sum_opt(p, p, p, p, p, 2, 50, 1025, p, p, p, big, 0),
        lambda: lib.fs2_forward_sum_opt(p, p, p, p, p, 2, 2049, 9, p, p, p, big, 0),
        lambda: lib.fs2_forward_sum_opt(p, p, p, p, p, 65536, 50, 9, p, p, p, big, 0),
        lambda: lib.fs2_forward_sum_opt(p, p, p, p, p, 2, 50, 9, p, p, p,
                                        lib.fs2_forward_sum_ws_bytes(2, 50, 9) - 1, 0),
        lambda: lib.fs2_mas_opt(p, p, p, None, 2, 50, 9, p, p, big, 0),  # no mask
        lambda: lib.fs2_mas_opt(p, p, None, p, 2, 50, 9, p, p, big, 0),
        lambda: lib.fs2_mas_opt(p, p, p, p, 2, 2049, 9, p, p, big, 0),
        lambda: lib.fs2_mas_opt(p, p, p, p, 2, 50, 0, p, p, big, 0),
        lambda: lib.fs2_mas_opt(p, p, p, p, 2, 50, 9, p, p, lib.fs2_mas_ws_bytes(2, 50, 9) - 1, 0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(L.KernelError):
            call()
            pytest.fail(f"call {k} was accepted")
    assert lib.fs2_forward_sum_opt(None, None, None, None, None, 0, 50, 9, None, None, None, 0,
                                   0) == 0
    assert lib.fs2_mas_opt(None, None, None, None, 0, 50, 9, None, None, 0, 0) == 0


def test_wrappers_take_the_mask_and_reject_host_tensors():
    K = _mod("kernels")
    lp, n = torch.zeros(1, 4, 3), torch.tensor([3])
    mask = torch.zeros(1, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        K.mas(lp, n, n, optional=mask)
    with pytest.raises(RuntimeError, match="GPU"):
        K.forward_sum(lp, n, n, torch.ones(1), optional=mask)


# ------------------------------------------------------------------ the premise of convergence
@pytest.fixture(scope="module")
def run():
    return S.oracle_run(S.SEED)


def test_the_oracle_learns_the_pauses(run):
    """Conditions on the inputs of tests/test_gpu_align_sil.py, from the measurements above: the
    model trained with the mask is above the same model without positions for the pauses (by what
    margin depends on the seed, see above), clearly above itself untrained, and its pause
    decisions are clearly better than the untrained model's."""
    print({k: round(v, 3) for k, v in run.items() if k != "init"})
    assert run["trained"] >= 0.85 and run["pause"] >= 0.85
    assert run["trained"] > run["unmasked"]  # 0.933 against 0.778 here; positive on all five seeds
    assert run["untrained"] <= 0.20 and run["trained"] >= run["untrained"] + 0.50
    assert run["pause"] >= run["untrained_pause"] + 0.25  # 0.940 against 0.483
