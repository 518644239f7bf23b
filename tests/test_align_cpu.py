"""The aligner's parts that need no GPU: the oracle (``align_oracle``) against independent
references -- forward-sum against ``torch.nn.functional.ctc_loss``, MAS against enumeration of
every monotonic path, the prior against scipy -- the TextGrid writer's round trip through the
existing reader and trim, ``.phn`` parsing, and the argument checks of the new entry points."""
import importlib
import itertools

import numpy as np
import pytest
import torch

import align_oracle as O

PKG = "mid-attribute-speaker-generation_amd"
NEW = ("fs2_align_logprob", "fs2_align_logprob_bwd_ws_bytes", "fs2_align_logprob_bwd",
       "fs2_forward_sum_ws_bytes", "fs2_forward_sum", "fs2_mas_ws_bytes", "fs2_mas")


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


# ------------------------------------------------------------------ forward-sum
@pytest.mark.parametrize("lens", [[(1, 1)], [(5, 5)], [(3, 7), (1, 4), (6, 6), (4, 11)]],
                         ids=["one-by-one", "N=M", "ragged"])
def test_oracle_forward_sum_is_ctc_loss(lens):
    """Loss and gradient through the blank log-softmax, fp64."""
    rng = np.random.default_rng(11)
    B, T_s, T_m = len(lens), max(n for n, _ in lens) + 1, max(m for _, m in lens) + 2
    logp = torch.from_numpy(rng.standard_normal((B, T_m, T_s)) * 2.0 - 3.0).requires_grad_()
    src, mel = [n for n, _ in lens], [m for _, m in lens]
    nll = O.forward_sum_torch(logp, src, mel)
    nll.sum().backward()
    nll = nll.detach()
    for b, (n, m) in enumerate(lens):
        got, grad = O.forward_sum(logp[b].detach().numpy(), n, m)
        assert abs(got - float(nll[b])) <= 1e-10 * max(1.0, abs(got)), (b, got, float(nll[b]))
        want = logp.grad[b].numpy()
        np.testing.assert_allclose(grad, want[:m, :n], rtol=0, atol=1e-10)
        assert not want[m:].any() and not want[:, n:].any()


def test_oracle_forward_sum_without_a_path():
    nll, grad = O.forward_sum(np.zeros((2, 3)), 3, 2)
    assert nll == np.inf and grad.shape == (2, 3) and not grad.any()


# ------------------------------------------------------------------ MAS
def test_oracle_mas_is_brute_force():
    """Small integers: every path score is exact in fp32 and fp64, so ties are exact and the
    tie rule (the diagonal) decides which of the equal paths comes out."""
    rng = np.random.default_rng(12)
    ties = 0
    for N in range(1, 5):
        for M in range(N, 9):
            for trial in range(6):
                hi = 1 if trial < 3 else 4  # few distinct values: many ties
                x = rng.integers(-hi, 1, (M, N)).astype(np.float32)
                dur = O.mas(x, N, M)
                score, want = O.mas_brute(x, N, M)
                assert dur.sum() == M and (dur >= 1).all()
                assert float(x[np.arange(M), O.path_of(dur)].sum()) == score, (N, M, trial)
                assert np.array_equal(dur, want), (N, M, trial, dur, want)
                n_best = sum(1 for c in itertools.combinations(range(1, M), N - 1)
                             if float(x[np.arange(M), O.path_of(np.diff((0,) + c + (M,)))].sum())
                             == score)
                ties += n_best > 1
    assert ties >= 30  # the tie rule was exercised, not avoided


def test_oracle_mas_rejects_fewer_frames_than_phonemes():
    with pytest.raises(ValueError):
        O.mas(np.zeros((2, 3), np.float32), 3, 2)


# ------------------------------------------------------------------ prior
def test_prior_is_scipys_beta_binomial():
    from scipy.stats import betabinom
    for N, M, omega in ((1, 1, 1.0), (1, 9, 1.0), (7, 7, 1.0), (12, 40, 0.5), (130, 300, 1.0),
                        (64, 200, 2.0)):
        got = O.log_prior(N, M, omega)
        t = np.arange(M)[:, None]
        want = betabinom.logpmf(np.arange(N)[None, :], N - 1, omega * (t + 1), omega * (M - t))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))
        np.testing.assert_allclose(np.exp(got).sum(1), 1.0, atol=1e-9)


# ------------------------------------------------------------------ TextGrid round trip
@pytest.mark.parametrize("hop,sr", [(256, 22050), (300, 24000)])
def test_write_textgrid_round_trip(tmp_path, hop, sr):
    """The existing reader, ``durations_from_intervals`` and the trim of ``Preprocessor._stage``
    give back the durations and a waveform that holds every frame."""
    io, pre = _mod("corpus_io"), _mod("preprocess")
    rng = np.random.default_rng(13)
    path = str(tmp_path / "u.TextGrid")
    for trial in range(40):
        n = int(rng.integers(1, 40))
        d = rng.integers(1, 10, n)
        d[rng.random(n) < 0.4] = 1  # 1-frame phonemes
        if trial % 4 == 0:
            d[int(rng.integers(n))] += int(rng.integers(100, 3000))  # far boundaries too
        phones = [("a", "k", "sp", 'q"uote')[int(i)] for i in rng.integers(0, 4, n)]
        phones[0] = phones[-1] = "a"  # no silence at the ends: nothing is trimmed
        io.write_textgrid(path, phones, d, hop, sr)
        tiers = io.read_textgrid(path)
        assert list(tiers) == ["phones"]
        got_p, got_d, start, end = pre.durations_from_intervals(tiers["phones"], sr, hop)
        assert got_p == phones and got_d == d.tolist()
        assert int(sr * start) == 0 and int(sr * end) - int(sr * start) >= int(d.sum()) * hop
        assert int(sr * end) == int(d.sum()) * hop  # and not a sample more than was aligned


def test_boundary_time_for_every_frame_count():
    """``n hop / sr`` itself fails the trim for some n; the written time does not."""
    io = _mod("corpus_io")
    for hop, sr in ((256, 22050), (300, 24000)):
        short = 0
        for n in range(1, 4000):
            t = float(repr(io.boundary_time(n, hop, sr)))
            assert int(sr * t) == n * hop and int(np.round(t * sr / hop)) == n
            short += int(sr * float(repr(n * hop / sr))) < n * hop
        if hop == 256:
            assert short == 326


def test_write_textgrid_rejects_bad_input(tmp_path):
    io = _mod("corpus_io")
    for phones, d in ((["a"], [1, 2]), ([], []), (["a", " "], [1, 1]), (["a"], [-1])):
        with pytest.raises(ValueError):
            io.write_textgrid(str(tmp_path / "x.TextGrid"), phones, d, 256, 22050)


# ------------------------------------------------------------------ .phn parsing
def test_phn_parsing(tmp_path):
    A = _mod("align")
    table = {s: i for i, s in enumerate(_mod("dataset").symbol_table())}
    p = str(tmp_path / "u.phn")
    for text in ("a k a sp k\n", "{a k a sp k}\nsecond line\n", "  a  k a sp k  "):
        with open(p, "w", encoding="utf-8") as f:
            f.write(text)
        phones, ids = A.parse_phn(p)
        assert phones == ["a", "k", "a", "sp", "k"] and ids == [table[s] for s in phones]
    for text in ("a zzz k\n", "\n", "a _ k\n", "{}\n"):  # unknown, empty, the padding symbol
        with open(p, "w", encoding="utf-8") as f:
            f.write(text)
        with pytest.raises(ValueError, match="u.phn"):
            A.parse_phn(p)
    with pytest.raises(ValueError, match="missing.phn"):
        A.parse_phn(str(tmp_path / "missing.phn"))


# ------------------------------------------------------------------ the C entry points
def test_entries_validate_arguments_before_any_launch():
    L = _mod("_lib")
    assert set(NEW) <= set(L.lib.symbols())
    lib, p, big = L.lib, 16, 1 << 40  # p: a non-null placeholder, never dereferenced
    bad = [
        lambda: lib.fs2_align_logprob(None, p, p, p, 2, 50, 9, 40, 0.05, 1.0, p, 0),
        lambda: lib.fs2_align_logprob(p, p, p, p, 2, 50, 9, 40, 0.05, 1.0, None, 0),
        lambda: lib.fs2_align_logprob(p, p, p, p, 2, 2049, 9, 40, 0.05, 1.0, p, 0),
        lambda: lib.fs2_align_logprob(p, p, p, p, 2, 50, 1025, 40, 0.05, 1.0, p, 0),
        lambda: lib.fs2_align_logprob(p, p, p, p, 2, 0, 9, 40, 0.05, 1.0, p, 0),
        lambda: lib.fs2_align_logprob(p, p, p, p, 2, 50, 9, 44, 0.05, 1.0, p, 0),   # A % 8
        lambda: lib.fs2_align_logprob(p, p, p, p, 2, 50, 9, 136, 0.05, 1.0, p, 0),  # A > 128
        lambda: lib.fs2_align_logprob(p, p, p, p, 2, 50, 9, 40, 0.0, 1.0, p, 0),    # temperature
        lambda: lib.fs2_align_logprob_bwd(p, p, None, p, p, 2, 50, 9, 40, 0.05, p, p, p, big, 0),
        lambda: lib.fs2_align_logprob_bwd(p, p, p, p, p, 2, 50, 9, 40, 0.05, p, p, p,
                                          lib.fs2_align_logprob_bwd_ws_bytes(2, 50, 9, 40) - 1, 0),
        lambda: lib.fs2_align_logprob_bwd(p, p, p, p, p, 2, 50, 9, 12, 0.05, p, p, p, big, 0),
        lambda: lib.fs2_forward_sum(p, p, p, None, 2, 50, 9, p, p, p, big, 0),
        lambda: lib.fs2_forward_sum(p, p, p, p, 2, 50, 1025, p, p, p, big, 0),
        lambda: lib.fs2_forward_sum(p, p, p, p, 2, 50, 9, p, p, p,
                                    lib.fs2_forward_sum_ws_bytes(2, 50, 9) - 1, 0),
        lambda: lib.fs2_mas(p, p, None, 2, 50, 9, p, p, big, 0),
        lambda: lib.fs2_mas(p, p, p, 2, 2049, 9, p, p, big, 0),
        lambda: lib.fs2_mas(p, p, p, 2, 50, 9, p, p, lib.fs2_mas_ws_bytes(2, 50, 9) - 1, 0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(L.KernelError):
            call()
            pytest.fail(f"call {k} was accepted")
    # an empty batch launches nothing and needs no operand
    assert lib.fs2_align_logprob(None, None, None, None, 0, 50, 9, 40, 0.05, 1.0, None, 0) == 0
    assert lib.fs2_align_logprob_bwd(None, None, None, None, None, 0, 50, 9, 40, 0.05, None, None,
                                     None, 0, 0) == 0
    assert lib.fs2_forward_sum(None, None, None, None, 0, 50, 9, None, None, None, 0, 0) == 0
    assert lib.fs2_mas(None, None, None, 0, 50, 9, None, None, 0, 0) == 0
    # dL/dscore and the 256-frame dk partials; the label states' alpha in fp64; a step byte a cell
    assert lib.fs2_align_logprob_bwd_ws_bytes(2, 300, 9, 40) == 2 * (300 * 9 + 2 * 9 * 40) * 4
    assert lib.fs2_forward_sum_ws_bytes(2, 50, 9) == 2 * 50 * 9 * 8
    assert lib.fs2_mas_ws_bytes(2, 50, 9) == 2 * 50 * 9
    assert lib.fs2_mas_ws_bytes(1, 2049, 9) == 0 and lib.fs2_forward_sum_ws_bytes(0, 50, 9) == 0


def test_wrappers_reject_host_tensors_and_rows_without_a_path():
    K = _mod("kernels")
    lp, n = torch.zeros(1, 4, 3), torch.tensor([3])
    with pytest.raises(RuntimeError, match="GPU"):
        K.mas(lp, n, n)
    with pytest.raises(RuntimeError, match="GPU"):
        K.align_logprob(torch.zeros(1, 4, 8), torch.zeros(1, 3, 8), n, n, 0.05)
