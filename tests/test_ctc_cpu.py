"""The phoneme error rate's parts that need no GPU: the oracle (``ctc_oracle``) against
independent references -- the CTC loss against ``torch.nn.functional.ctc_loss`` composed with
``log_softmax``, the edit distance against a second DP and known answers, the greedy decoder on
hand-made frames -- and the argument checks of the new entry points, wrappers and command lines."""
import importlib

import numpy as np
import pytest
import torch

import ctc_oracle as O

PKG = "mid-attribute-speaker-generation_amd"
NEW = ("fs2_ctc_loss_ws_bytes", "fs2_ctc_loss", "fs2_ctc_greedy", "fs2_edit_distance_ws_bytes",
       "fs2_edit_distance")


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


# ------------------------------------------------------------------ CTC
# (C, blank, [(target, M)]): feasible rows, repeated labels and blank != 0 among them
CTC_CASES = {
    "distinct": (6, 0, [([1, 2, 3], 5), ([4], 1), ([2, 5, 1, 3], 9)]),
    "repeats": (5, 0, [([1, 1], 3), ([2, 2, 2], 7), ([1, 3, 3, 1, 1, 4], 11)]),
    "blank-2": (7, 2, [([0, 1, 1, 6], 8), ([3], 4), ([0, 0], 3), ([6, 5, 4, 3], 4)]),
    "empty": (4, 0, [([], 3), ([1], 2)]),
}


@pytest.mark.parametrize("name", list(CTC_CASES))
def test_oracle_ctc_is_torch_ctc_loss_after_log_softmax(name):
    """Loss and the LOGITS gradient through autograd of both ops, fp64 (torch's CTC backward is
    only correct composed with the log-softmax)."""
    C, blank, rows = CTC_CASES[name]
    rng = np.random.default_rng(21)
    B, T, ld = len(rows), max(m for _, m in rows) + 2, C + 3
    L_max = max(1, max(len(t) for t, _ in rows))
    x32 = (rng.standard_normal((B, T, ld)) * 2.0).astype(np.float32)
    logits = torch.from_numpy(x32.astype(np.float64)).requires_grad_()
    targets = np.zeros((B, L_max), np.int64)
    for b, (t, _) in enumerate(rows):
        targets[b, :len(t)] = t
    nll = O.ctc_torch(logits, targets, [m for _, m in rows], [len(t) for t, _ in rows], C, blank)
    nll.sum().backward()
    for b, (t, m) in enumerate(rows):
        got, grad = O.ctc(x32[b], t, m, C, blank)
        want = float(nll[b].detach())
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (b, got, want)
        g = logits.grad[b].numpy()
        np.testing.assert_allclose(grad, g[:m, :C], rtol=0, atol=1e-10)
        assert not g[m:].any() and not g[:, C:].any()


def test_oracle_ctc_rows_without_a_path():
    x = np.zeros((4, 5), np.float32)
    for target, M, C, blank in (([1, 1], 2, 5, 0),     # a repeat needs a blank between
                                ([1, 2, 3], 2, 5, 0),  # fewer frames than labels
                                ([1, 5], 4, 5, 0),     # a label equal to C
                                ([1, -1], 4, 5, 0),
                                ([1, 0], 4, 5, 0),     # a label equal to blank
                                ([1, 2], 4, 5, 2)):
        nll, grad = O.ctc(x, target, M, C, blank)
        assert nll == np.inf and grad.shape == (M, C) and not grad.any()
    nll, grad = O.ctc(x, [1, 1], 3, 5, 0)  # exactly one path: 1, blank, 1
    assert abs(nll - 3 * np.log(5.0)) < 1e-12
    assert np.isfinite(grad).all()


# ------------------------------------------------------------------ edit distance
def test_oracle_edit_distance_is_the_plain_dp():
    rng = np.random.default_rng(22)
    for trial in range(300):
        n_sym = 2 if trial % 3 == 0 else 4
        ref = rng.integers(0, n_sym, int(rng.integers(0, 14)))
        hyp = rng.integers(0, n_sym, int(rng.integers(0, 14)))
        d, s, de, i = O.edit_distance(ref, hyp)
        assert d == O.edit_distance_plain(ref.tolist(), hyp.tolist())
        assert s + de + i == d and len(ref) - de == len(hyp) - i and min(s, de, i) >= 0


def test_oracle_edit_distance_known_answers():
    assert O.edit_distance(list("kitten"), list("sitting")) == (3, 2, 0, 1)
    assert O.edit_distance([], []) == (0, 0, 0, 0)
    assert O.edit_distance([], [3, 4, 5]) == (3, 0, 0, 3)
    assert O.edit_distance([3, 4, 5], []) == (3, 0, 3, 0)
    assert O.edit_distance([1, 2, 3], [1, 2, 3]) == (0, 0, 0, 0)
    assert O.edit_distance([1, 2], [3, 4, 5]) == (3, 2, 0, 1)
    # a tie between a deletion and an insertion path of the same cost: substitutions win
    assert O.edit_distance([1, 2], [2, 1]) == (2, 2, 0, 0)


# ------------------------------------------------------------------ greedy
def test_oracle_greedy_on_hand_made_frames():
    nan = np.nan
    x = np.asarray([[0, 5, 5, 1],      # a tie: the lowest class, 1
                    [0, 5, 5, 1],      # a repeat: collapsed
                    [9, 0, 0, 0],      # blank
                    [0, 5, 0, 0],      # 1 again, across a blank: kept
                    [nan, nan, nan, nan],   # all NaN: blank
                    [nan, 1, nan, 2],  # a NaN never wins: 3
                    [nan, -np.inf, nan, -np.inf],  # the lowest class that is not a NaN: 1
                    [0, 0, 3, 0]], np.float32)
    assert O.argmax_frames(x, 8, 4).tolist() == [1, 1, 0, 1, 0, 3, 1, 2]
    assert O.greedy(x, 8, 4).tolist() == [1, 1, 3, 1, 2]
    assert O.greedy(x, 3, 4).tolist() == [1]
    assert O.greedy(x, 8, 3).tolist() == [1, 1, 1, 2]       # the last column is not a class
    assert O.greedy(x, 8, 4, blank=1).tolist() == [0, 3, 2]  # frame 4, all NaN, is the blank 1


# ------------------------------------------------------------------ the C entry points
def test_entries_validate_arguments_before_any_launch():
    L = _mod("_lib")
    assert set(NEW) <= set(L.lib.symbols())
    lib, p, big = L.lib, 16, 1 << 40  # p: a non-null placeholder, never dereferenced

    def loss(logits=p, targets=p, fl=p, tl=p, w=p, B=2, T=50, C=13, ld=16, blank=0, L_max=9,
             nll=p, grad=p, ws=p, ws_bytes=big):
        return lib.fs2_ctc_loss(logits, targets, fl, tl, w, B, T, C, ld, blank, L_max, nll, grad,
                                ws, ws_bytes, 0)

    def greedy(logits=p, fl=p, B=2, T=50, C=13, ld=16, blank=0, ids=p, lens=p, am=None):
        return lib.fs2_ctc_greedy(logits, fl, B, T, C, ld, blank, ids, lens, am, 0)

    def edit(ref=p, rl=p, hyp=p, hl=p, B=2, R=9, H=11, out=p, ws=p, ws_bytes=big):
        return lib.fs2_edit_distance(ref, rl, hyp, hl, B, R, H, out, ws, ws_bytes, 0)

    bad = [
        lambda: loss(logits=None), lambda: loss(targets=None), lambda: loss(fl=None),
        lambda: loss(tl=None), lambda: loss(w=None), lambda: loss(nll=None),
        lambda: loss(grad=None), lambda: loss(ws=None),
        lambda: loss(T=2049), lambda: loss(T=0), lambda: loss(L_max=1025), lambda: loss(L_max=-1),
        lambda: loss(C=1025, ld=1032), lambda: loss(C=0),
        lambda: loss(blank=13), lambda: loss(blank=-1),
        lambda: loss(C=17),  # C > ld
        lambda: loss(B=-1), lambda: loss(B=65536),
        lambda: loss(ws_bytes=lib.fs2_ctc_loss_ws_bytes(2, 50, 9) - 1),
        lambda: greedy(logits=None), lambda: greedy(fl=None), lambda: greedy(ids=None),
        lambda: greedy(lens=None),
        lambda: greedy(T=2049), lambda: greedy(C=1025, ld=1032), lambda: greedy(blank=13),
        lambda: greedy(C=17), lambda: greedy(B=-1),
        lambda: edit(ref=None), lambda: edit(rl=None), lambda: edit(hyp=None),
        lambda: edit(hl=None), lambda: edit(out=None), lambda: edit(ws=None),
        lambda: edit(R=2049), lambda: edit(H=2049), lambda: edit(R=-1), lambda: edit(B=-1),
        lambda: edit(ws_bytes=lib.fs2_edit_distance_ws_bytes(2, 9, 11) - 1),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(L.KernelError):
            call()
            pytest.fail(f"call {k} was accepted")
    # an empty batch launches nothing and needs no operand
    assert lib.fs2_ctc_loss(None, None, None, None, None, 0, 50, 13, 16, 0, 9, None, None, None,
                            0, 0) == 0
    assert lib.fs2_ctc_greedy(None, None, 0, 50, 13, 16, 0, None, None, None, 0) == 0
    assert lib.fs2_edit_distance(None, None, None, None, 0, 9, 11, None, None, 0, 0) == 0
    # every state's alpha in fp64; a step byte per cell of the (R + 1) x (H + 1) table's diagonals
    assert lib.fs2_ctc_loss_ws_bytes(2, 50, 9) == 2 * 50 * 19 * 8
    assert lib.fs2_ctc_loss_ws_bytes(3, 2048, 1024) == 3 * 2048 * 2049 * 8
    assert lib.fs2_ctc_loss_ws_bytes(1, 7, 0) == 7 * 8
    assert lib.fs2_edit_distance_ws_bytes(2, 9, 11) == 2 * 21 * 10
    assert lib.fs2_edit_distance_ws_bytes(1, 0, 0) == 1
    assert lib.fs2_ctc_loss_ws_bytes(1, 2049, 9) == 0 and lib.fs2_ctc_loss_ws_bytes(0, 50, 9) == 0
    assert lib.fs2_ctc_loss_ws_bytes(1, 50, 1025) == 0
    assert lib.fs2_edit_distance_ws_bytes(1, 2049, 1) == 0
    assert lib.fs2_edit_distance_ws_bytes(0, 9, 11) == 0
    assert lib.fs2_abi_version() == 1


def test_wrappers_reject_host_tensors():
    K = _mod("kernels")
    n = torch.tensor([3])
    with pytest.raises(RuntimeError, match="GPU"):
        K.ctc_loss(torch.zeros(1, 4, 8), torch.ones(1, 3, dtype=torch.int64), n, n,
                   torch.ones(1), n_classes=5)
    with pytest.raises(RuntimeError, match="GPU"):
        K.ctc_greedy(torch.zeros(1, 4, 8), n, n_classes=5)
    with pytest.raises(RuntimeError, match="GPU"):
        K.edit_distance(torch.ones(1, 3, dtype=torch.int64), n, torch.ones(1, 3, dtype=torch.int64),
                        n)


def test_per_from_sums():
    M = _mod("metrics")
    out = M.per_from_sums([7, 3, 1, 3, 5])
    assert out == {"distance": 7, "substitutions": 3, "deletions": 1, "insertions": 3,
                   "phonemes": 5, "per": 1.4}  # insertions count: above 1
    assert np.isnan(M.per_from_sums([0, 0, 0, 0, 0])["per"])


def test_recognizer_rejects_bad_shapes():
    R = _mod("recognizer")
    for kw in (dict(n_mels=81), dict(channels=60), dict(kernel=4), dict(layers=0)):
        with pytest.raises(ValueError):
            R.PhonemeRecognizer(13, device="cpu", **kw)
    with pytest.raises(ValueError):
        R.PhonemeRecognizer(1025, device="cpu")
    m = R.PhonemeRecognizer(429, channels=16, layers=1, kernel=3, device="cpu")
    assert m.ld == 432 and tuple(m.out.weight.shape) == (432, 16, 1)
    assert set(m.state_dict()) == set(O.TorchRecognizer(429, 80, 16, 1, 3).state_dict())


def test_command_lines_reject_bad_arguments(tmp_path):
    rec, se, tr = _mod("recognize"), _mod("speaker_eval"), _mod("train")
    for argv in (["--config", "JVS-VCTK", "--steps", "0"],
                 ["--config", "JVS-VCTK", "--batch", "0"],
                 ["--config", str(tmp_path / "nowhere")],
                 ["--steps", "5"],
                 ["--config", "JVS-VCTK", "--steps", "many"]):
        with pytest.raises(SystemExit):
            rec.main(argv)
    with pytest.raises(SystemExit):
        se.main(["-c", "JVS-VCTK", "--embedder", "e.pt", "--recognizer",
                 str(tmp_path / "missing.pt")])
    with pytest.raises(SystemExit):
        tr.main(["-c", "JVS-VCTK", "--synth_metrics", "--synth_recognizer",
                 str(tmp_path / "missing.pt")])
    with pytest.raises(SystemExit):
        tr.main(["-c", "JVS-VCTK", "--synth_recognizer", str(tmp_path / "missing.pt")])
    junk = str(tmp_path / "junk.pt")
    torch.save({"model": {}}, junk)
    with pytest.raises(ValueError, match="recogniser"):
        _mod("recognizer").load_recognizer(junk, "cpu")
