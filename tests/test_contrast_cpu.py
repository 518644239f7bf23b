"""The GE2E contrast loss, the parts that need no GPU: the fp64 closed form against the
reference's own ``get_similarity`` + ``get_contrast_loss`` (recorded in float64 as g18, and live
where the reference tree is present), the tie rule and the zeroed diagonal on hand-built
similarities, the C entry's argument validation, and ``GE2ELoss``'s choice of loss."""
import importlib
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
import contrast_oracle as co

PKG = "mid-attribute-speaker-generation_amd"


def _agree(got, want, tag, rel=1e-12):
    """Both sides are float64 evaluations of one formula: agreement to about 1e-12 of the
    reference tensor's max-abs (a few hundred roundings at 1.1e-16 each)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, peak = np.abs(got - want).max(), np.abs(want).max()
    print(f"{tag}: err {err:.3e} peak {peak:.3e}")
    assert err <= rel * peak, (tag, err, peak)


def _check_case(shape, ref):
    loss, demb, dw, db = co.ge2e_contrast(co.make_embeddings(*shape, co.SEEDS[shape]))
    assert demb.shape == shape
    for tag, got, want in zip(("loss", "demb", "dw", "db"), (loss, demb, dw, db), ref):
        _agree(got, want, f"{tag} at {shape}")


@pytest.mark.parametrize("k", range(len(co.CPU_SHAPES)))
def test_closed_form_reproduces_recorded_reference(k):
    g = load_golden("g18_contrast.npz")
    shape = co.CPU_SHAPES[k]
    assert tuple(g["shapes"][k]) == shape and int(g["seeds"][k]) == co.SEEDS[shape]
    _check_case(shape, [g[f"c{k}.{n}"] for n in ("loss", "demb", "dw", "db")])


@pytest.mark.parametrize("shape", co.CPU_SHAPES)
def test_closed_form_matches_reference_autograd(shape):
    """The reference's functions themselves, under torch autograd in float64."""
    mg = importlib.import_module("oracle.make_golden")
    if not os.path.isdir(os.path.join(mg.REF, "Multilingual-Speaker-Encoder-with-Domain-Adaptation")):
        pytest.skip("the reference tree is not on this machine (g18 holds its recorded results)")
    import sys
    import torch
    loaded = set(sys.modules)
    try:
        sen = mg.import_discriminator()
        utils = importlib.import_module(sen.__package__ + ".utils")
    finally:  # the reference package and its librosa stand-in stay out of the other tests
        for name in set(sys.modules) - loaded:
            if name == "librosa" or name.startswith("Multilingual-Speaker-Encoder"):
                del sys.modules[name]
    e = co.make_embeddings(*shape, co.SEEDS[shape])
    et = torch.from_numpy(e.astype(np.float64)).requires_grad_()
    w = torch.tensor(10.0, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(-5.0, dtype=torch.float64, requires_grad=True)
    loss = utils.get_contrast_loss(w * utils.get_similarity(et) + b)
    loss.backward()
    _check_case(shape, (loss.item(), et.grad.numpy(), w.grad.item(), b.grad.item()))


def test_similarity_matches_softmax_oracle_scores():
    """S is the softmax oracle's S: sum_k exp S recovers that loss."""
    from embedder_oracle import ge2e_softmax
    e = co.make_embeddings(4, 3, 64, 7)
    S, _ = co.similarity(e)
    own = S[np.arange(4), :, np.arange(4)]
    want = ge2e_softmax(e)[0]
    got = np.log(np.exp(S).sum(axis=2) + 1e-6).sum() - own.sum()
    assert abs(got - want) <= 1e-12 * abs(want)


def test_equal_negatives_give_the_lowest_k_the_gradient():
    S = np.full((4, 1, 4), -3.0)
    S[np.arange(4), 0, np.arange(4)] = 2.0
    S[2, 0, 1] = S[2, 0, 3] = 0.5  # row of speaker 2: k = 1 and k = 3 tie above k = 0
    S[0, 0, 1] = S[0, 0, 2] = S[0, 0, 3] = -1.0  # speaker 0: the own entry (k = 0) is lowest
    loss, dS, win = co.contrast_from_similarity(S)
    sig = lambda s: 1.0 / (1.0 + np.exp(-s))  # noqa: E731
    assert win[2, 0] == 1 and dS[2, 0, 1] == sig(0.5) * (1 - sig(0.5)) and dS[2, 0, 3] == 0
    assert win[0, 0] == 1 and dS[0, 0, 1] > 0 and dS[0, 0, 2] == 0 and dS[0, 0, 3] == 0
    assert win[1, 0] == 0 and win[3, 0] == 0  # all negatives equal: k = 0
    # one own entry and one winner per row, nothing else
    assert ((dS != 0).sum(axis=2) == 2).all()
    assert (dS[np.arange(4), 0, np.arange(4)] == -sig(2.0) * (1 - sig(2.0))).all()
    want = 4 * (1 - sig(2.0)) + sig(0.5) + sig(-1.0) + 2 * sig(-3.0)
    assert abs(loss - want) <= 1e-15 * 8
    # torch.max reports the same index on the zeroed tensor
    import torch
    s = torch.from_numpy(sig(S))
    s[list(range(4)), :, list(range(4))] = 0
    assert torch.equal(torch.max(s, dim=2)[1], torch.from_numpy(win))


def test_one_speaker_has_no_second_term():
    S = np.array([[[1.5], [-0.5], [0.0]]])  # (1, 3, 1)
    loss, dS, win = co.contrast_from_similarity(S)
    sig = 1.0 / (1.0 + np.exp(-S[0, :, 0]))
    assert loss == (1 - sig).sum()  # loss_2 = 0: the maximum is the zeroed own entry
    assert (win == 0).all() and np.array_equal(dS[0, :, 0], -sig * (1 - sig))
    e = co.make_embeddings(1, 2, 8, 3)
    S1, parts = co.similarity(e)
    loss, demb, dw, db = co.ge2e_contrast(e)
    s1 = 1.0 / (1.0 + np.exp(-S1[0, :, 0]))
    assert abs(loss - (1 - s1).sum()) <= 1e-15 and abs(db + (s1 * (1 - s1)).sum()) <= 1e-15
    assert np.abs(demb).max() > 0


def test_saturated_negative_below_the_zeroed_entry_carries_nothing():
    """sig underflows to 0 for every negative: the maximum is 0 at the lowest k, and whichever
    entry that is, nothing but the own entry has a gradient."""
    S = np.full((3, 2, 3), -800.0)
    S[np.arange(3), :, np.arange(3)] = 1.0
    with np.errstate(over="ignore"):
        loss, dS, win = co.contrast_from_similarity(S)
    assert (win == 0).all()
    off = dS.copy()
    off[np.arange(3), :, np.arange(3)] = 0
    assert (off == 0).all() and np.isfinite(loss)


def test_entry_is_declared_bound_and_validates_before_any_launch():
    """FS2_ERR_ARG paths return before a stream is touched, so they run without a GPU."""
    L = importlib.import_module(PKG + "._lib")
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "fs2hip.h")).read(),
                 flags=re.S)
    sig = lambda name: re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src).group(1)  # noqa: E731
    types = lambda args: [re.sub(r"\s*\w+$", "", a.strip()) for a in args.split(",")]  # noqa: E731
    assert types(sig("fs2_ge2e_contrast")) == types(sig("fs2_ge2e_softmax"))
    assert types(sig("fs2_ge2e_contrast_ws_bytes")) == ["int64_t"] * 3
    assert {"fs2_ge2e_contrast", "fs2_ge2e_contrast_ws_bytes"} <= set(L.lib.symbols())
    lib, p, big = L.lib, 16, 1 << 30  # p: a non-null, aligned placeholder, never dereferenced
    ws = lib.fs2_ge2e_contrast_ws_bytes
    # 3 N D centroid tables, N norms, 3 NM row scalars, NM D exclude-self gradients
    assert ws(3, 3, 64) == (3 * 3 * 64 + 3 + 3 * 9 + 9 * 64) * 4
    assert ws(17, 3, 64) < lib.fs2_ge2e_softmax_ws_bytes(17, 3, 64)  # no (NM, N) tables
    for shape in ((0, 3, 64), (3, 1, 64), (3, 0, 64), (3, 3, 0), (3, 3, 257), (-1, 3, 64),
                  (1 << 20, 1 << 20, 64), (1 << 62, 4, 64)):
        assert ws(*shape) == 0, shape
    ok = dict(emb=p, n=3, m=3, d=64, w=p, b=p, loss=p, ws=p, ws_bytes=big)
    bad = [dict(m=1), dict(m=0), dict(n=0), dict(d=0), dict(d=257), dict(n=1 << 20, m=1 << 20),
           dict(emb=None), dict(w=None), dict(b=None), dict(ws=None), dict(ws_bytes=8),
           dict(ws_bytes=ws(3, 3, 64) - 1)]
    for kw in bad:
        a = dict(ok, **kw)
        for demb in (None, p):  # loss-only and gradient calls alike
            with pytest.raises(L.KernelError) as err:
                lib.fs2_ge2e_contrast(a["emb"], a["n"], a["m"], a["d"], a["w"], a["b"], None,
                                      a["loss"], demb, demb, demb, a["ws"], a["ws_bytes"], 0)
                pytest.fail(f"{kw} was accepted")
            assert "fs2_ge2e_contrast" in str(err.value)


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_contrast_has_no_path_off_the_gpu(device):
    """A tensor off the GPU is refused before any kernel call."""
    import torch
    G = importlib.import_module(PKG + ".ge2e")
    crit = G.GE2ELoss(device, loss="contrast")
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(torch.empty(2, 2, 64, device=device), None, None)


def test_ge2e_loss_choice_is_checked_at_construction():
    G = importlib.import_module(PKG + ".ge2e")
    T = importlib.import_module(PKG + ".embedder_train")
    with pytest.raises(ValueError):
        G.GE2ELoss("meta", loss="bogus")
    with pytest.raises(ValueError):
        T.EmbedderTrainer(device="meta", n_utt=3, loss="bogus")
    assert G.GE2ELoss("meta").loss == "softmax"
    crit = G.GE2ELoss("meta", loss="contrast")
    assert crit.loss == "contrast" and sorted(crit.state_dict()) == ["b", "w"]
    assert T.EmbedderTrainer(device="meta", n_utt=3).loss == "softmax"
    tr = T.EmbedderTrainer(device="meta", n_utt=3, loss="contrast")
    assert tr.loss == tr.criterion.loss == "contrast"
    # a criterion passed in keeps its own choice
    tr = T.EmbedderTrainer(criterion=crit, device="meta", n_utt=3, loss="softmax")
    assert tr.criterion is crit and tr.loss == "contrast"
    # ... and one that names no loss at all is taken as it is
    import torch

    class Plain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor(10.0, device="meta"))
            self.b = torch.nn.Parameter(torch.tensor(-5.0, device="meta"))

    plain = T.EmbedderTrainer(criterion=Plain(), device="meta", n_utt=3)
    assert plain.loss is None and sorted(plain.state_dict()["ge2e"]) == ["b", "w"]
    # the checkpoint format does not know the loss: w and b only
    assert sorted(tr.state_dict()["ge2e"]) == ["b", "w"]
