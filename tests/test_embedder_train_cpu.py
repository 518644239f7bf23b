"""Speaker-encoder training, the parts that need no GPU: the fp64 closed form of the GE2E
softmax loss against the reference's own fp32 results (g14), the fixture's trajectories, and
the trainer's checkpoint layout."""
import importlib

import numpy as np
import pytest

from conftest import load_golden
from embedder_oracle import ge2e_softmax

CASES = ((3, 3), (4, 2), (2, 5))


@pytest.mark.parametrize("k", range(3))
def test_closed_form_reproduces_reference_loss_cases(k):
    g = load_golden("g14_embedder_train.npz")
    e = g[f"loss{k}.emb"]
    assert e.shape == CASES[k] + (64,)
    loss, demb, dw, db = ge2e_softmax(e)
    assert abs(loss - float(g[f"loss{k}.loss"])) <= 1e-5 * abs(float(g[f"loss{k}.loss"]))
    ref = g[f"loss{k}.demb"]
    assert np.abs(demb - ref).max() <= 1e-5 * np.abs(ref).max()
    assert abs(dw - float(g[f"loss{k}.dw"])) <= 1e-5 * abs(float(g[f"loss{k}.dw"]))
    assert abs(db - float(g[f"loss{k}.db"])) <= 1e-6


def test_fixture_trajectories():
    g = load_golden("g14_embedder_train.npz")
    for tag, steps in (("shipped", 3), ("ge2e", 3), ("da_only", 2)):
        s = g[f"{tag}.scalars"]
        assert s.shape == (steps, 5) and np.isfinite(s).all()
    assert (g["shipped.scalars"][:, 3] == 0).all()  # loss.backward is commented out: w, b idle
    assert (g["ge2e.scalars"][:, 3] > 0).all()
    # the issue's step-0 values of this recipe
    np.testing.assert_allclose(g["shipped.scalars"][0, [0, 1, 2, 4]],
                               [11.7655, 6.19792, 2.00043, 1.92205], rtol=2e-5)
    # the device gate is exercised: progress is past da_startpoint and every da_loss is below
    # the threshold by far more than fp32 rounding
    assert float(g["progress"]) > 0
    for tag in ("shipped", "ge2e"):
        assert (g[f"{tag}.gate"] == 1).all()
        assert (g[f"{tag}.scalars"][:, 1] < float(g["threshold"]) * (1 - 1e-3)).all()


def test_trainer_checkpoint_layout_matches_reference():
    g = load_golden("g14_embedder_train.npz")
    T = importlib.import_module("mid-attribute-speaker-generation_amd.embedder_train")
    tr = T.EmbedderTrainer(device="meta", n_utt=3)
    sd = tr.state_dict()
    assert sorted(sd) == ["embedder_net", "ge2e"]
    want = {k: tuple(int(x) for x in s.split(",")) for k, s in zip(g["sd.keys"], g["sd.shapes"])}
    assert {k: tuple(v.shape) for k, v in sd["embedder_net"].items()} == want
    assert list(sd["ge2e"]) == list(g["ge2e.keys"])
    assert all(v.shape == () for v in sd["ge2e"].values())
    # parameter sets of the three optimisers (speech_embedder_net.py:97-101)
    e = tr.embedder
    assert len(e.main_parameters()) == 14 and len(e.da_parameters()) == 6
    ids = {id(p) for p in e.main_parameters()} | {id(p) for p in e.da_parameters()}
    assert ids == {id(p) for p in e.parameters()}


def test_trainer_optimisers_and_anneal():
    """train_speech_embedder.py:104-113 and lr_schedule (83-95, 207): lr 1e-3 everywhere, L2
    1e-6 on main and da only; the anneal epochs halve main and ge2e, never da."""
    T = importlib.import_module("mid-attribute-speaker-generation_amd.embedder_train")
    tr = T.EmbedderTrainer(device="meta", n_utt=3)
    o = tr.optimizers
    assert [o[k].lr for k in ("main", "ge2e", "da")] == [1e-3] * 3
    assert [o[k].weight_decay for k in ("main", "ge2e", "da")] == [1e-6, 0.0, 1e-6]
    assert o["main"].arena.numel == sum(p.numel() for p in tr.embedder.main_parameters())
    for epoch in range(0, 2400, 100):
        tr.anneal(epoch)
    assert o["main"].lr == o["ge2e"].lr == 1e-3 / 16 and o["da"].lr == 1e-3


def test_new_entries_validate_arguments_before_any_launch():
    """FS2_ERR_ARG paths return before a stream is touched, so they run without a GPU: hidden a
    multiple of 256, steps and n_seq >= 1, beta in {0, 1}, the workspace size, and M >= 2."""
    L = importlib.import_module("mid-attribute-speaker-generation_amd._lib")
    lib, p = L.lib, 16  # a non-null, 16-byte aligned placeholder: never dereferenced
    big = 1 << 30
    assert lib.fs2_lstm_stack_wgrad_ws_bytes(1, 1, 80, 256, 3) == 3 * 1024 * (512 + 1) * 4
    assert lib.fs2_lstm_stack_wgrad_ws_bytes(0, 1, 80, 256, 3) == 0
    assert lib.fs2_ge2e_softmax_ws_bytes(3, 3, 64) > 0 and lib.fs2_clf_head_wgrad_ws_bytes(9) > 0
    bad = [dict(hidden=128), dict(steps=0), dict(n_seq=0), dict(beta=2), dict(c_in=82),
           dict(ws_bytes=8)]
    for kw in bad:
        a = dict(n_seq=1, steps=1, c_in=80, hidden=256, beta=0, ws_bytes=big)
        a.update(kw)
        with pytest.raises(L.KernelError):
            lib.fs2_lstm_stack_wgrad(p, p, p, a["n_seq"], a["steps"], a["c_in"], a["hidden"], 3, p,
                                     p, p, p, a["beta"], p, a["ws_bytes"], 0)
    with pytest.raises(L.KernelError):  # M = 1: the exclude-self centroid divides by 0
        lib.fs2_ge2e_softmax(p, 3, 1, 64, p, p, None, p, None, None, None, p, big, 0)
    with pytest.raises(L.KernelError):
        lib.fs2_ge2e_softmax(p, 3, 3, 257, p, p, None, p, None, None, None, p, big, 0)


def test_contrast_loss_stays_unbuilt():
    import torch
    G = importlib.import_module("mid-attribute-speaker-generation_amd.ge2e")
    with pytest.raises(NotImplementedError):
        G.GE2ELoss("meta", loss="contrast")(torch.empty(2, 2, 64, device="meta"), None, None)
