"""``lstm_oracle`` (the float64 restatement the discriminator kernel tests compare with)
against torch on the CPU in float64: ``nn.LSTM`` with autograd for the stack and the
per-layer ``dgates``, autograd for the head with explicit masks, ``contrast_oracle``'s
``torch_embedder`` for the whole module, and ``chunk_mels``' documented chunking for
``repad``.  No GPU and no project kernel runs here."""
import importlib

import numpy as np
import pytest
import torch

import lstm_oracle as lo
from contrast_oracle import torch_embedder

D = 80
TOL = 1e-12  # of the reference tensor's max-abs: float64 with another summation order


def _close(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err, peak = np.abs(got - want).max(), np.abs(want).max()
    print(f"{tag}: err {err:.3e} peak {peak:.3e}")
    assert err <= TOL * peak, (tag, err, peak)


_CASES = {}


def _case(N, T, H, L):
    """The oracle and nn.LSTM(...).double() with autograd on the same weights, once a shape."""
    key = (N, T, H, L)
    if key in _CASES:
        return _CASES[key]
    gen = torch.Generator().manual_seed(100 + N + T)
    ref = torch.nn.LSTM(D, H, num_layers=L, batch_first=True).double()
    with torch.no_grad():
        for prm in ref.parameters():
            prm.copy_(torch.randn(prm.shape, generator=gen, dtype=torch.float64) * 0.1)
    W = lambda n: getattr(ref, n).detach().numpy()  # noqa: E731
    w_ih_up = np.stack([W(f"weight_ih_l{l}") for l in range(1, L)]) if L > 1 else None
    w_hh = np.stack([W(f"weight_hh_l{l}") for l in range(L)])
    bias = np.stack([W(f"bias_ih_l{l}") + W(f"bias_hh_l{l}") for l in range(L)])
    x = torch.randn(N, T, D, generator=gen, dtype=torch.float64)
    dh = torch.randn(N, T, H, generator=gen, dtype=torch.float64) * 0.1
    got = lo.lstm_stack(x.numpy(), (W("weight_ih_l0"), w_ih_up), w_hh, bias, dh.numpy())
    xr = x.clone().requires_grad_()
    out, (hn, cn) = ref(xr)
    out.backward(dh)
    _CASES[key] = (got, x.numpy(), ref, out.detach().numpy(), hn.detach().numpy(),
                   cn.detach().numpy(), xr.grad.numpy())
    return _CASES[key]


SHAPES = [(5, 1, 256, 3), (3, 2, 256, 3), (4, 7, 256, 1), (2, 5, 512, 2)]


@pytest.mark.parametrize("N,T,H,L", SHAPES)
def test_stack_matches_torch_lstm_float64(N, T, H, L):
    got, _, _, out, hn, cn, dx = _case(N, T, H, L)
    assert got["h"].dtype == np.float64 and got["h"].shape == (L, N, T, H)
    assert got["act"].shape == got["dgates"].shape == (L, N, T, 4 * H)
    _close(got["h"][L - 1], out, "h (top layer)")
    _close(got["h"][:, :, -1], hn, "last-step h per layer")
    _close(got["c"][:, :, -1], cn, "last-step c per layer")
    _close(got["dx"], dx, "dx")


@pytest.mark.parametrize("N,T,H,L", SHAPES)
def test_stack_dgates_reproduce_autograd_weight_gradients(N, T, H, L):
    """dW_ih = sum dgates^T (x) input, dW_hh = sum dgates_t^T (x) h_{t-1}, db = sum dgates:
    wrong per-layer dgates could not give autograd's weight gradients."""
    got, x, ref, *_ = _case(N, T, H, L)
    for l in range(L):
        dg = got["dgates"][l]
        below = x if l == 0 else got["h"][l - 1]
        G = lambda n: getattr(ref, f"{n}_l{l}").grad.numpy()  # noqa: E731
        _close(np.einsum("ntg,ntk->gk", dg, below), G("weight_ih"), f"dW_ih[{l}]")
        _close(np.einsum("ntg,ntk->gk", dg[:, 1:], got["h"][l][:, :-1]), G("weight_hh"),
               f"dW_hh[{l}]")
        _close(dg.sum(axis=(0, 1)), G("bias_ih"), f"db_ih[{l}]")
        _close(dg.sum(axis=(0, 1)), G("bias_hh"), f"db_hh[{l}]")


def test_stack_without_top_gradient_is_zero():
    N, T, H, L = 3, 2, 256, 3
    got, x, ref, *_ = _case(N, T, H, L)
    W = lambda n: getattr(ref, n).detach().numpy()  # noqa: E731
    none = lo.lstm_stack(
        x, (W("weight_ih_l0"), np.stack([W(f"weight_ih_l{l}") for l in range(1, L)])),
        np.stack([W(f"weight_hh_l{l}") for l in range(L)]),
        np.stack([W(f"bias_ih_l{l}") + W(f"bias_hh_l{l}") for l in range(L)]), None)
    assert np.array_equal(none["h"], got["h"]) and np.array_equal(none["act"], got["act"])
    assert not none["dgates"].any() and not none["dx"].any()


def _head_weights(gen, d=256):
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64) * 0.2  # noqa: E731
    return {"wp": mk(64, d), "bp": mk(64), "w0": mk(64, 64), "b0": mk(64), "w1": mk(64, 64),
            "b1": mk(64), "w2": mk(1, 64), "b2": mk(1)}


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("which", ["demb", "dlogit", "both"])
def test_head_matches_torch_autograd_with_explicit_masks(p, which):
    n = 9
    gen = torch.Generator().manual_seed(7)
    w = _head_weights(gen)
    x = torch.randn(n, 256, generator=gen, dtype=torch.float64)
    keep = lambda: ((torch.rand(n, 64, generator=gen) >= p).double() / (1 - p))  # noqa: E731
    m0, m1 = keep(), keep()
    if p > 0:
        assert 0 < (m0 == 0).sum() < m0.numel()
    demb = torch.randn(n, 64, generator=gen, dtype=torch.float64) if which != "dlogit" else None
    dlogit = torch.randn(n, generator=gen, dtype=torch.float64) if which != "demb" else None
    got = lo.clf_head(x.numpy(), {k: v.numpy() for k, v in w.items()}, m0.numpy(), m1.numpy(),
                      None if demb is None else demb.numpy(),
                      None if dlogit is None else dlogit.numpy())
    xr = x.clone().requires_grad_()
    pr = xr @ w["wp"].t() + w["bp"]
    e = pr / pr.norm(dim=1, keepdim=True)
    a0 = torch.relu((e @ w["w0"].t() + w["b0"]) * m0)
    a1 = torch.relu((a0 @ w["w1"].t() + w["b1"]) * m1)
    logit = (a1 @ w["w2"].t() + w["b2"]).squeeze(1)
    loss = 0
    if demb is not None:
        loss = loss + (e * demb).sum()
    if dlogit is not None:
        loss = loss + (logit * dlogit).sum()
    loss.backward()
    _close(got["emb"], e.detach().numpy(), "emb")
    _close(got["logit"], logit.detach().numpy(), "logit")
    _close(got["dx"], xr.grad.numpy(), "dx")
    assert np.abs(np.linalg.norm(got["emb"], axis=1) - 1).max() < 1e-14


def test_stack_and_head_equal_the_torch_embedder():
    """The oracle's stack feeding its head (masks of ones) is ``torch_embedder`` over the
    module's own seeded parameters, in float64."""
    PKG = importlib.import_module("mid-attribute-speaker-generation_amd")
    G = importlib.import_module("mid-attribute-speaker-generation_amd.ge2e")
    m = PKG.seeded.load_seeded_(G.SpeechEmbedder(device="cpu")).double()
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(5, 4, D, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        e, logits = torch_embedder(m, x)
    W = lambda n: getattr(m.LSTM_stack, n).detach().numpy()  # noqa: E731
    st = lo.lstm_stack(x.numpy(),
                       (W("weight_ih_l0"), np.stack([W(f"weight_ih_l{l}") for l in (1, 2)])),
                       np.stack([W(f"weight_hh_l{l}") for l in range(3)]),
                       np.stack([W(f"bias_ih_l{l}") + W(f"bias_hh_l{l}") for l in range(3)]), None)
    lin = m._head_layers()
    w = {}
    for name, layer in zip(("p", "0", "1", "2"), lin):
        w["w" + name] = layer.weight.detach().numpy()
        w["b" + name] = layer.bias.detach().numpy()
    ones = np.ones((5, 64))
    got = lo.clf_head(st["h"][2][:, -1], w, ones, ones, None, None)
    _close(got["emb"], e.numpy(), "embeddings")
    _close(got["logit"], logits.numpy(), "logits")
    assert not got["dx"].any()


def test_bce_rows_and_gradient_match_torch():
    x = torch.tensor([0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4,
                      0.7, -2.5], dtype=torch.float64)
    for t in (0.0, 1.0, 0.3):
        y = torch.full_like(x, t)
        xr = x.clone().requires_grad_()
        rows = torch.nn.functional.binary_cross_entropy_with_logits(xr, y, reduction="none")
        (rows.sum() * 0.37 * 2.5).backward()
        got, dgot = lo.bce_rows(x.numpy(), y.numpy()), lo.dbce(x.numpy(), y.numpy(), 0.37, 2.5)
        assert np.isfinite(got).all() and np.isfinite(dgot).all()
        _close(got, rows.detach().numpy(), f"bce rows, target {t}")
        assert np.abs(dgot - xr.grad.numpy()).max() <= 1e-15


@pytest.mark.parametrize("T", [149, 150, 151, 300])
def test_repad_is_the_documented_chunking(T):
    """``chunk_mels``: (B, T, 80) -> (B * (T // 150 + 1), 150, 80), zero-padded, a full zero
    chunk when T is a multiple of 150."""
    B, C, chunk = 2, 80, 150
    x = np.random.default_rng(T).standard_normal((B, T, C)).astype(np.float32) + 3.0
    r = T // chunk + 1
    assert r == {149: 1, 150: 2, 151: 2, 300: 3}[T]
    y = lo.repad(x, r * chunk)
    assert y.dtype == x.dtype and y.shape == (B, r * chunk, C)
    chunks = y.reshape(B * r, chunk, C)
    for b in range(B):
        for k in range(r):
            want = np.zeros((chunk, C), np.float32)
            part = x[b, k * chunk:(k + 1) * chunk]
            want[:len(part)] = part
            assert np.array_equal(chunks[b * r + k], want)
        if T % chunk == 0:
            assert not chunks[b * r + r - 1].any() and chunks[b * r + r - 2].all()
    # the gradient's direction: truncation back to T frames undoes the padding
    assert np.array_equal(lo.repad(y, T), x)


def test_repeat_col():
    meta = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert lo.repeat_col(meta, 2, 3).tolist() == [2, 2, 2, 6, 6, 6, 10, 10, 10]
    assert lo.repeat_col(meta, 0, 1).tolist() == [0, 4, 8]
