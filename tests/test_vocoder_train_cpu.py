"""tests/vocoder_train_oracle.py checked on the CPU, and the built library's new exports."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import melspec_oracle as mo
import vocoder_oracle as VO
import vocoder_train_oracle as VT

F64 = torch.float64
SMALL = {"upsample_initial_channel": 128, "upsample_rates": [2, 2], "upsample_kernel_sizes": [4, 4],
         "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5]] * 3}

NEW_SYMBOLS = (
    "fs2_conv_wgrad_dil_ws_bytes", "fs2_conv_wgrad_dil", "fs2_lrelu_bwd",
    "fs2_vocoder_post_bwd_ws_bytes", "fs2_vocoder_post_bwd", "fs2_convT_wgrad_fold",
    "fs2_melspec_bwd_ws_bytes", "fs2_melspec_bwd", "fs2_mel_l1_ws_bytes", "fs2_mel_l1")


def test_library_exports_new_symbols():
    """The header declares them and the built library defines them (binding is by header)."""
    L = importlib.import_module("mid-attribute-speaker-generation_amd._lib")
    declared = L.parse_header()
    assert os.path.exists(L.LIB_PATH), "build() has not run"
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/fs2hip.h"
        assert hasattr(dll, name), f"{name} is not exported by {L.LIB_PATH}"
    assert L.lib.fs2_abi_version() == 1


@pytest.mark.parametrize("length,kind", [(2304, "speech"), (2048, "tone7600"), (700, "speech")])
def test_mel_equals_oracle64(length, kind):
    x = mo.fixture(length, seed=3, kind=kind)
    got = VT.mel(torch.from_numpy(x.astype(np.float64)), 256).numpy()
    want = mo.oracle64(x, 256)[1]
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-9


def test_reflect_index_clamps_short_rows():
    """Below the padding the second reflection falls under 0 and is clamped there."""
    idx = VT.reflect_index(np.arange(-512, 1024), 300)
    assert idx.min() == 0 and idx.max() == 299
    assert idx[512 - 100] == 100 and idx[512 + 400] == 2 * 299 - 400 and idx[512 + 700] == 0


@pytest.mark.parametrize("length", [700, 300])
def test_mel_gradient_matches_finite_differences(length):
    g = torch.Generator().manual_seed(length)
    x = torch.from_numpy(mo.fixture(length, seed=5).astype(np.float64))
    cot = torch.randn(80, mo.n_frames(length, 256), generator=g, dtype=F64)
    xv = x.clone().requires_grad_(True)
    (VT.mel(xv, 256) * cot).sum().backward()
    f = lambda v: float((VT.mel(v, 256) * cot).sum())  # noqa: E731
    eps = 1e-6
    for t in (0, 1, 2, 37, length // 2, length - 2, length - 1):
        e = torch.zeros_like(x)
        e[t] = eps
        fd = (f(x + e) - f(x - e)) / (2 * eps)
        assert abs(fd - float(xv.grad[t])) <= 1e-5 * max(1.0, abs(fd)), (t, fd, float(xv.grad[t]))


def test_generator_pieces_agree_with_vocoder_oracle():
    """ResBlock1 and the head against tests/vocoder_oracle.py (its fp32-free, fp64 settings)."""
    g = torch.Generator().manual_seed(1)
    C, k, dil, B, T = 32, 7, (1, 3, 5), 2, 48
    sd = VT.init_state(SMALL, seed=2)
    x = torch.randn(B * T, C, generator=g, dtype=F64)
    names = [f"resblocks.3.{c}.{m}" for c in ("convs1", "convs2") for m in range(3)]
    assert sd[names[0] + ".weight"].shape == (C, C, 3)
    w = {n: torch.randn(C, C, k, generator=g, dtype=F64) * 0.05 for n in names}
    rb = {n + ".weight": w[n] for n in names}
    rb.update({n + ".bias": sd[n + ".bias"] for n in names})
    got = VT.resblock(rb, 3, k, dil, x.view(B, T, C).transpose(1, 2)).transpose(1, 2).reshape(B * T, C)
    want, _ = VO.resblock1(x.float(), [w[n] for n in names[:3]], [w[n] for n in names[3:]],
                           [rb[n + ".bias"] for n in names[:3]], [rb[n + ".bias"] for n in names[3:]],
                           k, dil, T=T, bf16=False)
    # vocoder_oracle rounds the residual stream to fp32 after every pair
    assert (got - want.double()).abs().max() < 1e-5 * max(1.0, float(got.abs().max()))
    pw = torch.randn(1, C, 7, generator=g, dtype=F64) * 0.1
    pb = torch.randn(1, generator=g, dtype=F64)
    wav, _, _, _ = VT.head(x, pw.reshape(-1), pb, torch.ones(B * T, dtype=F64), T, F64)
    want_wav, _, _ = VO.conv_post(x, pw, pb, T=T, max_wav=32768.0)
    assert (wav - want_wav).abs().max() < 1e-12


def test_generator_shape_and_grad_keys():
    sd = VT.init_state(SMALL, seed=0)
    mel = torch.randn(2, 80, 8, dtype=F64)
    wav, grads, d_mel = VT.generator_grads(sd, SMALL, mel, torch.randn(2, 32, dtype=F64), F64)
    assert wav.shape == (2, 32) and d_mel.shape == mel.shape
    assert set(grads) == set(sd) and all(grads[k].shape == sd[k].shape for k in sd)
    assert float(wav.abs().max()) < 1.0


@pytest.mark.parametrize("s", [2, 8])
def test_fold_round_trips_conv_transpose(s):
    g = torch.Generator().manual_seed(s)
    c_in, c_out, B, T = 6, 4, 2, 9
    x = torch.randn(B, c_in, T, generator=g, dtype=F64)
    w = torch.randn(c_in, c_out, 2 * s, generator=g, dtype=F64, requires_grad=True)
    b = torch.randn(c_out, generator=g, dtype=F64, requires_grad=True)
    cot = torch.randn(B, c_out, T * s, generator=g, dtype=F64)
    y = F.conv_transpose1d(x, w, b, stride=s, padding=s // 2)
    (y * cot).sum().backward()
    wc = VT.phase_weight(w.detach(), s).requires_grad_(True)
    bc = b.detach().repeat(s).requires_grad_(True)
    yc = VT.phase_conv(x, wc, bc, s)
    assert (yc - y).abs().max() < 1e-12
    (yc * cot).sum().backward()
    dw, db = VT.fold(wc.grad, bc.grad, c_in, c_out, s)
    assert (dw - w.grad).abs().max() < 1e-12 and (db - b.grad).abs().max() < 1e-12
    # every target element has exactly one source: folding the prepared weight gives it back
    assert torch.equal(VT.fold(VT.phase_weight(w.detach(), s), None, c_in, c_out, s)[0], w.detach())


def test_adam_trajectory_descends():
    seg = torch.from_numpy(np.stack([mo.fixture(1024, seed=s) for s in (1, 2)]).astype(np.float64))
    h = dict(SMALL, upsample_rates=[16, 16], upsample_kernel_sizes=[32, 32])
    losses = VT.adam_trajectory(VT.init_state(h, seed=0), h, seg, 256, 3, 2e-4, (0.8, 0.99), 1e-8, F64)
    assert len(losses) == 3 and losses[2] < losses[0]
