"""Vocoder training on the GPU against the fp64 oracle of tests/vocoder_train_oracle.py.

No tolerance here is picked.  Every comparison allows 4 x the error that the SAME quantity has
when plain torch evaluates it in float32 on the CPU (against float64), computed here per case and
printed; 4 is the factor ``melspec_oracle.bounds`` uses.  For bf16 the operands are rounded to
bf16 before the oracle sees them (products of bf16 values are exact in the fp32 accumulator), and
the same rule applies.
"""
import importlib
import json
import math

import numpy as np
import pytest
import torch

import melspec_oracle as mo
import vocoder_train_oracle as VT

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("mid-attribute-speaker-generation_amd")
K = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
HG = importlib.import_module("mid-attribute-speaker-generation_amd.hifigan")
DEV = "cuda"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
HOP = 256

SMALL = {"upsample_initial_channel": 128, "upsample_rates": [2, 2], "upsample_kernel_sizes": [4, 4],
         "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5]] * 3}
TRAIN_H = dict(SMALL, upsample_rates=[16, 16], upsample_kernel_sizes=[32, 32])  # x256 = the hop
_CACHE = {}


def dev(t, dtype=None):
    t = torch.as_tensor(t)
    return t.to(DEV, dtype or t.dtype).contiguous()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def check(what, got, f32, f64):
    """|got - f64| <= 4 x max |f32 - f64|, figures printed first."""
    bound = VT.tol(f32, f64)
    err = float((got.detach().cpu().double() - f64.double()).abs().max())
    print(f"{what}: max |gpu - fp64| {err:.3e}, allowed {bound:.3e} (4 x the fp32 CPU error), "
          f"scale {float(f64.abs().max()):.3e}")
    assert math.isfinite(err) and err <= bound, (what, err, bound)


def front_end():
    if "fe" not in _CACHE:
        _CACHE["fe"] = importlib.import_module(
            "mid-attribute-speaker-generation_amd.audio").MelFrontEnd(PKG.config.load_configs("JVS-VCTK")[0])
    return _CACHE["fe"]


# ------------------------------------------------------------------ fs2_conv_wgrad_dil
WGRAD_CASES = [  # c_in, c_out, taps, dil, seq_len, utterances
    (80, 64, 7, 1, 96, 2),     # seq_len not a multiple of 64
    (32, 32, 11, 5, 16, 2),    # the 25-row radius exceeds the utterance
    (32, 32, 3, 3, 200, 2),
    (64, 64, 7, 3, 128, 2),
    (64, 256, 3, 1, 64, 2),    # the phase form
    (32, 32, 11, 5, 4096, 2),  # deep split: 8192 rows
]


def wgrad_problem(case, dtype):
    if (case, dtype) in _CACHE:
        return _CACHE[case, dtype]
    c_in, c_out, taps, dil, T, B = case
    g = torch.Generator().manual_seed(1000 * c_in + 10 * taps + dil + T)
    dy = torch.randn(B * T, c_out, generator=g)
    x = torch.randn(B * T, c_in, generator=g)
    dw0 = torch.randn(c_out, c_in, taps, generator=g)
    db0 = torch.randn(c_out, generator=g)
    if dtype == BF:
        dy, x = dy.to(BF).float(), x.to(BF).float()
    pad = (taps - 1) * dil // 2
    w64, b64 = VT.conv_wgrad(dy, x, T, taps, pad, dil, F64)
    w32, b32 = VT.conv_wgrad(dy, x, T, taps, pad, dil, F32)
    # the kernel accumulates: the quantity is dw0 + gradient, in fp32 on the yardstick's side
    ref = dict(dy=dy, x=x, dw0=dw0, db0=db0, pad=pad, w64=dw0.double() + w64, b64=db0.double() + b64,
               w32=dw0 + w32, b32=db0 + b32)
    _CACHE[case, dtype] = ref
    return ref


def run_wgrad(case, dtype, p, with_db=True):
    c_in, c_out, taps, dil, T, B = case
    dw, db = dev(p["dw0"]).clone(), dev(p["db0"]).clone() if with_db else None
    K.conv_wgrad_dil(dev(p["dy"], dtype), dev(p["x"], dtype), dw, B * T, T, c_in, c_out, taps,
                     p["pad"], dil, db=db)
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_dil(case, dtype):
    p = wgrad_problem(case, dtype)
    dw, db = run_wgrad(case, dtype, p)
    check(f"dw {case}", dw, p["w32"], p["w64"])
    check(f"db {case}", db, p["b32"], p["b64"])
    dw2, db2 = run_wgrad(case, dtype, p)
    assert torch.equal(bits(dw), bits(dw2)) and torch.equal(bits(db), bits(db2)), "not reproducible"
    dw3, _ = run_wgrad(case, dtype, p, with_db=False)  # db NULL: the same dw
    assert torch.equal(bits(dw), bits(dw3))


def test_conv_wgrad_dil_refusals():
    L = importlib.import_module("mid-attribute-speaker-generation_amd._lib")
    x = torch.zeros(64, 8, device=DEV)
    with pytest.raises(L.KernelError):  # taps > 11
        K.conv_wgrad_dil(x, x, torch.zeros(8, 8, 13, device=DEV), 64, 64, 8, 8, 13, 6)
    with pytest.raises(L.KernelError):  # pad past the taps' reach
        K.conv_wgrad_dil(x, x, torch.zeros(8, 8, 3, device=DEV), 64, 64, 8, 8, 3, 5, 2)


# ------------------------------------------------------------------ fs2_melspec_bwd, fs2_mel_l1
MEL_LENS = (2304, 2048, 700, 300)  # 700: reflection reaches deep; 300: the clamp at 0 is active


def mel_problem():
    if "mel" in _CACHE:
        return _CACHE["mel"]
    S = max(MEL_LENS)
    Fm = mo.n_frames(S, HOP)
    g = torch.Generator().manual_seed(7)
    wav = np.zeros((len(MEL_LENS), S), np.float32)
    for b, n in enumerate(MEL_LENS):
        wav[b, :n] = mo.fixture(n, seed=20 + b)
    d_mel = torch.randn(len(MEL_LENS), 80, Fm, generator=g)
    rows = []
    for b, n in enumerate(MEL_LENS):
        nf = mo.n_frames(n, HOP)
        out = {}
        for dt in (F32, F64):
            x = torch.from_numpy(wav[b, :n]).to(dt).requires_grad_(True)
            (VT.mel(x, HOP) * d_mel[b, :, :nf].to(dt)).sum().backward()
            out[dt] = x.grad
        rows.append(out)
    _CACHE["mel"] = (wav, d_mel, rows)
    return _CACHE["mel"]


def run_melspec_bwd(wav, lens, d_mel):
    window, twiddle, fb = front_end()._dev_tables()
    out = torch.full(wav.shape, float("nan"), device=DEV)
    K.melspec_bwd(dev(wav), dev(np.asarray(lens, np.int64)), dev(d_mel), HOP, window, twiddle, fb, 80,
                  out=out)
    torch.cuda.synchronize()
    return out.cpu()


def test_melspec_bwd_against_autograd():
    wav, d_mel, rows = mel_problem()
    got = run_melspec_bwd(wav, MEL_LENS, d_mel)
    for b, n in enumerate(MEL_LENS):
        check(f"d_wav, row of {n} samples", got[b, :n], rows[b][F32], rows[b][F64])
        assert torch.equal(got[b, n:], torch.zeros(wav.shape[1] - n)), "samples past len must be 0"


def test_melspec_bwd_is_batch_invariant():
    wav, d_mel, _ = mel_problem()
    got = run_melspec_bwd(wav, MEL_LENS, d_mel)
    order = [2, 0, 3, 1]
    again = run_melspec_bwd(wav[order], [MEL_LENS[i] for i in order], d_mel[order])
    for pos, b in enumerate(order):
        assert torch.equal(bits(again[pos]), bits(got[b])), f"row {b} changed with its place"
    single = run_melspec_bwd(wav[2:3], MEL_LENS[2:3], d_mel[2:3])
    assert torch.equal(bits(single[0]), bits(got[2]))


def test_mel_l1():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(3, 80, 9, generator=g), torch.randn(3, 80, 9, generator=g)
    b[0, :5] = a[0, :5]  # equal entries: zero gradient
    loss, d_a = K.mel_l1(dev(a), dev(b))
    f64 = VT.mel_l1(a.double(), b.double())
    check("mel_l1 loss", loss[0], VT.mel_l1(a, b), f64)
    n = a.numel()
    check("mel_l1 d_a", d_a, torch.sign(a - b) / n, torch.sign(a.double() - b.double()) / n)
    loss2, _ = K.mel_l1(dev(a), dev(b))
    assert torch.equal(bits(loss), bits(loss2))


def test_mel_loss_autograd():
    VTR = importlib.import_module("mid-attribute-speaker-generation_amd.vocoder_train")
    fe = front_end()
    seg = np.stack([mo.fixture(2048, seed=s) for s in (41, 42)])
    tgt = np.stack([mo.fixture(2048, seed=s, kind="tone7600") for s in (43, 44)])
    res = {}
    for dt in (F32, F64):
        x = torch.from_numpy(seg).to(dt).requires_grad_(True)
        loss = VT.mel_l1(VT.mel_batch(x, HOP), VT.mel_batch(torch.from_numpy(tgt).to(dt), HOP))
        loss.backward()
        res[dt] = (loss.detach(), x.grad)
    target = fe(dev(tgt))[0]
    x = dev(seg).requires_grad_(True)
    loss = VTR.MelLoss(fe)(x, target)
    loss.backward()
    # the device target is itself an fp32 evaluation: its own error is part of the yardstick
    check("MelLoss", loss, res[F32][0], res[F64][0])
    check("MelLoss d_wav", x.grad, res[F32][1], res[F64][1])


# ------------------------------------------------------------------ head, fold, lrelu_bwd
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_vocoder_post_bwd(dtype):
    g = torch.Generator().manual_seed(11)
    C, T, B = 32, 200, 3  # 600 rows: blocks of 128 span utterances, the last is partial
    x = torch.randn(B * T, C, generator=g)
    if dtype == BF:
        x = x.to(BF).float()
    w = torch.randn(C * 7, generator=g) * 0.05
    b = torch.randn(1, generator=g) * 0.1
    d_wav = torch.randn(B * T, generator=g)
    r64, r32 = VT.head(x, w, b, d_wav, T, F64), VT.head(x, w, b, d_wav, T, F32)
    dw0, db0 = torch.randn(C * 7, generator=g), torch.randn(1, generator=g)
    dw, db = dev(dw0).clone(), dev(db0).clone()
    # the saved wav is the oracle's fp32 one, so only the backward is under test
    dx = K.vocoder_post_bwd(dev(x, dtype), dev(r32[0]), dev(d_wav), B * T, T, C, dev(w), dw, db)
    w32 = VT.head(x, w, b, d_wav, T, F32)
    check("head dx", dx, w32[1], r64[1])
    check("head dw", dw, dw0 + w32[2], dw0.double() + r64[2])
    check("head db", db, db0 + w32[3], db0.double() + r64[3])
    dw2, db2 = dev(dw0).clone(), dev(db0).clone()
    K.vocoder_post_bwd(dev(x, dtype), dev(r32[0]), dev(d_wav), B * T, T, C, dev(w), dw2, db2)
    assert torch.equal(bits(dw), bits(dw2)) and torch.equal(bits(db), bits(db2))


@pytest.mark.parametrize("s", [2, 8])
def test_convT_wgrad_fold(s):
    g = torch.Generator().manual_seed(s)
    c_in, c_out = 24, 12
    dwc = torch.randn(s * c_out, c_in, 3, generator=g)
    dbc = torch.randn(s * c_out, generator=g)
    want_w, want_b = VT.fold(dwc.double(), dbc.double(), c_in, c_out, s)
    ref_w, ref_b = VT.fold(dwc, dbc, c_in, c_out, s)
    dw, db = torch.zeros(c_in, c_out, 2 * s, device=DEV), torch.zeros(c_out, device=DEV)
    K.convT_wgrad_fold(dev(dwc), dev(dbc), dw, db, s)
    assert torch.equal(dw.cpu(), ref_w), "the fold is a pure index map"
    check("fold db", db, ref_b, want_b)
    # ... and the inverse of fs2_convT_weight_prep
    w = torch.randn(c_in, c_out, 2 * s, generator=g)
    wc, _ = K.convT_weight_prep(dev(w), dev(torch.zeros(c_out)), s)
    assert torch.equal(wc.cpu(), VT.phase_weight(w, s))
    back = torch.zeros(c_in, c_out, 2 * s, device=DEV)
    K.convT_wgrad_fold(wc, None, back, None, s)
    assert torch.equal(back.cpu(), w)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_lrelu_bwd(dtype):
    g = torch.Generator().manual_seed(5)
    v = torch.randn(1000, 3, generator=g)
    v[::7] = 0.0  # torch's convention at 0: the slope alpha
    v[1::7, 0] = -0.0
    if dtype == BF:
        v = v.to(BF).float()
    dy = torch.randn(1000, 3, generator=g)
    for alpha in (0.1, 0.01):
        want, ref = VT.lrelu_bwd(v, dy, alpha, F64), VT.lrelu_bwd(v, dy, alpha, F32)
        got = K.lrelu_bwd(dev(v, dtype), dev(dy), alpha)
        check(f"lrelu_bwd {alpha}", got, ref, want)
        # the leaky-ReLU'd copy has the same sign: the same result from it
        copy = torch.nn.functional.leaky_relu(v, alpha)
        if dtype == BF:
            copy = copy.to(BF).float()
        assert torch.equal(bits(K.lrelu_bwd(dev(copy, dtype), dev(dy), alpha)), bits(got))
        base = torch.randn(1000, 3, generator=g)
        acc = K.lrelu_bwd(dev(v, dtype), dev(dy), alpha, out=dev(base).clone(), accumulate=True)
        check(f"lrelu_bwd {alpha} accumulate", acc, base + ref, base.double() + want)


# ------------------------------------------------------------------ the whole generator
def make_generator(h, sd64, dtype=F32):
    gen = HG.Generator(HG.AttrDict(h), device=DEV, compute_dtype=dtype)
    gen.load_state_dict({k: v.float() for k, v in sd64.items()})
    return gen


def generator_case(h, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    sd64 = {k: v.float().double() for k, v in VT.init_state(h, seed=seed).items()}
    mel = torch.randn(B, 80, T, generator=g).double()
    up = math.prod(h["upsample_rates"])
    cot = torch.randn(B, T * up, generator=g).double()
    r64 = VT.generator_grads(sd64, h, mel, cot, F64)
    r32 = VT.generator_grads(sd64, h, mel, cot, F32)
    gen = make_generator(h, sd64)
    rows = dev(mel.float().transpose(1, 2).reshape(B * T, 80)).requires_grad_(True)
    wav = gen.forward_train(rows, B, T)
    wav.backward(dev(cot.float()).reshape(-1))
    torch.cuda.synchronize()
    check("waveform", wav.view(B, -1), r32[0], r64[0])
    wav_rows, _ = gen.forward_rows(rows.detach(), B, T, pcm=False)
    diff, bound = float((wav.detach() - wav_rows).abs().max()), VT.tol(r32[0], r64[0])
    print(f"forward_train vs forward_rows: max |diff| {diff:.3e}, allowed {bound:.3e}")
    assert diff <= bound
    # fp32 mode: the same launches conv by conv, so in fact the same bits
    assert torch.equal(bits(wav), bits(wav_rows))
    for name, p in gen.named_parameters():
        assert p.grad is not None, name
        check(name, p.grad, r32[1][name], r64[1][name])
    d_mel = rows.grad.view(B, T, 80).transpose(1, 2)
    check("d_mel", d_mel, r32[2], r64[2])


def test_generator_small_config():
    generator_case(SMALL, B=2, T=8, seed=0)


def test_generator_bundled_config():
    generator_case(dict(HG.load_config()), B=1, T=4, seed=1)


MANY_TILES = {"upsample_initial_channel": 64, "upsample_rates": [2], "upsample_kernel_sizes": [4],
              "resblock_kernel_sizes": [3, 11], "resblock_dilation_sizes": [[1, 3, 5]] * 2}


def test_generator_many_row_tiles():
    """32 channels over 2 x 16384 = 32768 rows: every conv of the resblocks is hundreds of row
    tiles, launched as independent blocks that read their neighbours' rows as halo (25 rows at
    k = 11, d = 5).  A data gradient written over its own input passes at one-tile shapes and
    not here."""
    generator_case(MANY_TILES, B=2, T=8192, seed=3)


def test_generator_bf16_mode_runs_and_tracks_fp32():
    """A smoke check, not a parity test: the bf16 kernels are held to the yardstick one by one
    above, and no whole-generator oracle with bf16-rounded operands exists to take a bound from.
    bf16 compute, fp32 masters: gradients arrive for every parameter and point the fp32 way.
    The bound is reasoned, not measured: each of the ~40 conv operands on a path (forward
    copies and cast gradients) is rounded to 8 bits, relative error 2^-9 each, adding
    incoherently to about sqrt(40) 2^-9 = 1.2e-2 of the gradient's norm; the cosine of two
    vectors e apart is 1 - e^2 / 2 = 0.9999.  0.98 is e = 0.2, some sixteen times that (room for
    leaky-ReLU signs that flip under rounding); a wrong kernel gives no correlation at all."""
    g = torch.Generator().manual_seed(2)
    sd64 = VT.init_state(SMALL, seed=2)
    mel = torch.randn(2, 8, 80, generator=g).reshape(16, 80)
    cot = torch.randn(2 * 8 * 4, generator=g)
    grads = {}
    for dt in (F32, BF):
        gen = make_generator(SMALL, sd64, dt)
        gen.forward_train(dev(mel), 2, 8).backward(dev(cot))
        grads[dt] = torch.cat([p.grad.reshape(-1) for p in gen.parameters()]).double()
    cos = float(torch.dot(grads[F32], grads[BF]) / (grads[F32].norm() * grads[BF].norm()))
    print(f"bf16 vs fp32 gradient cosine {cos:.5f}")
    assert cos > 0.98


# ------------------------------------------------------------------ trainer, checkpoint
def trainer_and_segments():
    VTR = importlib.import_module("mid-attribute-speaker-generation_amd.vocoder_train")
    sd64 = {k: v.float().double() for k, v in VT.init_state(TRAIN_H, seed=4).items()}
    seg = np.stack([mo.fixture(2048, seed=s) for s in (51, 52)])
    gen = make_generator(TRAIN_H, sd64)
    return VTR, VTR.VocoderTrainer(gen, front_end()), sd64, seg


def test_three_optimiser_steps_follow_the_oracle():
    VTR, tr, sd64, seg = trainer_and_segments()
    store = VTR.WaveStore([seg[0], seg[1]], DEV)
    batch = store.gather(store.offsets, 2048)  # the fixed batch, through fs2_wave_segments
    assert torch.equal(batch.cpu(), torch.from_numpy(seg))
    got = [float(tr.step(batch)[0]) for _ in range(3)]
    segs = torch.from_numpy(seg).double()
    t64 = VT.adam_trajectory(sd64, TRAIN_H, segs, HOP, 3, VTR.LR, VTR.BETAS, VTR.EPS, F64)
    t32 = VT.adam_trajectory(sd64, TRAIN_H, segs, HOP, 3, VTR.LR, VTR.BETAS, VTR.EPS, F32)
    for i in range(3):
        check(f"loss of step {i + 1}", torch.tensor(got[i]), torch.tensor(t32[i]),
              torch.tensor(t64[i], dtype=F64))
    assert got[2] < got[0]


def test_checkpoint_round_trip(tmp_path):
    VTR, tr, _, seg = trainer_and_segments()
    tr.step(dev(seg))
    ckpt, conf = str(tmp_path / "g.pth.tar"), str(tmp_path / "hifigan.json")
    tr.save(ckpt)
    with open(conf, "w") as f:
        json.dump(TRAIN_H, f)
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert sd["steps"] == 1 and not any(k.endswith(("weight_g", "weight_v")) for k in sd["generator"])
    loaded = HG.get_vocoder(config=conf, device=DEV, ckpt=ckpt, compute_dtype=F32)
    rows = dev(torch.randn(2 * 8, 80, generator=torch.Generator().manual_seed(9)))
    a, _ = tr.gen.forward_rows(rows, 2, 8, pcm=False)
    b, _ = loaded.forward_rows(rows, 2, 8, pcm=False)
    assert torch.equal(bits(a), bits(b))
