"""Frame-level pitch / energy on the GPU (model/modules.py:116-148, model/loss.py:51-63):

1. fs2_lr_expand_embed_fwd against the four launches it fuses, bitwise;
2. fs2_fs2loss_level_fwd / _bwd against torch autograd on masked_select;
3. three training steps against the reference's own (g12_*), fp32 and bf16;
4. every forward tensor and parameter gradient of one step against the CPU oracle;
5. the eval-mode forward against the reference's (g13);
6. bitwise repeatability, and the phoneme-level step unchanged from the parent commit.

Tolerances are test_gpu_parity.py's: 1e-4 of a tensor's scale in fp32 (north_star), its bf16
row for bf16; index tensors, masks and lengths exact.
"""
import importlib

import numpy as np
import pytest
import torch

import frame_level_oracle as flo
from conftest import load_golden
from oracle import fs2_cpu

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("mid-attribute-speaker-generation_amd")
M = importlib.import_module("mid-attribute-speaker-generation_amd.model")
T = importlib.import_module("mid-attribute-speaker-generation_amd.train")
L = importlib.import_module("mid-attribute-speaker-generation_amd.loss")
K = PKG.kernels
DEV = "cuda"

TOL = {torch.float32: dict(loss=1e-4, out=1e-4, probe=1e-3),  # tests/test_gpu_parity.py:193-194
       torch.bfloat16: dict(loss=1e-2, out=2e-2, probe=5e-2)}


def close(a, b, rtol=1e-4, what=""):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    scale = max(np.abs(b).max(), 1e-6)
    err = np.abs(a - b).max()
    print(f"{what}: max abs err {err:.3e}, scale {scale:.3e}")
    assert err <= rtol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------ 1. the fused kernel
B1, TS1, D1, TM1, NB = 3, 11, 256, 37, 256
# utterance 0 sums to 41 > 37 (cropped), 1 to exactly 37, 2 to 25 (12 padded frames); zeros inside
DUR1 = [[4, 0, 5, 3, 0, 6, 2, 7, 1, 9, 4], [3, 3, 0, 4, 5, 2, 0, 6, 7, 4, 3],
        [2, 0, 0, 5, 1, 3, 4, 0, 6, 4, 0]]
LEN1 = [37, 37, 25]


@pytest.fixture(scope="module")
def expand_case():
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B1 * TS1, D1, generator=g)
    tabs = [torch.randn(NB, D1, generator=g) for _ in range(2)]
    bins = [torch.linspace(-2.5, 3.0, NB - 1), torch.linspace(-1.5, 2.0, NB - 1)]
    vals = []
    for _ in range(2):  # zero-padded per-frame targets, as pad_1D leaves them
        v = torch.randn(B1, TM1, generator=g)
        for b, n in enumerate(LEN1):
            v[b, n:] = 0.0
        vals.append(v)
    vals[0][0, 3] = bins[0][17]  # a value on a bin edge (bucketize right=False)
    pos = fs2_cpu.sinusoid_table(64, D1)
    dur = torch.tensor(DUR1)
    assert dur.sum(1).tolist() == [41, 37, 25]
    dev = lambda t: t.to(DEV).contiguous()
    cum, mel_len = K.lr_index(dev(dur))
    assert mel_len.tolist() == [41, 37, 25]
    return dict(x=dev(x), tabs=[dev(t) for t in tabs], bins=[dev(b) for b in bins],
                vals=[dev(v) for v in vals], pos=dev(pos), cum=cum,
                zero_bucket=[int(torch.bucketize(torch.zeros(()), b)) for b in bins])


def _composition(c, pitch, energy, T_dec, copy):
    """lr_expand (no posenc) -> bucket_embed -> bucket_embed -> + posenc[:T_dec], existing launches."""
    v, v_t = K.lr_expand(c["x"], c["cum"], TM1, copy=copy)
    pre = v if copy is None else v_t
    mid = p_idx = e_idx = None
    if pitch:
        v, v_t, p_idx = K.bucket_embed(v, c["vals"][0].view(-1), c["bins"][0], c["tabs"][0], copy=copy)
        mid = v if copy is None else v_t
    if energy:
        v, _, e_idx = K.bucket_embed(v, c["vals"][1].view(-1), c["bins"][1], c["tabs"][1])
    out = v.clone().view(B1, TM1, D1)
    for b in range(B1):
        K.add(out[b, :T_dec], c["pos"][:T_dec], out=out[b, :T_dec])
    out = out.view(-1, D1)
    return pre, mid, out, (K.cast_bf16(out) if copy is not None else None), p_idx, e_idx


@pytest.mark.parametrize("T_dec", [37, 29])
@pytest.mark.parametrize("pitch,energy", [(True, False), (False, True), (True, True)])
def test_fused_expand_embed_bitwise_vs_composition(expand_case, pitch, energy, T_dec):
    c = expand_case
    feat = lambda i: (c["vals"][i], c["bins"][i], c["tabs"][i])
    for copy in (None, torch.bfloat16):
        want = _composition(c, pitch, energy, T_dec, copy)
        got = K.lr_expand_embed(c["x"], c["cum"], TM1, pitch=feat(0) if pitch else None,
                                energy=feat(1) if energy else None, posenc=c["pos"],
                                pos_len=T_dec, copy=copy, want_pre=True, want_mid=pitch)
        names = ("pre", "mid", "out", "out_t", "p_idx", "e_idx")
        for name, g_, w_ in zip(names, got, want):
            assert (g_ is None) == (w_ is None), (name, copy)
            if g_ is not None:
                assert g_.dtype == w_.dtype and torch.equal(g_, w_), (name, copy, pitch, energy)
        for i, on in enumerate((pitch, energy)):
            if on:
                ref = torch.bucketize(c["vals"][i].cpu(), c["bins"][i].cpu()).view(-1)
                assert torch.equal(got[4 + i].cpu().long(), ref)
        # a padded frame is not zero: it holds the embeddings of bucket(0) (+ the position row)
        out = got[2].view(B1, TM1, D1)
        for t in (25, 28, 30, 36):
            row = torch.zeros(D1, device=DEV)
            if pitch:
                row = row + c["tabs"][0][c["zero_bucket"][0]]
            if energy:
                row = row + c["tabs"][1][c["zero_bucket"][1]]
            if t < T_dec:
                row = row + c["pos"][t]
            assert torch.equal(out[2, t], row), (t, T_dec)
        # the product's own composition switch gives the same tensors
        alt = M._frame_expand(c["x"], c["cum"], TM1, feat(0) if pitch else None,
                              feat(1) if energy else None, c["pos"], T_dec, copy, True, pitch,
                              fused=False)
        for g_, a_ in zip(got, alt):
            assert (g_ is None) == (a_ is None) and (g_ is None or torch.equal(g_, a_))


def test_fused_expand_embed_unread_outputs_are_not_written():
    """Stage calls of the inference path: no decoder output, no indices; f64 values bucketize
    as f32 ones do."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2 * 5, 64, generator=g).to(DEV)
    cum, _ = K.lr_index(torch.tensor([[2, 0, 3, 1, 1], [1, 1, 1, 0, 2]], device=DEV))
    vals = torch.randn(2, 7, generator=g).to(DEV)
    bins = torch.linspace(-2, 2, 15).to(DEV)
    tab = torch.randn(16, 64, generator=g).to(DEV)
    pre, mid, out, out_t, pi, ei = K.lr_expand_embed(x, cum, 7, pitch=(vals, bins, tab), want_mid=True,
                                                     want_out=False, want_idx=False)
    assert pre is None and out is None and out_t is None and pi is None and ei is None
    full = K.lr_expand_embed(x, cum, 7, pitch=(vals.double(), bins, tab))
    assert torch.equal(mid, full[2]) and full[3] is None
    with pytest.raises(RuntimeError):
        K.lr_expand_embed(x, cum, 7, pitch=(vals[:, :6].contiguous(), bins, tab))


# ------------------------------------------------------------------ 2. the levelled loss
@pytest.mark.parametrize("with_denoms", [False, True])
@pytest.mark.parametrize("levels", [(False, False), (True, False), (False, True), (True, True)])
def test_level_loss_vs_autograd(levels, with_denoms):
    """fp32 sums of a few hundred terms (double in the finaliser) against torch's fp32 means:
    both are within ~1e-6 relative of the exact value, checked at the suite's 1e-4 of scale."""
    g = torch.Generator().manual_seed(5)
    Bn, Ts, Tm, n_mel = 3, 7, 23, 80
    src_lens, mel_lens = torch.tensor([7, 4, 6]), torch.tensor([23, 9, 17])
    src_pad = torch.arange(Ts)[None] >= src_lens[:, None]
    mel_pad = torch.arange(Tm)[None] >= mel_lens[:, None]
    rnd = lambda *s: torch.randn(*s, generator=g)
    widths = [Tm if f else Ts for f in levels]
    cpu = dict(mel=rnd(Bn, Tm, n_mel), post=rnd(Bn, Tm, n_mel), p=rnd(Bn, widths[0]),
               e=rnd(Bn, widths[1]), logd=rnd(Bn, Ts))
    mels, p_t, e_t = rnd(Bn, Tm + 3, n_mel), rnd(Bn, widths[0]), rnd(Bn, widths[1])
    d_t = torch.randint(0, 6, (Bn, Ts), generator=g)
    w6 = torch.rand(6, generator=g) + 0.5
    denoms = torch.tensor([2.5 * float(mel_lens.sum()) * n_mel, 3.0 * float(src_lens.sum())]) \
        if with_denoms else None

    ref_in = {k: v.clone().requires_grad_() for k, v in cpu.items()}
    sv, mv = ~src_pad, ~mel_pad
    n_fr = denoms[0] / n_mel if with_denoms else mv.sum()
    n_ph = denoms[1] if with_denoms else sv.sum()
    n_el = denoms[0] if with_denoms else mv.sum() * n_mel
    mt = mels[:, :Tm].masked_select(mv[..., None])
    l1 = lambda x: (x.masked_select(mv[..., None]) - mt).abs().sum() / n_el
    mse = lambda x, t, frame: ((x.masked_select(mv if frame else sv)
                                - t.masked_select(mv if frame else sv)) ** 2).sum() / (n_fr if frame else n_ph)
    r = [None, l1(ref_in["mel"]), l1(ref_in["post"]), mse(ref_in["p"], p_t, levels[0]),
         mse(ref_in["e"], e_t, levels[1]), mse(ref_in["logd"], torch.log(d_t.float() + 1), False)]
    r[0] = r[1] + r[2] + r[5] + r[3] + r[4]
    if not with_denoms:  # the local-count form is model/loss.py's masked_select + mean
        want = flo.fs2_loss((None,) * 6 + (mels, None, None, p_t, e_t, d_t),
                            (cpu["mel"], cpu["post"], cpu["p"], cpu["e"], cpu["logd"], None, src_pad,
                             mel_pad), levels)
        np.testing.assert_allclose([float(v) for v in want], [float(v) for v in r], rtol=1e-5)
    sum(w * v for w, v in zip(w6, r)).backward()

    dv = {k: v.to(DEV).requires_grad_() for k, v in cpu.items()}
    got = L.FS2LevelLossFn.apply(dv["mel"], dv["post"], dv["p"], dv["e"], dv["logd"], mels.to(DEV),
                                 p_t.to(DEV), e_t.to(DEV), d_t.to(DEV), src_pad.to(DEV),
                                 mel_pad.to(DEV), None if denoms is None else denoms.to(DEV), None,
                                 levels)
    close(torch.stack(list(got)), torch.stack([v.detach() for v in r]), 1e-4, f"losses {levels}")
    sum(w * v for w, v in zip(w6.to(DEV), got)).backward()
    for k in cpu:
        close(dv[k].grad, ref_in[k].grad, 1e-4, f"d {k} {levels}")
        pad = (mel_pad if dv[k].shape[1] == Tm else src_pad).to(DEV)
        assert not dv[k].grad[pad].any(), f"d {k}: gradient on a padded position"


# ------------------------------------------------------------------ 3. trajectories
def _hip_trainer(levels, B, Ts, seed=0, dtype=torch.float32, dropout=False, graph=False):
    pp, mc, tc, path = flo.level_configs("JVS-VCTK", levels)
    model = M.FastSpeech2(pp, mc, path, device=DEV, compute_dtype=dtype)
    PKG.seeded.load_seeded_(model)
    model.dropout = dropout
    model.train()
    tr = T.Trainer(model, pp, mc, tc, graph=graph)
    return model, tr, flo.level_batch("JVS-VCTK", B, Ts, seed, levels, DEV)


def _check_trajectory(g, model, tr, batch, dtype):
    """test_gpu_parity._check_trajectory's comparisons; the predictions are compared per shape
    (pred_probe: the (B, Ts) ones, frame_pred_probe: the (B, T_mel) ones)."""
    tol = TOL[dtype]
    Ts = int(g["Ts"])
    close(model.encoder.position_enc[0, ::97, ::31], g["pos_enc_probe"], 0, "position_enc")
    for s in range(3):
        losses, eloss, gnorm, out = tr.step(batch)
        close(torch.stack(list(losses)), g[f"s{s}.losses"], tol["loss"], f"step {s} losses")
        close(eloss, g[f"s{s}.eloss"], tol["loss"], f"step {s} eloss")
        close(gnorm, g[f"s{s}.gnorm"], tol["loss"], f"step {s} grad norm")
        assert abs(tr.opt._optimizer.param_groups[0]["lr"] - float(g[f"s{s}.lr"])) < 1e-15
        np.testing.assert_array_equal(out[9].cpu().numpy(), g[f"s{s}.mel_lens"])
        o, po = out[0].double(), out[1].double()
        close(torch.stack([o.sum(), o.abs().sum(), po.sum(), po.abs().sum()]), g[f"s{s}.out_sum"],
              tol["out"], f"step {s} output sums")
        close(out[1][:, ::37, ::7], g[f"s{s}.out_probe"], tol["probe"], f"step {s} postnet probe")
        preds = [out[2], out[3], out[4]]
        close(torch.stack([p for p in preds if p.shape[1] == Ts]), g[f"s{s}.pred_probe"],
              tol["probe"], f"step {s} phoneme-level preds")
        close(torch.stack([p for p in preds if p.shape[1] != Ts]), g[f"s{s}.frame_pred_probe"],
              tol["probe"], f"step {s} frame-level preds")


@pytest.mark.parametrize("name,dtype", [("g12_frame_step_b3_t16.npz", torch.float32),
                                        ("g12_mixed_step_b3_t16.npz", torch.float32),
                                        ("g12_frame_step_b3_t16.npz", torch.bfloat16)])
def test_frame_level_trajectory_vs_reference(name, dtype):
    g = load_golden(name)
    levels = (str(g["pitch_level"]), str(g["energy_level"]))
    model, tr, batch = _hip_trainer(levels, int(g["B"]), int(g["Ts"]), int(g["seed"]), dtype)
    _check_trajectory(g, model, tr, batch, dtype)


# ------------------------------------------------------------------ 4. full tensors
def _structural_zero(name):  # tests/test_gpu_parity.py: gradients that are zero in exact arithmetic
    return name.endswith("slf_attn.w_ks.bias") or ("postnet" in name or "convolutions" in name) \
        and name.endswith(".0.conv.bias")


# Seeds are screened on the CPU oracle for ReLU kinks, as test_gpu_parity.py's are: frame-level
# predictors have 4x the rows, so some pre-activation always lies near zero, and one within the
# two fp32 implementations' rounding difference flips its ReLU gradient.  Of seeds 1-8 these keep
# the oracle's smallest |ReLU input| largest (3.1e-6 and 2.8e-6; seed 3 of "frame" has 4.2e-7).
@pytest.mark.parametrize("key,B,Ts,seed", [("frame", 3, 13, 4), ("pitch", 2, 9, 8)])
def test_frame_level_step_vs_oracle_full_tensors(key, B, Ts, seed):
    """One step on the CPU oracle: every output tensor and every parameter gradient (odd sizes;
    "pitch": frame-level pitch with phoneme-level energy, whose predictor then reads x0)."""
    levels = flo.LEVELS[key]
    model, tr, batch = _hip_trainer(levels, B, Ts, seed)
    out = model(*(batch[2:12]), accents=batch[13], speaker_meta=batch[12])
    losses = tr.Loss(batch[:12], out[:-2])
    losses[0].backward()
    (-tr.eLoss(out[-1], out[-2])).backward()
    fs2_cpu.DROPOUT["enabled"] = False
    try:
        ref = flo.build("JVS-VCTK", levels)
        ref.train()
        cb = flo.level_batch("JVS-VCTK", B, Ts, seed, levels)
        ro = ref(*cb[2:12], accents=cb[13], speaker_meta=cb[12])
        rl = flo.fs2_loss(cb[:12], ro[:-2], ref.levels)
        rl[0].backward()
        (-fs2_cpu.speaker_enc_loss(ro[-1], ro[-2])).backward()
    finally:
        fs2_cpu.DROPOUT["enabled"] = True
    close(torch.stack(list(losses)), torch.stack([v.detach() for v in rl]), 1e-4, "losses")
    for i in (0, 1, 2, 3, 4):
        close(out[i], ro[i], 1e-4, f"output {i}")
    assert torch.equal(out[6].cpu(), ro[6]) and torch.equal(out[7].cpu(), ro[7])
    ours = dict(model.named_parameters())
    for name, p in ref.named_parameters():
        if p.grad is None:
            continue
        if _structural_zero(name):
            w = dict(ref.named_parameters())[name.rsplit(".", 1)[0] + ".weight"]
            assert M._g(ours[name]).abs().max().item() <= 1e-3 * w.grad.abs().max().item(), name
            continue
        close(M._g(ours[name]), p.grad, 2e-4, name)


# ------------------------------------------------------------------ 5. inference
def test_frame_level_inference_vs_reference():
    g = load_golden("g13_frame_infer.npz")
    levels = flo.LEVELS["frame"]
    pp, mc, _, path = flo.level_configs("JVS-VCTK", levels)
    m = M.FastSpeech2(pp, mc, path, device=DEV)
    PKG.seeded.load_seeded_(m)
    sd = m.state_dict()
    with torch.no_grad():
        for k in g.files:
            if k.startswith("ov."):
                sd[k[3:]].copy_(torch.from_numpy(g[k]))
    m.eval()
    b = flo.level_batch("JVS-VCTK", int(g["B"]), int(g["Ts"]), int(g["seed"]), levels, DEV)

    def check(tag, out):
        np.testing.assert_array_equal(out[9].cpu().numpy(), g[f"{tag}.mel_lens"])
        np.testing.assert_array_equal(out[5].cpu().numpy(), g[f"{tag}.d_r"])
        np.testing.assert_array_equal(out[7].cpu().numpy(), g[f"{tag}.mel_mask"])
        for i, name in enumerate(("out", "post", "p", "e", "log_d")):
            close(out[i].float(), g[f"{tag}.{name}"], 1e-4, f"{tag}.{name}")

    with torch.no_grad():
        check("A", m(b[2], b[3], b[4], b[5], p_control=float(g["p_control"]),
                     d_control=float(g["d_control"]), accents=b[13], speaker_meta=b[12]))
        out = m(*(b[2:12]), accents=b[13], speaker_meta=b[12])
        check("B", out)
        losses = L.FastSpeech2Loss(pp, mc)(b[:12], out[:-2])
    close(torch.stack(list(losses)), g["B.losses"], 1e-4, "B.losses")


def test_frame_level_eval_past_max_seq_len_and_training_refusal():
    """Eval mode does not truncate (Models.py:160-165): 1,056 frames run whole; training mode
    raises the ValueError naming the reference lines."""
    levels = flo.LEVELS["frame"]
    pp, mc, _, path = flo.level_configs("JVS-VCTK", levels)
    m = M.FastSpeech2(pp, mc, path, device=DEV)
    PKG.seeded.load_seeded_(m)
    b = flo.level_batch("JVS-VCTK", 2, 264, 0, levels, DEV)
    m.train()
    with pytest.raises(ValueError, match=r"Models\.py:166-173"):
        m(*(b[2:12]), accents=b[13], speaker_meta=b[12])
    m.eval()
    with torch.no_grad():
        out = m(*(b[2:12]), accents=b[13], speaker_meta=b[12])
    assert out[0].shape == (2, 1056, 80) and out[2].shape == out[3].shape == (2, 1056)
    assert out[7].shape == (2, 1056) and bool(torch.isfinite(out[1]).all())
    assert not out[2][out[7]].any() and not out[3][out[7]].any()  # masked predictions are 0.0


# ------------------------------------------------------------------ 6. repeatability
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_frame_level_step_bitwise_reproducible(dt):
    """Two runs of 2 steps (dropout on) from the same weights and seed: bitwise-equal weights
    and Adam moments (fixed summation order in the frame-level backward, no atomics); a graph
    replay of the same step matches them too."""
    finals = []
    for graph in (False, False, True):
        model, tr, batch = _hip_trainer(flo.LEVELS["frame"], 3, 16, seed=2, dtype=dt, dropout=True,
                                        graph=graph)
        model.seed(41)
        for _ in range(2):
            tr.step(batch)
        torch.cuda.synchronize()
        finals.append((model.arena().flat.clone(), tr.opt.m.clone(), tr.opt.v.clone()))
    for other in finals[1:]:
        for a, b in zip(finals[0], other):
            assert torch.equal(a, b)


# total loss of the third fp32 step at SYN-3x16 (seed 0, dropout off, phoneme-level config) on
# the parent commit, as float.hex() (recorded from a run of the parent's tree on an MI355X)
PARENT_PHONEME_LOSS_HEX = "0x1.c09f860000000p+3"


def test_phoneme_level_step_unchanged_from_parent():
    pp, mc, tc, path = PKG.config.load_configs("JVS-VCTK")
    model = M.FastSpeech2(pp, mc, path, device=DEV)
    PKG.seeded.load_seeded_(model)
    model.dropout = False
    model.train()
    tr = T.Trainer(model, pp, mc, tc)
    batch = PKG.data.to_device(PKG.data.syn_batch_for("JVS-VCTK", 3, 16, seed=0), DEV)
    for _ in range(3):
        losses = tr.step(batch)[0]
    got = float(losses[0]).hex()
    print("phoneme-level total loss after 3 steps:", got, float(losses[0]))
    assert got == PARENT_PHONEME_LOSS_HEX


def test_frame_level_data_parallel_step_and_grad_accumulation():
    """The data-parallel step on one GPU (stand-in collectives, as tests/test_dp.py runs it) with
    both features frame-level and grad_acc_step = 2: the frame-level terms are normalised by
    denoms[0] / n_mel, every gradient bucket goes out once per optimiser step (the notify order of
    the frame-level backward releases them), and losses / weights match the plain step at that
    test's bounds (1e-5 relative, 1e-6 of the weights' scale)."""
    levels = flo.LEVELS["frame"]
    res = {}
    for mode in ("plain", "model"):
        pp, mc, tc, path = flo.level_configs("JVS-VCTK", levels)
        tc["optimizer"]["grad_acc_step"] = 2
        model = M.FastSpeech2(pp, mc, path, device=DEV, compute_dtype=torch.bfloat16)
        PKG.seeded.load_seeded_(model)
        model.train()
        model.dropout = False
        if mode == "plain":
            t = T.Trainer(model, pp, mc, tc)
        else:
            t = T.Trainer(model, pp, mc, tc, collective_model=T.CollectiveModel(
                ranks=8, busbw_gbs=300.0, blocks=8, latency_us=5.0), bucket_bytes=16 << 20)
            t.buckets.log = []
        outs = [t.step(flo.level_batch("JVS-VCTK", 3, 16, s, levels, DEV)) for s in range(4)]
        torch.cuda.synchronize()
        assert [o[2] is None for o in outs] == [True, False, True, False]  # steps every 2nd batch
        res[mode] = ([[float(x) for x in o[0]] for o in outs], model.arena().flat.cpu(),
                     list(t.buckets.log) if t.buckets is not None else None)
        if mode == "model":
            n_frames = float(flo.level_batch("JVS-VCTK", 3, 16, 3, levels)[7].sum())
            assert float(t.Loss.denoms[0]) == n_frames * 80
    for a_, b_ in zip(res["model"][0], res["plain"][0]):
        for x, y in zip(a_, b_):
            assert abs(x - y) <= 1e-5 * max(abs(y), 1e-6), (a_, b_)
    w, wp = res["model"][1], res["plain"][1]
    assert (w - wp).abs().max().item() <= 1e-6 * wp.abs().max().item()
    nb = len(t.buckets.sizes)
    assert sorted(res["model"][2]) == sorted(list(range(nb)) * 2)
