"""Timings for the frame-level variance adaptor (profiles/frame_level_*.txt), device events only.

  --ab     fs2_lr_expand_embed_fwd against the four-launch composition it replaces (lr_expand ->
           bucket_embed -> bucket_embed -> + posenc -> bf16 copy) at B x Ts x T_mel x d, bf16
           copies on, alternating the two in one process; prints each one's median, min-max
           spread over the repeats and the bytes its launches stream.
  --step   the bf16 training step (Trainer.step, dropout on) at SYN-B with both features
           phoneme-level and both frame-level, alternating, median and spread.
  --root   import the package from another tree (a checkout of another commit) for --step; a tree
           without the level keywords times the phoneme-level step only.
"""
import argparse
import copy
import importlib
import os
import statistics
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--ab", action="store_true")
ap.add_argument("--step", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--batch", type=int, default=48)
ap.add_argument("--src", type=int, default=128)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
PKG = importlib.import_module("mid-attribute-speaker-generation_amd")
M = importlib.import_module("mid-attribute-speaker-generation_amd.model")
T = importlib.import_module("mid-attribute-speaker-generation_amd.train")
K = PKG.kernels
if not torch.cuda.is_available():
    raise SystemExit("frame_level_timing.py needs the GPU (no CPU timing is meaningful)")
DEV = "cuda"
print(f"package: {os.path.dirname(PKG.__file__)}  device: {torch.cuda.get_device_name(0)}")


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us per call


def report(name, xs, extra=""):
    print(f"{name:34s} median {statistics.median(xs):9.1f} us   min {min(xs):9.1f}   max {max(xs):9.1f}"
          f"   ({len(xs)} repeats){extra}", flush=True)
    return statistics.median(xs), max(xs) - min(xs)


def kernel_ab():
    B, Ts, d, fpp = args.batch, args.src, 256, 4
    Tm = Ts * fpp
    b = PKG.data.to_device(PKG.data.syn_batch(B, Ts, seed=0, pitch_level="frame_level",
                                              energy_level="frame_level"), DEV)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B * Ts, d, generator=g).to(DEV)
    tabs = [torch.randn(256, d, generator=g).to(DEV) for _ in range(2)]
    bins = [torch.linspace(-3, 3, 255).to(DEV) for _ in range(2)]
    pos = M.sinusoid_table(1001, d).to(DEV)
    cum, _ = K.lr_index(b[11].contiguous())
    pitch, energy = (b[9].contiguous(), bins[0], tabs[0]), (b[10].contiguous(), bins[1], tabs[1])
    tiled = pos[:Tm].repeat(B, 1).contiguous()  # the composition's "+ posenc" as one launch
    run = {name: (lambda f=f: M._frame_expand(x, cum, Tm, pitch, energy, pos, Tm, torch.bfloat16,
                                              True, True, fused=f, pos_tiled=tiled))
           for name, f in (("fused", True), ("composition", False))}
    for a_, c_ in zip(run["fused"](), run["composition"]()):
        assert torch.equal(a_, c_), "fused and composed outputs differ"
    n = B * Tm * d
    # streamed bytes per output element (the phoneme rows, tables and position rows are small and
    # re-read from cache): fused writes pre, mid, out_t (bf16) and out (fp32) after one gather;
    # the composition writes / re-reads an fp32 tensor per launch plus its bf16 copies
    per = {"fused": 4 + 2 + 2 + 4 + 2,
           "composition": (4 + 4 + 2) + (4 + 4 + 2) + (4 + 4) + (4 + 4 + 4) + (4 + 2)}
    for fn in run.values():
        timed(fn, 10)
    res = {k: [] for k in run}
    for _ in range(args.repeats):
        for k, fn in run.items():
            res[k].append(timed(fn, args.iters))
    print(f"kernel A/B at B={B} Ts={Ts} T_mel={Tm} d={d}, bf16 copies on, outputs bitwise equal")
    out = {}
    for k in run:
        mb = per[k] * n / 1e6
        out[k] = report(k, res[k], f"   {per[k]} B/element = {mb:.0f} MB"
                        f" -> {mb / statistics.median(res[k]) * 1e3 / 1e3:.2f} TB/s")
    gain = out["composition"][0] - out["fused"][0]
    spread = max(out["fused"][1], out["composition"][1])
    print(f"composition - fused = {gain:.1f} us, larger spread {spread:.1f} us: fused "
          f"{'beats the composition by more than the spread' if gain > spread else 'does NOT beat the composition by more than the spread'}")


def step_timing():
    pp0, mc, tc, path = PKG.config.load_configs("JVS-VCTK")
    levelled = "pitch_level" in PKG.data.syn_batch.__code__.co_varnames
    cases = [("phoneme_level", "phoneme_level")] + ([("frame_level", "frame_level")] if levelled else [])
    trainers = {}
    for lv in cases:
        pp = copy.deepcopy(pp0)
        pp["pitch"]["feature"], pp["energy"]["feature"] = lv
        model = M.FastSpeech2(pp, mc, path, device=DEV, compute_dtype=torch.bfloat16)
        PKG.seeded.load_seeded_(model)
        model.train()
        model.seed(1)
        kw = dict(pitch_level=lv[0], energy_level=lv[1]) if levelled else {}
        batch = PKG.data.to_device(PKG.data.syn_batch_for("JVS-VCTK", args.batch, args.src, seed=0, **kw), DEV)
        tr = T.Trainer(model, pp, mc, tc)
        trainers[lv[0]] = (lambda tr=tr, batch=batch: tr.step(batch))
    for fn in trainers.values():
        timed(fn, 5)
    res = {k: [] for k in trainers}
    iters = max(args.iters // 5, 5)
    for _ in range(args.repeats):
        for k, fn in trainers.items():
            res[k].append(timed(fn, iters))
    print(f"bf16 training step at SYN-{args.batch} ({args.batch} x {args.src} phonemes x "
          f"{4 * args.src} frames), eager Trainer.step, dropout on, {iters} steps per repeat")
    for k in trainers:
        report(f"step, pitch+energy {k}", res[k])


if args.ab:
    kernel_ab()
if args.step:
    step_timing()
