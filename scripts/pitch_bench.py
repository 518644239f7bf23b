"""The F0 contour, timed: ``fs2_f0_yin`` on 16 utterances of 10 s and on one (22 050 Hz, hop 256,
the default 71..800 Hz range: 310 lags, 512-sample window), synthetic voiced signals.  Times are
device time per call (events around ``--inner`` calls, a synchronise before the clock is read),
medians over ``--reps`` repeats with the spread (min, max) beside them, after a warm-up of every
shape.  Reported with what the algorithm needs, counted from the shapes: 3 floating-point
operations (subtract, multiply, add) per sample pair, ``3 * 512 * tau_max`` per frame, and the
bytes it must move (4 S in, 8 F out per utterance).  The whole batch is also run through
``preprocess.FeatureExtractor`` (mel + energy + F0 + fill + phoneme means) for the end-to-end
frames per second.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = "mid-attribute-speaker-generation_amd"
A = importlib.import_module(NAME + ".audio")
K = importlib.import_module(NAME + ".kernels")
PRE = importlib.import_module(NAME + ".preprocess")
SECONDS, SR, W = 10, 22050, 512


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "reps": len(ms)}


def device_time(run, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def voiced(B, S, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(B):
        f = np.linspace(90.0 + 100.0 * rng.random(), 120.0 + 200.0 * rng.random(), S)
        phase = 2.0 * np.pi * np.cumsum(f) / SR
        x = sum(a * np.sin(h * phase + 6.28 * rng.random()) for h, a in ((1, 1.0), (2, 0.6), (3, 0.4)))
        rows.append(0.1 * x + 0.003 * rng.standard_normal(S))
    return torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    px = A.PitchExtractor()
    fx = PRE.FeatureExtractor()
    tau_max = int(px.sr // px.f0_floor)
    res = {"device": torch.cuda.get_device_name(0), "hop": px.hop, "tau_max": tau_max}
    for B in (16, 1):
        S = SECONDS * SR
        wav = voiced(B, S, B)
        F = 1 + S // px.hop
        out = (torch.empty(B, F, device="cuda"), torch.empty(B, F, device="cuda"),
               torch.empty(B, dtype=torch.int64, device="cuda"))
        durs = [[F // 40] * 40 for _ in range(B)]

        def yin():
            return K.f0_yin(wav, None, px.hop, px.sr, px.f0_floor, px.f0_ceil, px.threshold, out=out)

        def features():
            return fx(wav, None, durs)

        for _ in range(5):
            yin(), features()
        t_yin = [device_time(yin, a.inner) for _ in range(a.reps)]
        t_all = [device_time(features, max(a.inner // 5, 1)) for _ in range(a.reps)]
        flop = 3.0 * W * tau_max * F * B
        r = {"shape": [B, S], "frames": B * F, "fs2_f0_yin": spread(t_yin),
             "feature_extractor": spread(t_all), "flop": flop, "bytes_moved": B * (4 * S + 8 * F),
             "voiced_share": round(float((out[0] > 0).float().mean()), 3)}
        ms = r["fs2_f0_yin"]["median_ms"]
        r["fs2_f0_yin"]["frames_per_s"] = round(B * F / ms * 1e3)
        r["fs2_f0_yin"]["tflop_per_s"] = round(flop / ms / 1e9, 2)
        r["feature_extractor"]["frames_per_s"] = round(B * F / r["feature_extractor"]["median_ms"] * 1e3)
        res[f"b{B}_10s"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
