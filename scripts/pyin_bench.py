"""pYIN beside YIN, timed: ``fs2_f0_pyin`` and, from the same run on the same inputs,
``fs2_f0_yin``, on one utterance of 589 frames and on the 16 utterances of 10 s that
``pitch_bench.py`` times (22 050 Hz, hop 256, 71..800 Hz: 310 lags, 210 pitch bins, reach 25).
The two stages are also timed alone (``fs2_f0_pyin_candidates``, and ``fs2_f0_pyin_viterbi`` on
the first stage's output, also with a reach of 1 bin, where the maximisation is next to nothing)
for the Viterbi pass's share.  Device time per call as in
``pitch_bench.py``: events around ``--inner`` calls, medians over ``--reps`` repeats with the
spread, after a warm-up of every shape.  Prints one JSON line."""
import argparse
import importlib
import json

import torch

from pitch_bench import NAME, SECONDS, SR, device_time, spread, voiced

A = importlib.import_module(NAME + ".audio")
K = importlib.import_module(NAME + ".kernels")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    px = A.PitchExtractor(method="pyin")
    prior, tri, centres = px.tables
    res = {"device": torch.cuda.get_device_name(0), "hop": px.hop, "n_bins": centres.numel(),
           "reach": tri.numel() - 1}
    for tag, B, S in (("b1_589_frames", 1, 588 * px.hop), ("b16_10s", 16, SECONDS * SR)):
        wav = voiced(B, S, B)
        F = 1 + S // px.hop
        args = (wav, None, px.hop, px.sr, px.f0_floor, px.f0_ceil)
        out_y = (torch.empty(B, F, device="cuda"), torch.empty(B, F, device="cuda"),
                 torch.empty(B, dtype=torch.int64, device="cuda"))
        out_p = tuple(torch.empty_like(o) for o in out_y)
        mass, cf0, v, _, nf = K.f0_pyin_candidates(*args, prior, centres.numel())
        tri1 = tri[-2:].contiguous()

        runs = {
            "fs2_f0_yin": lambda: K.f0_yin(*args, px.threshold, out=out_y),
            "fs2_f0_pyin": lambda: K.f0_pyin(*args, prior, tri, centres, out=out_p),
            "candidates": lambda: K.f0_pyin_candidates(*args, prior, centres.numel()),
            "viterbi": lambda: K.f0_pyin_viterbi(mass, v, nf, tri, cf0, centres),
            # the same pass with a reach of 1 bin: what a frame costs beside the maximisation
            "viterbi_reach_1": lambda: K.f0_pyin_viterbi(mass, v, nf, tri1, cf0, centres),
        }
        for run in runs.values():
            for _ in range(3):
                run()
        r = {"shape": [B, S], "frames": B * F}
        for name, run in runs.items():
            r[name] = spread([device_time(run, a.inner) for _ in range(a.reps)])
        r["viterbi_share"] = round(r["viterbi"]["median_ms"] / r["fs2_f0_pyin"]["median_ms"], 3)
        r["voiced_share"] = {"yin": round(float((out_y[0] > 0).float().mean()), 3),
                             "pyin": round(float((out_p[0] > 0).float().mean()), 3)}
        res[tag] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
