"""The resampler, timed: ``fs2_resample`` on 16 utterances of 10 s and on one, 48 000 and
24 000 -> 22 050 Hz, synthetic voiced signals.  Times are device time per call (events around
``--inner`` calls, a synchronise before the clock is read), medians over ``--reps`` repeats with
the spread (min, max) beside them, after a warm-up of every shape.  Reported with what the
algorithm needs, counted from the shapes: one multiply-add per live tap, ``(2 half + 1) / L`` per
output, and the bytes it must move (4 S in and 4 n_out out per utterance, the table once).
``scipy.signal.resample_poly`` on the host with the same table is the reference line (host clock,
median of 3).  A whole ``preprocess.Preprocessor`` group (16 files of 10 s at 48 000 Hz, 16-bit:
decode, copy, resample, mel, F0, phoneme means, statistics, files) is timed by the host clock
around ``build_from_path`` after one warm-up run.  Prints one JSON line."""
import argparse
import contextlib
import importlib
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = "mid-attribute-speaker-generation_amd"
A = importlib.import_module(NAME + ".audio")
K = importlib.import_module(NAME + ".kernels")
PRE = importlib.import_module(NAME + ".preprocess")
CFG = importlib.import_module(NAME + ".config")
SECONDS, SR_OUT = 10, 22050


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


def voiced(B, S, sr, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(B):
        f = np.linspace(90.0 + 100.0 * rng.random(), 120.0 + 200.0 * rng.random(), S)
        phase = 2.0 * np.pi * np.cumsum(f) / sr
        x = sum(a * np.sin(h * phase + 6.28 * rng.random()) for h, a in ((1, 1.0), (2, 0.6), (3, 0.4)))
        rows.append(0.1 * x + 0.003 * rng.standard_normal(S))
    return np.stack(rows).astype(np.float32)


def kernel_rows(a):
    from scipy.signal import resample_poly
    res = {}
    for sr_in in (48000, 24000):
        table, L, M, half = A.resample_filter(sr_in, SR_OUT)
        tab = torch.from_numpy(table).cuda()
        for B in (16, 1):
            S = SECONDS * sr_in
            host = voiced(B, S, sr_in, B)
            wav = torch.from_numpy(host).cuda()
            n_out = -(-S * L // M)
            out = (torch.empty(B, n_out, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda"))

            def run():
                return K.resample(wav, None, tab, L, M, half, out=out)

            for _ in range(5):
                run()
            t = [device_time(run, a.inner) for _ in range(a.reps)]
            macs = B * n_out * (2 * half + 1) / L
            moved = B * 4 * (S + n_out) + 4 * len(table)
            r = {"shape": [B, S], "outputs": B * n_out, "L": L, "M": M, "taps": len(table),
                 "fs2_resample": spread(t), "macs": macs, "bytes_moved": moved}
            ms = r["fs2_resample"]["median_ms"]
            r["fs2_resample"]["gmac_per_s"] = round(macs / ms / 1e6, 1)
            r["fs2_resample"]["gb_per_s"] = round(moved / ms / 1e6, 1)
            r["fs2_resample"]["x_realtime"] = round(B * SECONDS / ms * 1e3)
            h = table.astype(np.float64) / L
            cpu = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = resample_poly(host.astype(np.float64), L, M, axis=1, window=h, padtype="constant")
                cpu.append((time.perf_counter() - t0) * 1e3)
            r["scipy_resample_poly_host"] = spread(cpu)
            r["max_abs_dev_from_scipy"] = float(np.abs(out[0].cpu().numpy() - ref).max())
            res[f"{sr_in}_b{B}_10s"] = r
    return res


def long_textgrid(rows, xmax):
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", f"xmax = {xmax}",
           "tiers? <exists>", "size = 1", "item []:", "    item [1]:", '        class = "IntervalTier"',
           '        name = "phones"', "        xmin = 0", f"        xmax = {xmax}",
           f"        intervals: size = {len(rows)}"]
    for i, (s, e, t) in enumerate(rows, 1):
        out += [f"        intervals [{i}]:", f"            xmin = {s!r}", f"            xmax = {e!r}",
                f'            text = "{t}"']
    return "\n".join(out) + "\n"


def preprocessor_group(B=16, sr=48000):
    root = tempfile.mkdtemp(prefix="resample_bench_")
    try:
        raw, pre = os.path.join(root, "raw"), os.path.join(root, "pre")
        os.makedirs(os.path.join(raw, "spk")), os.makedirs(os.path.join(pre, "TextGrid", "spk"))
        x = voiced(B, SECONDS * sr, sr, 7)
        step = (SECONDS - 0.4) / 40
        tier = [(0.0, 0.2, "sil")] + [(round(0.2 + i * step, 4), round(0.2 + (i + 1) * step, 4), "a")
                                      for i in range(40)] + [(SECONDS - 0.2, float(SECONDS), "sil")]
        for b in range(B):
            with wave.open(os.path.join(raw, "spk", f"u{b:02d}.wav"), "wb") as w:
                w.setnchannels(1), w.setsampwidth(2), w.setframerate(sr)
                w.writeframes(np.round(x[b] * 32767.0).astype("<i2").tobytes())
            with open(os.path.join(raw, "spk", f"u{b:02d}.lab"), "w") as f:
                f.write("a\n")
            with open(os.path.join(pre, "TextGrid", "spk", f"u{b:02d}.TextGrid"), "w") as f:
                f.write(long_textgrid(tier, float(SECONDS)))
        pp = CFG.load_configs()[0]
        pp.update(val_size=0.1, test_size=0.1)
        cfg = {"dataset": "bench", "path": {"raw_path": raw, "preprocessed_path": pre}, "preprocessing": pp}
        ms = []
        for _ in range(3):  # the first run is the warm-up
            p = PRE.Preprocessor(cfg, batch=B, seed=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):  # its progress lines
                out = p.build_from_path()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"files": B, "seconds_each": SECONDS, "sr_in": sr, "written": sum(len(s) for s in out),
                "warmup_ms": round(ms[0], 1), "host_clock_ms": [round(v, 1) for v in ms[1:]],
                "x_realtime": round(B * SECONDS / min(ms[1:]) * 1e3)}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "sr_out": SR_OUT}
    res.update(kernel_rows(a))
    res["preprocessor_group"] = preprocessor_group()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
