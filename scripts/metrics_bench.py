"""The objective synthesis metrics, timed:

* ``dtw``: ``fs2_dtw`` for B = 16 pairs of 800 x 800 frames, K = 13, and ``dtw_one_pair``.  Device
  events around one call, the median of ``--reps`` repeats after a warm-up, with (min, max);
* ``mfcc`` and ``path_metrics`` at the same size, likewise;
* ``oracle_cpu``: the numpy fp64 oracle (tests/dtw_oracle.py) on the same 16 pairs, wall clock,
  and whether the device's costs and paths equal it;
* ``evaluate_synthesis``: one pass over the 13-utterance synthetic validation corpus of the tests
  with the seeded model, without and with the F0 comparison (Griffin-Lim, 60 iterations), wall
  clock around the call, which ends in its host read.

Prints one JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAME = "mid-attribute-speaker-generation_amd"


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "reps": len(ms)}


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    K = importlib.import_module(NAME + ".kernels")
    MT = importlib.import_module(NAME + ".metrics")
    import dtw_oracle as O

    B, T, k = args.pairs, args.frames, 13
    rng = np.random.default_rng(0)
    a = rng.standard_normal((B, T, k)).astype(np.float32)
    b = rng.standard_normal((B, T, k)).astype(np.float32)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    n = torch.full((B,), T, dtype=torch.int64, device="cuda")
    out = {"pairs": B, "frames": T, "K": k}

    out["dtw"] = spread(timed(lambda: K.dtw(da, db, n, n), args.reps))
    one = torch.ones(1, dtype=torch.int64, device="cuda") * T
    out["dtw_one_pair"] = spread(timed(lambda: K.dtw(da[:1], db[:1], one, one), args.reps))

    mel = torch.from_numpy(rng.uniform(-11.6, 2.0, (B, 80, T)).astype(np.float32)).cuda()
    out["mfcc"] = spread(timed(lambda: MT.mfcc(mel, n), args.reps))
    cost, path, path_len = K.dtw(da, db, n, n)
    f0 = torch.full((B, T), 200.0, device="cuda")
    out["path_metrics"] = spread(timed(
        lambda: K.path_metrics(cost, path, path_len, n, n, T, T, f0, f0), args.reps))

    t0 = time.perf_counter()
    want = [O.dtw(a[p], b[p]) for p in range(B)]
    out["oracle_cpu"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1)}
    cost, path, path_len = cost.cpu().numpy(), path.cpu().numpy(), path_len.cpu().numpy()
    out["oracle_cpu"]["max_rel_cost_err"] = float(max(
        abs(cost[p] - want[p][0]) / want[p][0] for p in range(B)))
    out["oracle_cpu"]["paths_equal"] = bool(all(
        np.array_equal(path[p, :path_len[p]], want[p][1]) for p in range(B)))

    # one evaluate_synthesis pass over the tests' synthetic validation corpus
    from corpus_store_helpers import corpora_at, datasets, write_val
    pkg = importlib.import_module(NAME)
    A = importlib.import_module(NAME + ".audio")
    C = importlib.import_module(NAME + ".corpus_store")
    M = importlib.import_module(NAME + ".model")
    Tr = importlib.import_module(NAME + ".train")
    pp, mc, tc, cfg_path = pkg.config.load_configs("JVS-VCTK")
    with tempfile.TemporaryDirectory() as root:
        corpus = corpora_at(root)
        write_val(corpus)
        val = C.CorpusStore(datasets(corpus, sort=False, drop_last=False, filename="val.txt"),
                            device="cuda")
    model = M.FastSpeech2(pp, mc, cfg_path, device="cuda", compute_dtype=torch.float32)
    pkg.seeded.load_seeded_(model)
    model.train()
    fe = A.MelFrontEnd(pp, device="cuda")
    kw = dict(vocoder=A.GriffinLim(front_end=fe), pitch=A.PitchExtractor(pp, device="cuda"),
              front_end=fe)
    for name, extra in (("evaluate_synthesis", {}), ("evaluate_synthesis_f0", kw)):
        wall = []
        for rep in range(2 + min(args.reps, 7)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            figures = Tr.evaluate_synthesis(model, 1, val, batch_size=4, **extra)[0]
            torch.cuda.synchronize()
            if rep >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(spread(wall), utterances=figures["utterances"],
                         path_len=figures["path_len"])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
