"""The FastSpeech2 data path, timed at B = 48 on a synthetic on-disk corpus with T_mel near 800:

* ``host_loader``: the reference's loader (``DataLoader(batch_size=48 * 4, shuffle=True,
  collate_fn, num_workers=--workers)``) producing collated numpy batches, per batch of 48.  Runs
  first, before the process touches the GPU (worker processes are forked);
* ``host_path``: ``dataset[i]`` x 48, ``collate_fn``, ``BatchStager.stage`` in this process;
* ``gather_path``: ``CorpusStore.gather`` of the same index groups (host index arithmetic, B int32
  over the bus, one kernel);
* ``gather_kernel``: ``fs2_batch_gather`` alone (device time) against the bytes it moves, and
  ``d2d_copy``: a plain device-to-device copy of the batch's mel tensor in the same run.

The files were written moments before, so the host paths read them from the page cache (no disk
time).  Prints one JSON line; times are medians over ``--reps`` repeats with (min, max)."""
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = "mid-attribute-speaker-generation_amd"
B, GROUP, NMELS = 48, 4, 80
META = {"gender": {"M": 0, "F": 1}, "language": {"ja": 0, "en": 1}}


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "reps": len(ms)}


def write_corpus(root, n, seed=0):
    """``n`` utterances of 88-112 phonemes and about 700-900 frames in the preprocessed layout
    (mel f32, pitch f64, energy f32, duration int64, accent strings) -> (config_dir, corpus)."""
    rng = np.random.default_rng(seed)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), NAME,
                           "configs", "symbols.json"), encoding="utf-8") as f:
        syms = [s for s in json.load(f)[1:] if s.isalpha() and len(s) <= 2]
    pre, cfg = os.path.join(root, "BENCH"), os.path.join(root, "config")
    for d in ("mel", "pitch", "energy", "duration", "accent"):
        os.makedirs(os.path.join(pre, d))
    os.makedirs(cfg)
    speakers = {f"spk{k:02d}": [k, "MF"[k % 2], ("ja", "en")[k % 2]] for k in range(8)}
    for d in (pre, cfg):
        with open(os.path.join(d, "speakers.json"), "w") as f:
            json.dump(speakers, f)
    with open(os.path.join(cfg, "stats.json"), "w") as f:
        json.dump({"pitch": [-1.9, 9.1, 210.0, 45.0], "energy": [-1.3, 19.5, 30.0, 12.0]}, f)
    lines = []
    for u in range(n):
        spk, base = f"spk{u % 8:02d}", f"bench_{u:05d}"
        L = int(rng.integers(88, 113))
        dur = rng.integers(4, 13, size=L).astype(np.int64)
        T = int(dur.sum())
        np.save(os.path.join(pre, "mel", f"{spk}-mel-{base}.npy"),
                rng.standard_normal((T, NMELS)).astype(np.float32))
        np.save(os.path.join(pre, "pitch", f"{spk}-pitch-{base}.npy"), rng.uniform(80, 400, size=L))
        np.save(os.path.join(pre, "energy", f"{spk}-energy-{base}.npy"),
                rng.uniform(0, 80, size=L).astype(np.float32))
        np.save(os.path.join(pre, "duration", f"{spk}-duration-{base}.npy"), dur)
        with open(os.path.join(pre, "accent", base + ".accent"), "w") as f:
            f.write("".join("0[]#"[int(i)] for i in rng.integers(0, 4, size=L)))
        ph = " ".join(syms[int(i)] for i in rng.integers(0, len(syms), size=L))
        lines.append(f"{base}|{spk}|{{{ph}}}|raw text {u}")
    with open(os.path.join(pre, "train.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    corpus = {"dataset": "BENCH", "path": {"preprocessed_path": pre},
              "text": {"text_cleaners": ["english_cleaners"], "language": "ja"},
              "accent": {"use_accent": True}}
    return cfg, corpus


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--utterances", type=int, default=480)
    ap.add_argument("--workers", type=int, default=15, help="loader processes beside this one")
    a = ap.parse_args()
    D = importlib.import_module(NAME + ".dataset")
    with tempfile.TemporaryDirectory() as tmp:
        cfg, corpus = write_corpus(tmp, a.utterances)
        pp = {"speaker_generation": {"metadata": META}}
        tc = {"optimizer": {"batch_size": B}}

        def concat(sort):
            return D.ConcatDataset(cfg, [D.Dataset("train.txt", D.corpus_config(pp, corpus), tc,
                                                   sort=sort, drop_last=True)])
        res = {"batch": B, "utterances": a.utterances, "workers": a.workers}

        # ---- the reference's loader with worker processes; nothing here touches the GPU
        data = concat(True)
        loader = torch.utils.data.DataLoader(data, batch_size=B * GROUP, shuffle=True,
                                             collate_fn=data.collate_fn, num_workers=a.workers)
        per_batch = []
        for rep in range(a.reps + 1):  # the first epoch also starts the workers: dropped
            t, n = time.perf_counter(), 0
            for batchs in loader:
                n += len(batchs)
            per_batch.append((time.perf_counter() - t) * 1e3 / n)
        res["host_loader"] = spread(per_batch[1:])
        del loader

        # ---- from here on the GPU
        C = importlib.import_module(NAME + ".corpus_store")
        K = importlib.import_module(NAME + ".kernels")
        host = concat(False)
        t = time.perf_counter()
        store = C.CorpusStore(host)
        torch.cuda.synchronize()
        res["store_load_s"] = round(time.perf_counter() - t, 2)
        res["store_mb"] = round(store.nbytes / 2 ** 20, 1)
        g = torch.Generator()
        g.manual_seed(0)
        groups = list(C.CorpusBatcher(store, B, GROUP, generator=g).groups())
        res["groups"] = len(groups)
        res["mean_max_mel_len"] = round(float(np.mean([store.maxima(x)[1] for x in groups])), 1)

        stager = D.BatchStager("cuda")

        def host_epoch():
            for grp in groups:
                stager.stage(host.collate_fn([host[i] for i in grp])[0])

        def gather_epoch():
            for grp in groups:
                store.gather(grp)

        def wall(run):
            out = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                run()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t) * 1e3 / len(groups))
            return out
        host_epoch()
        res["host_path"] = spread(wall(host_epoch))
        gather_epoch()
        res["gather_path"] = spread(wall(gather_epoch))

    # ---- the kernel alone on the group with the longest mel, and a copy of the same mel bytes
    grp = max(groups, key=lambda x: store.maxima(x)[1])
    first = store.gather(grp)
    outs = (first[2], first[3], first[4], first[6], first[7], first[9], first[10], first[11],
            first[12], first[13])
    ts, tm = first[5], first[8]
    run = lambda: K.batch_gather(store, first.desc, first.indices, ts, tm, out=outs)  # noqa: E731
    idx = np.asarray(grp)
    small = 3 * 8 + 4 + store.energy.element_size()  # text, dur, accent, pitch, energy
    read = int(store.mel_len[idx].sum()) * NMELS * 4 + int(store.src_len[idx].sum()) * small + \
        B * (store.meta_dim * 4 + 8 + 8 + 4)
    written = sum(t.numel() * t.element_size() for t in outs)
    src = torch.randn_like(first[6])
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)  # noqa: E731

    def device_time(fn, inner=100, replays=20):
        """Device time per call: ``inner`` calls captured into one HIP graph (a linear chain, so
        the host's enqueue cost stays out of the figure), ``replays`` replays between events."""
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(inner):
                fn()
        graph.replay()
        out = []
        for _ in range(a.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(replays):
                graph.replay()
            e.record()
            torch.cuda.synchronize()
            out.append(s.elapsed_time(e) / (inner * replays))
        return out
    for name, fn, moved in (("gather_kernel", run, read + written),
                            ("d2d_copy", copy, 2 * src.numel() * 4)):
        fn()
        res[name] = spread(device_time(fn))
        res[name]["bytes_moved"] = moved
        res[name]["gb_per_s"] = round(moved / res[name]["median_ms"] / 1e6, 1)
    res["gather_kernel"]["shape"] = [B, ts, tm]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
