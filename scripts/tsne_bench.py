"""Wall time of embedding_map.TSNE.fit_transform (exact t-SNE, PCA initialisation, 1000
iterations) on clustered unit-norm points, the host time spent queueing its launches, and the
same fit with scikit-learn where it is installed.

    python scripts/tsne_bench.py [--n 240 600] [--dim 64] [--perplexity 50] [--reps 5]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import tsne_oracle as O  # noqa: E402

M = importlib.import_module("mid-attribute-speaker-generation_amd.embedding_map")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[240, 600])
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--perplexity", type=float, default=50.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for n in a.n:
        X = O.make_points(n // 4, 4, a.dim, 0)
        Xd = torch.from_numpy(X).cuda()
        t = M.TSNE(perplexity=a.perplexity)
        t.fit_transform(Xd)  # warm-up: module load, allocator
        torch.cuda.synchronize()
        wall, queue = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.fit_transform(Xd)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            queue.append(t.queue_seconds_)
        P, _, _ = O.joint_probabilities(X, a.perplexity)
        kl = float(O.kl_grad(t.embedding_.cpu().numpy(), P)[0])
        line = (f"N {len(X)} D {a.dim}: fit_transform {np.median(wall) * 1e3:.1f} ms (median of "
                f"{a.reps}), of it the host queueing the descent's launches "
                f"{np.median(queue) * 1e3:.1f} ms; n_iter {t.n_iter_}, KL {kl:.4f}")
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            print(line + "; scikit-learn is not installed")
            continue
        t0 = time.perf_counter()
        sk = TSNE(2, perplexity=a.perplexity, init="pca", method="exact", random_state=0).fit(X)
        dt = time.perf_counter() - t0
        print(line + f"; scikit-learn on {os.environ.get('OMP_NUM_THREADS', '?')} threads "
              f"{dt:.2f} s, KL {sk.kl_divergence_:.4f}")


if __name__ == "__main__":
    main()
