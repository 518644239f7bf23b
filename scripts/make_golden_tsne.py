"""Writes tests/golden/g17_tsne.npz: scikit-learn's exact t-SNE on the test point sets, and the
numpy oracle's (tests/tsne_oracle.py) runs and float32 deviations that size the GPU tests'
tolerances.  Runs on the CPU and needs scikit-learn; the tests never import it.

    python scripts/make_golden_tsne.py
"""
import os
import sys

import numpy as np
from scipy.spatial.distance import squareform
from sklearn.manifold import TSNE, _t_sne

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import tsne_oracle as O  # noqa: E402

# name: (n_per, groups, D, seed, perplexity)
SETS = {"a": (35, 2, 3, 1, 5.0), "b": (32, 3, 64, 2, 10.0), "c": (80, 3, 256, 3, 50.0)}
EXPLORE, SHORT = 10, 20  # the short run of the GPU tests


def rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def main():
    out = {}
    for name, (n_per, groups, D, seed, perp) in SETS.items():
        X = O.make_points(n_per, groups, D, seed)
        n = len(X)
        P, _, _ = O.joint_probabilities(X, perp)
        lr = O.auto_lr(n)
        if name in "ab":
            sk = squareform(_t_sne._joint_probabilities(O.sq_distances(X), perp, 0))
            Y = np.random.RandomState(10 + seed).standard_normal((n, 2))
            kl, grad = _t_sne._kl_divergence(Y.ravel(), squareform(sk), 1, n, 2)
            out[f"{name}_P"], out[f"{name}_Y"] = sk, Y
            out[f"{name}_kl"], out[f"{name}_grad"] = np.float64(kl), grad.reshape(n, 2)
            print(name, "oracle P vs sklearn", rel(P, sk), "kl", kl)
            # float32 numpy against float64, the same computation: sizes the KL test
            kl32, _ = O.kl_grad(Y.astype(np.float32), P, 1.0, np.float32)
            kl64, _ = O.kl_grad(Y.astype(np.float32), P, 1.0, np.float64)
            out[f"{name}_kl_dev32"] = np.float64(abs(float(kl32) - kl64) / abs(kl64))
            print(name, "kl dev32", out[f"{name}_kl_dev32"])
        if name == "b":
            Y0, S = O.pca_init(X)
            assert (S[2] / S[1]) ** 2 <= 0.9, S[:4]
            out["b_singular"] = S[:4]
            # the state after 60 iterations of stage 1, float32 as the kernels store it
            Y, upd, gains = Y0.copy(), np.zeros_like(Y0), np.ones_like(Y0)
            for _ in range(60):
                Y, upd, gains, _, _, _ = O.step(Y, upd, gains, P, 12.0, 0.5, lr, np.float32)
            out["b_state_Y"], out["b_state_update"], out["b_state_gains"] = Y, upd, gains
            r64 = O.step(Y, upd, gains, P, 12.0, 0.5, lr, np.float64)
            r32 = O.step(Y, upd, gains, P, 12.0, 0.5, lr, np.float32)
            ug = np.abs(r64[5])
            assert (ug >= 1e-6 * ug.max()).all(), "a coordinate of the state has update*grad ~ 0"
            out["b_step_dev32"] = np.array([rel(r32[0], r64[0]), rel(r32[1], r64[1]),
                                            abs(float(r32[3]) - r64[3]) / abs(r64[3]),
                                            abs(r32[4] - r64[4]) / abs(r64[4])])
            print("step dev32 (Y', update', kl, grad norm)", out["b_step_dev32"])
            # the short run with every switch, and the one that stops stage 1 on the norm
            for tag, kw in (("short", dict(max_iter=SHORT, exploration_iter=EXPLORE)),
                            ("norm", dict(max_iter=60, min_grad_norm=1e3))):
                y64, kl64, it64 = O.run(Y0, P, lr, np.float64, **kw)
                y32, kl32, it32 = O.run(Y0, P, lr, np.float32, **kw)
                assert it64 == it32
                out[f"b_{tag}_dev32"] = np.array([rel(y32, y64), abs(kl32 - kl64) / abs(kl64)])
                out[f"b_{tag}_n_iter"] = np.int64(it64)
                print(tag, "n_iter", it64, "dev32 (Y, kl)", out[f"b_{tag}_dev32"])
        if name in "bc":
            sk_kl = [TSNE(2, perplexity=perp, init="pca", method="exact",
                          random_state=s).fit(X).kl_divergence_ for s in range(4)]
            Y0, _ = O.pca_init(X)
            ours = [O.run(Y0, P, lr, np.float32)[1], O.run(Y0, P, lr, np.float64)[1]]
            for k in (1, 2, 3):
                for sgn in (1, -1):
                    ours.append(O.run(Y0.astype(np.float64) * (1 + sgn * k * 1e-3), P, lr)[1])
            out[f"{name}_final_kl"] = np.array(sk_kl + ours, np.float64)
            print(name, "final KL sklearn", sk_kl, "oracle", ours)
    path = os.path.join(REPO, "tests", "golden", "g17_tsne.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
