"""Closed form, numpy fp64, of the GE2E contrast loss and its gradients (the reference's
``utils.get_similarity`` + ``get_contrast_loss`` with ``S = w sim + b``,
speech_embedder_net.py:173-179).  A helper for the contrast-loss tests, not a test.

  S_jik  as in ``embedder_oracle`` (include-self centroids, the k = j entry against the
         exclude-self centroid, each norm clamped at 1e-8)
  sig    = 1 / (1 + exp(-S))
  loss   = sum_ji (1 - sig(S_jij)) + sum_ji max_k sig~_jik,
           sig~_jik = sig(S_jik) for k != j, sig~_jij = 0

The reference zeroes the own-speaker entry in place: it takes part in the maximum with value 0
and carries no gradient.  On equal values the lowest k wins (``torch.max(dim=2)``'s index).
"""
import numpy as np

from embedder_oracle import _cos_parts

# (N, M, D) -> seed of ``make_embeddings``.  Each seed was found by a search on the CPU for a
# batch whose every row's two largest negative scores differ by at least GAP, so that the
# hardest negative is the same in fp32 and fp64 (fp32 error in S is about 1e-6 at w = 10); the
# GPU test asserts that condition before it compares anything.
GAP = 1e-4
SEEDS = {(1, 2, 8): 180, (2, 2, 8): 181, (3, 3, 100): 182, (4, 3, 64): 183, (5, 4, 256): 184,
         (17, 3, 64): 185}
CPU_SHAPES = [(1, 2, 8), (2, 2, 8), (4, 3, 64), (17, 3, 64)]  # tied to the reference (g18)


def similarity(e, w=10.0, b=-5.0):
    """e (N, M, D) -> S (N, M, N) float64 and the cosine parts behind every entry."""
    e = np.asarray(e, dtype=np.float64)
    N, M, D = e.shape
    tot = e.sum(axis=1)
    cen = tot / M
    parts = [[[_cos_parts(e[j, i], (tot[j] - e[j, i]) / (M - 1) if k == j else cen[k])
               for k in range(N)] for i in range(M)] for j in range(N)]
    S = np.array([[[w * parts[j][i][k][0] + b for k in range(N)] for i in range(M)]
                  for j in range(N)], dtype=np.float64).reshape(N, M, N)
    return S, parts


def contrast_from_similarity(S):
    """S (N, M, N) -> loss, dloss/dS (N, M, N), winner (N, M) (the k of the maximum; j itself
    where the zeroed own entry wins)."""
    S = np.asarray(S, dtype=np.float64)
    N, M, _ = S.shape
    sig = 1.0 / (1.0 + np.exp(-S))
    dS = np.zeros_like(S)
    winner = np.zeros((N, M), dtype=np.int64)
    loss = 0.0
    for j in range(N):
        for i in range(M):
            so = sig[j, i, j]
            loss += 1.0 - so
            dS[j, i, j] = -so * (1.0 - so)
            row = sig[j, i].copy()
            row[j] = 0.0
            k = int(np.argmax(row))  # the first maximum
            winner[j, i] = k
            loss += row[k]
            if k != j:
                dS[j, i, k] = row[k] * (1.0 - row[k])
    return loss, dS, winner


def negative_gaps(S):
    """Per row, the difference of the two largest negative scores S_jik, k != j (inf where a
    row has fewer than two negatives): the margin by which the hardest negative is decided."""
    S = np.asarray(S, dtype=np.float64)
    N, M, _ = S.shape
    gaps = np.full((N, M), np.inf)
    if N < 3:
        return gaps
    for j in range(N):
        neg = np.sort(np.delete(S[j], j, axis=1), axis=1)
        gaps[j] = neg[:, -1] - neg[:, -2]
    return gaps


def ge2e_contrast(e, w=10.0, b=-5.0):
    """e (N, M, D) -> loss, demb (N, M, D), dw, db; all float64."""
    e = np.asarray(e, dtype=np.float64)
    N, M, D = e.shape
    S, parts = similarity(e, w, b)
    loss, dS, _ = contrast_from_similarity(S)
    demb = np.zeros_like(e)
    dcen = np.zeros((N, D))
    dw, db = 0.0, float(dS.sum())
    for j in range(N):
        for i in range(M):
            for k in range(N):
                if dS[j, i, k] == 0.0:
                    continue
                sim, da, dbv = parts[j][i][k]
                dw += dS[j, i, k] * sim
                g = w * dS[j, i, k]
                demb[j, i] += g * da
                if k == j:  # x_ji depends on the speaker's other utterances
                    for i2 in range(M):
                        if i2 != i:
                            demb[j, i2] += g * dbv / (M - 1)
                else:
                    dcen[k] += g * dbv
    demb += dcen[:, None, :] / M
    return loss, demb, dw, db


def torch_embedder(module, x):
    """Plain-torch restatement of ``SpeechEmbedder.forward`` (LSTM architecture, dropout off)
    over ``module``'s own ``nn.LSTM`` / ``nn.Linear`` parameters, in their dtype:
    x (rows, T, 80) -> unit-length embeddings (rows, 64), logits (rows)."""
    import torch
    out, _ = module.LSTM_stack(x)
    p = module.projection.linear_layer(out[:, -1])
    e = p / p.norm(dim=1, keepdim=True)
    lin = [getattr(module.da_classifier.classifier.layer, f"linear_{i}").linear_layer
           for i in range(3)]
    a = torch.relu(lin[1](torch.relu(lin[0](e))))
    return e, lin[2](a).squeeze(1)


def make_embeddings(N, M, D, seed):
    """Unit-norm float32 rows with a per-speaker offset: speakers are separated, utterances of
    one speaker close, like a partly trained encoder's output."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((N, M, D)) + 1.5 * rng.standard_normal((N, 1, D))
    return (e / np.linalg.norm(e, axis=2, keepdims=True)).astype(np.float32)
