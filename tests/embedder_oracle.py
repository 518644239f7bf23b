"""Closed form, numpy fp64, of the GE2E softmax loss and its gradients (the reference's
``utils.get_similarity`` + ``get_softmax_loss`` with ``S = w sim + b``,
speech_embedder_net.py:173-181).  A helper for the embedder-training tests, not a test.

  c_k    = mean_i e_ki                      include-self centroid
  x_ji   = (sum_i' e_ji' - e_ji) / (M - 1)  exclude-self centroid
  sim_jik = cos(e_ji, c_k) for k != j, cos(e_ji, x_ji) for k = j   (each norm clamped at 1e-8)
  loss   = sum_ji log(sum_k exp S_jik + 1e-6) - S_jij
"""
import numpy as np

EPS = 1e-8


def _cos_parts(a, b):
    na, nb = max(np.linalg.norm(a), EPS), max(np.linalg.norm(b), EPS)
    dot = float(a @ b)
    sim = dot / (na * nb)
    # d sim / d a, d sim / d b (the norms here are far from the clamp)
    da = b / (na * nb) - dot * a / (na ** 3 * nb)
    db = a / (na * nb) - dot * b / (na * nb ** 3)
    return sim, da, db


def ge2e_softmax(e, w=10.0, b=-5.0):
    """e (N, M, D) -> loss, demb (N, M, D), dw, db; all float64."""
    e = np.asarray(e, dtype=np.float64)
    N, M, D = e.shape
    tot = e.sum(axis=1)
    cen = tot / M
    loss, dw, db = 0.0, 0.0, 0.0
    demb = np.zeros_like(e)
    dcen = np.zeros_like(cen)
    for j in range(N):
        for i in range(M):
            a = e[j, i]
            xc = (tot[j] - a) / (M - 1)
            parts = [_cos_parts(a, xc if k == j else cen[k]) for k in range(N)]
            S = np.array([w * p[0] + b for p in parts])
            den = np.exp(S).sum() + 1e-6
            loss += np.log(den) - S[j]
            dS = np.exp(S) / den
            dS[j] -= 1.0
            db += -1e-6 / den  # sum_k dS in closed form
            dw += float(sum(dS[k] * parts[k][0] for k in range(N)))
            for k in range(N):
                g = w * dS[k]
                demb[j, i] += g * parts[k][1]
                if k == j:  # x_ji depends on the speaker's other utterances
                    for i2 in range(M):
                        if i2 != i:
                            demb[j, i2] += g * parts[k][2] / (M - 1)
                else:
                    dcen[k] += g * parts[k][2]
    demb += dcen[:, None, :] / M
    return loss, demb, dw, db
