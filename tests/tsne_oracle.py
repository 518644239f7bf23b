"""numpy transcription of scikit-learn's exact t-SNE (``sklearn/manifold/_t_sne.py`` and
``_utils.pyx``), written for the tests of ``embedding_map`` and ``csrc/tsne.hip``: the perplexity
search, the joint probabilities, the objective and its gradient, one descent step, the control
rules of ``_gradient_descent`` over the two stages of ``TSNE._tsne``, the PCA initialisation
(full SVD instead of scikit-learn's randomised one) and the seeded test points.

Everything takes a ``dtype``: float64 is the reference; float32 is the same arithmetic in
single precision, whose deviation from float64 sizes the tolerances of the GPU tests.
"""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)       # MACHINE_EPSILON
ZERO_SUM = float(np.float32(1e-8))          # _utils.pyx: cdef float EPSILON_DBL
TOL = float(np.float32(1e-5))               # _utils.pyx: cdef float PERPLEXITY_TOLERANCE
N_ITER_CHECK = 50


def make_points(n_per, groups, D, seed):
    """(n_per * groups, D) float32 unit-norm cluster points: normal centres plus 0.35 * normal
    noise, renormalised."""
    rng = np.random.RandomState(seed)
    centres = rng.standard_normal((groups, D))
    x = np.repeat(centres, n_per, axis=0) + 0.35 * rng.standard_normal((groups * n_per, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, np.float32)


def sq_distances(X):
    """Squared Euclidean distances from the direct (x_i - x_j)^2 form, summed in float64 and
    rounded to float32 (the search reads float32 distances)."""
    X = np.asarray(X, np.float64)
    diff = X[:, None, :] - X[None, :, :]
    return np.einsum("ijd,ijd->ij", diff, diff).astype(np.float32)


def binary_search(dist32, perplexity, n_steps=100):
    """_binary_search_perplexity: (conditional P (N, N) float64, beta (N), entropy (N))."""
    d = np.asarray(dist32, np.float32).astype(np.float64)
    n = d.shape[0]
    target = math.log(float(np.float32(perplexity)))
    P = np.zeros((n, n))
    betas, ents = np.zeros(n), np.zeros(n)
    for i in range(n):
        lo, hi, beta = -np.inf, np.inf, 1.0
        off = np.arange(n) != i
        for _ in range(n_steps):
            p = np.where(off, np.exp(-d[i] * beta), 0.0)
            s = float(np.cumsum(p)[-1])  # cumsum adds in index order, as the reference does
            if s == 0.0:
                s = ZERO_SUM
            p = p / s
            sd = float(np.cumsum(d[i] * p)[-1])
            ent = math.log(s) + beta * sd
            diff = ent - target
            P[i] = p
            if abs(diff) <= TOL:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        betas[i], ents[i] = beta, ent
    return P, betas, ents


def joint_probabilities(X, perplexity):
    """Dense (N, N) float64 P of _joint_probabilities (zero diagonal), beta, entropies."""
    C, beta, ent = binary_search(sq_distances(X), perplexity)
    P = C + C.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P, beta, ent


def _pairs(Y, dtype):
    Y = np.asarray(Y, dtype)
    diff = Y[:, None, :] - Y[None, :, :]
    w = (dtype(1.0) / (dtype(1.0) + (diff * diff).sum(-1, dtype=dtype))).astype(dtype)
    np.fill_diagonal(w, 0.0)
    return diff, w


def kl_grad(Y, P, exaggeration=1.0, dtype=np.float64):
    """_kl_divergence on dense operands: (KL, grad (N, 2)) of the embedding Y under
    ``exaggeration * P``."""
    dtype = np.dtype(dtype).type
    diff, w = _pairs(Y, dtype)
    off = ~np.eye(len(w), dtype=bool)
    Q = np.maximum(w / w.sum(dtype=dtype), dtype(EPS)).astype(dtype)
    Pe = (np.asarray(P, dtype) * dtype(exaggeration)).astype(dtype)
    terms = np.where(off, Pe * np.log(np.maximum(Pe, dtype(EPS)) / Q), 0).astype(dtype)
    kl = terms.sum(dtype=dtype)
    pqd = np.where(off, (Pe - Q) * w, 0).astype(dtype)
    grad = dtype(4.0) * (pqd[:, :, None] * diff).sum(1, dtype=dtype)
    return dtype(kl), grad.astype(dtype)


def step(Y, update, gains, P, exaggeration, momentum, lr, dtype=np.float64):
    """One iteration of _gradient_descent's body: (Y', update', gains', KL of Y, ||gains *
    grad||, update * grad before the gains)."""
    dtype = np.dtype(dtype).type
    Y, update, gains = (np.array(a, dtype) for a in (Y, update, gains))
    kl, grad = kl_grad(Y, P, exaggeration, dtype)
    ug = update * grad
    inc = ug < 0.0
    gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8)).astype(dtype)
    gains = np.maximum(gains, dtype(0.01))
    grad = grad * gains
    update = (dtype(momentum) * update - dtype(lr) * grad).astype(dtype)
    return (Y + update).astype(dtype), update, gains, kl, float(np.linalg.norm(grad)), ug


class Control:
    """The rules of _gradient_descent and of the two stages of TSNE._tsne as a state record:
    ``begin(i)`` gives the iteration's (exaggeration, momentum, evaluate error?, reset update
    and gains?), ``end(i, error, grad_norm)`` applies the checks.  Stage 1 runs to
    ``exploration_iter`` whatever ``max_iter`` is, as TSNE._tsne's does; where it ends at or past
    ``max_iter - 1`` there is no stage 2 (scikit-learn, which demands max_iter >= 250, would
    call an empty second descent there)."""

    def __init__(self, max_iter=1000, exploration_iter=250, n_iter_without_progress=300,
                 min_grad_norm=1e-7, early_exaggeration=12.0):
        self.max_iter, self.exploration_iter = int(max_iter), int(exploration_iter)
        self.window2, self.min_grad_norm = n_iter_without_progress, min_grad_norm
        self.early_exaggeration = early_exaggeration
        self.stage, self.start = 1, 0
        self.best, self.best_iter = np.finfo(np.float64).max, 0
        self.done, self.n_iter, self.error = False, -1, float("nan")

    def _last(self):
        return (self.exploration_iter if self.stage == 1 else self.max_iter) - 1

    def begin(self, i):
        check = (i + 1) % N_ITER_CHECK == 0
        first = self.stage == 1
        return (self.early_exaggeration if first else 1.0, 0.5 if first else 0.8,
                check or i == self._last(), self.stage == 2 and i == self.start)

    def end(self, i, error, grad_norm):
        if self.done:
            return
        check = (i + 1) % N_ITER_CHECK == 0
        if check or i == self._last():
            self.error = float(error)
        stop = False
        if check:
            window = self.exploration_iter if self.stage == 1 else self.window2
            if error < self.best:
                self.best, self.best_iter = float(error), i
            elif i - self.best_iter > window:
                stop = True
            if not stop and grad_norm <= self.min_grad_norm:
                stop = True
        if stop or i == self._last():
            if self.stage == 1 and i + 1 < self.max_iter:
                self.stage, self.start = 2, i + 1
                self.best, self.best_iter = np.finfo(np.float64).max, i + 1
            else:
                self.done, self.n_iter = True, i


def run(Y0, P, lr, dtype=np.float64, **control):
    """TSNE._tsne: (Y, kl_divergence_, n_iter_)."""
    dtype = np.dtype(dtype).type
    c = Control(**control)
    Y = np.array(Y0, dtype)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    for i in range(max(c.max_iter, c.exploration_iter)):
        ex, mom, _, reset = c.begin(i)
        if reset:
            update, gains = np.zeros_like(Y), np.ones_like(Y)
        Y, update, gains, kl, gn, _ = step(Y, update, gains, P, ex, mom, lr, dtype)
        c.end(i, kl, gn)
        if c.done:
            break
    return Y, c.error, c.n_iter


def auto_lr(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def pca_init(X):
    """PCA to 2 components by a full SVD in float64, signs as svd_flip's V-based rule (each
    component's largest-magnitude loading positive), scaled so the first column has standard
    deviation 1e-4; float32.  Also returns the singular values."""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0)
    _, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    V = Vt[:2]
    sign = np.sign(V[np.arange(2), np.abs(V).argmax(1)])
    Y = Xc @ (V * sign[:, None]).T
    return (Y / np.std(Y[:, 0]) * 1e-4).astype(np.float32), S
