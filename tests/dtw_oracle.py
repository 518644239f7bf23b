"""numpy fp64 oracle of the objective synthesis metrics (csrc/metrics.hip): the DTW recurrence
swept by anti-diagonals, its backtrack, the records along the path, and scipy's DCT as the MFCC.

    c(i, j) = sqrt(sum_k (a_ik - b_jk)^2)            (fp32 inputs cast to fp64 first)
    D(0, 0) = c(0, 0)
    D(i, j) = c(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1))

with a predecessor outside the matrix +inf and the FIRST minimum in that order taken at a tie:
one fp64 add per cell, so a kernel that keeps to it matches bit for bit wherever c is exact."""
import numpy as np

FIELDS = ("path_len", "mcd_db", "frames_a", "frames_b", "n_vv", "f0_sq_cents", "n_vuv", "len_err")


def local_cost(a, b):
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def accumulate(a, b):
    """``(D, step)``: the accumulated cost (T1, T2) fp64 and the winning predecessor of every
    cell, 0 = (i-1, j-1), 1 = (i-1, j), 2 = (i, j-1) (0 at (0, 0), where there is none)."""
    c = local_cost(a, b)
    T1, T2 = c.shape
    D = np.full((T1 + 1, T2 + 1), np.inf)  # one border row and column of +inf
    step = np.zeros((T1, T2), np.int8)
    for d in range(T1 + T2 - 1):
        i = np.arange(max(0, d - (T2 - 1)), min(d, T1 - 1) + 1)
        j = d - i
        cand = np.stack([D[i, j], D[i, j + 1], D[i + 1, j]])  # diagonal, (i-1, j), (i, j-1)
        s = np.argmin(cand, axis=0)  # the first minimum
        step[i, j] = s
        D[i + 1, j + 1] = c[i, j] + cand[s, np.arange(len(i))] if d else c[0, 0]
    return D[1:, 1:], step


def backtrack(step):
    i, j = step.shape[0] - 1, step.shape[1] - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        s = step[i, j]
        i, j = (i - 1, j - 1) if s == 0 else (i - 1, j) if s == 1 else (i, j - 1)
        path.append((i, j))
    return np.asarray(path[::-1], np.int32)


def dtw(a, b):
    """``(cost, path (n, 2) int32 from (0, 0) to (T1-1, T2-1))``."""
    D, step = accumulate(a, b)
    return D[-1, -1], backtrack(step)


def path_gap(a, b):
    """The smallest gap between the best and the second-best predecessor along the optimal path
    (cells with one predecessor inside the matrix do not count): 0 means an exact tie, and a
    path comparison is only meaningful where this is far above rounding."""
    D, step = accumulate(a, b)
    Dp = np.full((D.shape[0] + 1, D.shape[1] + 1), np.inf)
    Dp[1:, 1:] = D
    gap = np.inf
    for i, j in backtrack(step):
        cand = np.sort([Dp[i, j], Dp[i, j + 1], Dp[i + 1, j]])
        if np.isfinite(cand[1]):
            gap = min(gap, cand[1] - cand[0])
    return gap


def path_ties(a, b):
    """How many cells of the optimal path had an exact tie for the minimum."""
    D, step = accumulate(a, b)
    Dp = np.full((D.shape[0] + 1, D.shape[1] + 1), np.inf)
    Dp[1:, 1:] = D
    n = 0
    for i, j in backtrack(step):
        cand = np.sort([Dp[i, j], Dp[i, j + 1], Dp[i + 1, j]])
        n += bool(np.isfinite(cand[1]) and cand[1] == cand[0])
    return n


def brute_force(a, b):
    """Every monotone path of a small pair -> ``(minimum cost, the first-minimum path)``.  The
    costs are summed from (0, 0) on, as the recurrence does; among paths of the minimum cost the
    recurrence's tie rule, applied from the end backwards, prefers the diagonal step, then
    (i-1, j), then (i, j-1): the lexicographically smallest sequence of step codes read from the
    end."""
    c = local_cost(a, b)
    T1, T2 = c.shape
    best = [None, None]

    def walk(i, j, total, codes, cells):
        if (i, j) == (T1 - 1, T2 - 1):
            key = (total, codes[::-1])
            if best[0] is None or key < best[0]:
                best[:] = [key, list(cells)]
            return
        for s, (ni, nj) in enumerate(((i + 1, j + 1), (i + 1, j), (i, j + 1))):
            if ni < T1 and nj < T2:
                cells.append((ni, nj))
                walk(ni, nj, total + c[ni, nj], codes + (s,), cells)
                cells.pop()

    walk(0, 0, c[0, 0], (), [(0, 0)])
    return best[0][0], np.asarray(best[1], np.int32)


def path_metrics(cost, path, frames_a, frames_b, fa=None, fb=None):
    """The record of one pair, in the order of ``FIELDS``."""
    n = len(path)
    vv = sq = vuv = 0.0
    if fa is not None:
        x = np.asarray(fa, np.float32).astype(np.float64)[path[:, 0]]
        y = np.asarray(fb, np.float32).astype(np.float64)[path[:, 1]]
        both = (x > 0) & (y > 0)
        vv = float(both.sum())
        sq = float(((1200.0 * np.log2(x[both] / y[both])) ** 2).sum())
        vuv = float(((x > 0) != (y > 0)).sum())
    return np.array([n, 10.0 / np.log(10.0) * np.sqrt(2.0) * cost / n, frames_a, frames_b, vv, sq,
                     vuv, (frames_a - frames_b) / frames_b], np.float64)


def mfcc(logmel, n_coef=13):
    """logmel (..., n_mels) -> (..., n_coef): coefficients 1..n_coef of the orthonormal DCT-II."""
    from scipy.fft import dct
    return dct(np.asarray(logmel, np.float64), type=2, norm="ortho", axis=-1)[..., 1:n_coef + 1]
