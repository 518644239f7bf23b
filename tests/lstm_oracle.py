"""Plain numpy float64 restatement of what ``csrc/lstm.hip`` computes: the LSTM stack with a
hand-written backward (every intermediate per layer and step), the discriminator head with
explicit dropout keep-scales, the BCE rows and their gradient, the 150-frame re-padding and
the label repeat.  A helper for the discriminator kernel tests, not a test; it uses no GPU,
no project kernel and no autograd.

Layouts are those of the C ABI (``include/fs2hip.h``): gate order i, f, g, o along 4H,
h0 = c0 = 0, batch_first; ``w_ih = (w_ih0 (4H, D), w_ih_up (L-1, 4H, H) or None)``,
``w_hh (L, 4H, H)``, ``bias (L, 4H)`` = b_ih + b_hh.
"""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _sigm(z):
    """1 / (1 + exp(-z)) without overflow at either end."""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def lstm_stack(x, w_ih, w_hh, bias, dh_out):
    """x (N, T, D); dh_out (N, T, H), the top layer's output gradient, or None for zero.

    Returns float64 arrays ``h``, ``c`` (L, N, T, H), ``act`` (L, N, T, 4H: the activated
    gates sigma(i), sigma(f), tanh(g), sigma(o)), ``dgates`` (L, N, T, 4H: the gradient of the
    pre-activations) and ``dx`` (N, T, D)."""
    x, w_hh, bias, dh_out = _f64(x), _f64(w_hh), _f64(bias), _f64(dh_out)
    w_ih0, w_ih_up = _f64(w_ih[0]), _f64(w_ih[1])
    N, T, _ = x.shape
    L, G, H = w_hh.shape
    assert G == 4 * H and bias.shape == (L, G) and (L == 1 or w_ih_up.shape == (L - 1, G, H))
    w_in = [w_ih0] + [w_ih_up[l - 1] for l in range(1, L)]
    h, c = np.zeros((L, N, T, H)), np.zeros((L, N, T, H))
    act = np.zeros((L, N, T, G))
    for l in range(L):
        below = x if l == 0 else h[l - 1]
        hp, cp = np.zeros((N, H)), np.zeros((N, H))
        for t in range(T):
            z = below[:, t] @ w_in[l].T + hp @ w_hh[l].T + bias[l]
            i, f, o = _sigm(z[:, :H]), _sigm(z[:, H:2 * H]), _sigm(z[:, 3 * H:])
            g = np.tanh(z[:, 2 * H:3 * H])
            cp = f * cp + i * g
            hp = o * np.tanh(cp)
            h[l, :, t], c[l, :, t] = hp, cp
            act[l, :, t] = np.concatenate([i, f, g, o], axis=1)
    dgates = np.zeros((L, N, T, G))
    for l in range(L - 1, -1, -1):
        dc_next = np.zeros((N, H))  # dL/dc_t carried from step t + 1: dc_{t+1} * f_{t+1}
        for t in range(T - 1, -1, -1):
            if l == L - 1:
                dh = dh_out[:, t].copy() if dh_out is not None else np.zeros((N, H))
            else:
                dh = dgates[l + 1, :, t] @ w_in[l + 1]
            if t + 1 < T:
                dh = dh + dgates[l, :, t + 1] @ w_hh[l]
            a = act[l, :, t]
            i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
            tc = np.tanh(c[l, :, t])
            cprev = c[l, :, t - 1] if t > 0 else np.zeros((N, H))
            dc = dc_next + dh * o * (1.0 - tc * tc)
            dgates[l, :, t] = np.concatenate(
                [dc * g * i * (1.0 - i), dc * cprev * f * (1.0 - f), dc * i * (1.0 - g * g),
                 dh * tc * o * (1.0 - o)], axis=1)
            dc_next = dc * f
    return {"h": h, "c": c, "act": act, "dgates": dgates, "dx": dgates[0] @ w_ih0}


HEAD_NAMES = ("wp", "bp", "w0", "b0", "w1", "b1", "w2", "b2")


def clf_head(x, weights, m0, m1, demb, dlogit):
    """Projection -> L2 norm -> two (Linear, keep-scale, ReLU) -> Linear.

    x (n, D); ``weights`` maps HEAD_NAMES to wp (P, D), bp (P), w0, w1 (P, P), b0, b1 (P),
    w2 (1, P), b2 (1); m0, m1 (n, P) are the dropout keep-scales of the two hidden layers
    (ones for p = 0, else entries 0 or 1 / (1 - p)) and multiply the pre-activation before
    the ReLU; demb (n, P) / dlogit (n) are the output gradients (None: zero).

    Returns ``emb`` (n, P), ``logit`` (n), ``dx`` (n, D), and the masked pre-activations
    ``z0``, ``z1`` (n, P), whose distance from 0 says how firmly each ReLU is decided."""
    x, m0, m1 = _f64(x), _f64(m0), _f64(m1)
    w = {k: _f64(weights[k]) for k in HEAD_NAMES}
    n = x.shape[0]
    p = x @ w["wp"].T + w["bp"]
    nrm = np.sqrt((p * p).sum(axis=1, keepdims=True))
    e = p / nrm
    z0 = (e @ w["w0"].T + w["b0"]) * m0
    a0 = np.maximum(z0, 0.0)
    z1 = (a0 @ w["w1"].T + w["b1"]) * m1
    a1 = np.maximum(z1, 0.0)
    logit = a1 @ w["w2"].reshape(-1) + w["b2"].reshape(())
    dl = _f64(dlogit) if dlogit is not None else np.zeros(n)
    de = _f64(demb).copy() if demb is not None else np.zeros_like(e)
    dz1 = np.where(a1 > 0, dl[:, None] * w["w2"].reshape(1, -1), 0.0) * m1
    dz0 = np.where(a0 > 0, dz1 @ w["w1"], 0.0) * m0
    de = de + dz0 @ w["w0"]
    dp = (de - e * (e * de).sum(axis=1, keepdims=True)) / nrm  # e = p / |p|
    return {"emb": e, "logit": logit, "dx": dp @ w["wp"], "z0": z0, "z1": z1}


def bce_rows(logit, y):
    """BCEWithLogits per row: max(x, 0) - x y + log(1 + exp(-|x|))."""
    x, y = _f64(logit), _f64(y)
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def dbce(logit, y, g, scale):
    """Its logit gradient times the upstream gradient g and the host scale."""
    return float(g) * float(scale) * (_sigm(_f64(logit)) - _f64(y))


def repad(x, t_dst):
    """(B, T_src, C) -> (B, t_dst, C): the first min(T_src, t_dst) frames, zeros after."""
    x = np.asarray(x)
    B, Ts, C = x.shape
    out = np.zeros((B, t_dst, C), dtype=x.dtype)
    k = min(Ts, t_dst)
    out[:, :k] = x[:, :k]
    return out


def repeat_col(meta, col, rep):
    """y[b * rep + k] = meta[b, col]."""
    return np.repeat(np.asarray(meta)[:, col], rep)
