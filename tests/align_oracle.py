"""Oracle of the aligner (csrc/align.hip, aligner.py): numpy / torch on the CPU, written from the
definitions and not from the kernels.

  log_prior      the log beta-binomial prior, fp64
  logprob        log_softmax_s(-temperature |q_t - k_s|^2) + prior, torch fp64 (differentiable)
  forward_sum    the CTC forward-sum loss of the target 1..N and its gradient by explicit
                 alpha / beta over the 2N + 1 interleaved states, numpy fp64
  mas            monotonic alignment search in numpy fp32, one add and one compare per cell
  mas_brute      the same by enumeration of every monotonic path
  TorchAligner   the model in plain torch modules; ``train`` / ``agreement`` on ``synth_corpus``
"""
import itertools
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

BLANK_SCORE = -1.0


# ------------------------------------------------------------------ prior and log-probabilities
def log_prior(N, M, omega):
    """(M, N) fp64: log BetaBinomial(s; n = N - 1, a = omega (t + 1), b = omega (M - t))."""
    lg = np.vectorize(math.lgamma, otypes=[np.float64])
    n = N - 1
    s = np.arange(N, dtype=np.float64)[None, :]
    t = np.arange(M, dtype=np.float64)[:, None]
    a, b = omega * (t + 1.0), omega * (M - t)
    comb = lg(n + 1.0) - lg(s + 1.0) - lg(n - s + 1.0)
    return comb + lg(s + a) + lg(n - s + b) - lg(n + a + b) - (lg(a) + lg(b) - lg(a + b))


def logprob(q, k, N, M, temperature, omega):
    """q (T_m, A), k (T_s, A) torch -> (T_m, T_s) fp64, dead cells 0; differentiable in q, k."""
    q64, k64 = q.double(), k.double()
    T_m, T_s = q.shape[0], k.shape[0]
    d = ((q64[:M, None, :] - k64[None, :N, :]) ** 2).sum(-1)
    lp = torch.log_softmax(-float(temperature) * d, dim=1)
    if omega > 0:
        lp = lp + torch.from_numpy(log_prior(N, M, float(omega)))
    return F.pad(lp, (0, T_s - N, 0, T_m - M))


# ------------------------------------------------------------------ forward-sum (CTC)
def forward_sum(logp, N, M):
    """logp (>= M, >= N) -> ``(nll, grad (M, N) = d nll / d logp)``, numpy fp64.  Frame t's N + 1
    scores [BLANK_SCORE, logp[t, :N]] are log-softmaxed; the target is 1..N (state 2s + 1 = label
    s, even states blank).  ``M < N``: ``(inf, zeros)``."""
    x = np.asarray(logp, np.float64)[:M, :N]
    if M < N:
        return np.inf, np.zeros((M, N))
    sc = np.concatenate([np.full((M, 1), BLANK_SCORE), x], 1)
    mx = sc.max(1, keepdims=True)
    y = sc - (mx + np.log(np.exp(sc - mx).sum(1, keepdims=True)))  # (M, N + 1) log-softmax
    S = 2 * N + 1
    j = np.arange(S)
    e = y[:, np.where(j % 2 == 0, 0, (j + 1) // 2)]  # (M, S) emission of each state
    skip = (j % 2 == 1) & (j >= 2)                   # label to the next (distinct) label
    ninf = -np.inf

    def lse3(a, b, c):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.maximum(a, np.maximum(b, c))
            safe = np.where(m == ninf, 0.0, m)
            out = safe + np.log(np.exp(a - safe) + np.exp(b - safe) + np.exp(c - safe))
        return np.where(m == ninf, ninf, out)

    def shift(v, k):  # v[j - k], -inf outside (k < 0: v[j + |k|])
        out = np.full(S, ninf)
        if k > 0:
            out[k:] = v[:S - k]
        else:
            out[:S + k] = v[-k:]
        return out

    alpha = np.full((M, S), ninf)
    alpha[0, :2] = e[0, :2]
    for t in range(1, M):
        p = alpha[t - 1]
        alpha[t] = e[t] + lse3(p, shift(p, 1), np.where(skip, shift(p, 2), ninf))
    beta = np.full((M, S), ninf)
    beta[M - 1, S - 2:] = e[M - 1, S - 2:]
    skip_out = (j % 2 == 1) & (j + 2 < S)
    for t in range(M - 2, -1, -1):
        p = beta[t + 1]
        beta[t] = e[t] + lse3(p, shift(p, -1), np.where(skip_out, shift(p, -2), ninf))
    ll = float(lse3(alpha[M - 1, S - 1], alpha[M - 1, S - 2], ninf))
    lab = 2 * np.arange(N) + 1
    with np.errstate(invalid="ignore"):
        occ = np.exp(alpha[:, lab] + beta[:, lab] - e[:, lab] - ll)
    occ = np.where(np.isfinite(alpha[:, lab]) & np.isfinite(beta[:, lab]), occ, 0.0)
    grad = np.exp(e[:, lab]) - occ
    return -ll, grad


def forward_sum_torch(logp, src_lens, mel_lens, dtype=torch.float64):
    """The same loss through ``F.ctc_loss`` for a padded batch (B, T_m, T_s): ``nll`` (B),
    differentiable.  Used to check ``forward_sum`` and to train the oracle model."""
    B, T_m, T_s = logp.shape
    live = torch.arange(T_s)[None, None, :] < torch.as_tensor(src_lens)[:, None, None]
    x = F.pad(logp.to(dtype), (1, 0), value=BLANK_SCORE)
    mask = F.pad(live, (1, 0), value=True).expand(B, T_m, T_s + 1)
    x = x.masked_fill(~mask, -1e30)  # classes past a row's N take no mass
    y = torch.log_softmax(x, dim=2).transpose(0, 1)  # (T_m, B, C)
    targets = torch.arange(1, T_s + 1)[None, :].expand(B, T_s)
    return F.ctc_loss(y, targets, torch.as_tensor(mel_lens), torch.as_tensor(src_lens), blank=0,
                      reduction="none", zero_infinity=False)


# ------------------------------------------------------------------ monotonic alignment search
def mas(logp, N, M):
    """Durations (N) int64 of the best monotonic path, fp32: V[0, 0] = logp[0, 0], V[0, s > 0] =
    -inf, V[t, s] = logp[t, s] + max(V[t-1, s-1], V[t-1, s]), the diagonal on a tie."""
    if M < N:
        raise ValueError(f"{M} frames for {N} phonemes")
    x = np.asarray(logp, np.float32)[:M, :N]
    V = np.full((M, N), -np.inf, np.float32)
    diag = np.zeros((M, N), bool)
    V[0, 0] = x[0, 0]
    for t in range(1, M):
        dg = np.concatenate([np.float32([-np.inf]), V[t - 1, :-1]])
        up = V[t - 1]
        diag[t] = dg >= up
        V[t] = x[t] + np.where(diag[t], dg, up)  # one IEEE fp32 add per cell
    dur = np.zeros(N, np.int64)
    s = N - 1
    for t in range(M - 1, -1, -1):
        dur[s] += 1
        if t > 0 and s > 0 and diag[t, s]:
            s -= 1
    assert s == 0
    return dur


def mas_brute(logp, N, M):
    """``(best score, durations)`` over every split of M frames into N runs of >= 1 frame, the
    score summed in fp64 (exact for small integers).  Among equal-score paths the one the tie rule
    reaches: walking back from the last frame it steps down to s - 1 as soon as an optimal path
    allows, i.e. the smallest (s_{M-1}, s_{M-2}, ..) sequence."""
    x = np.asarray(logp, np.float64)[:M, :N]
    best = None
    for cuts in itertools.combinations(range(1, M), N - 1):
        edges = (0,) + cuts + (M,)
        dur = np.diff(edges)
        path = np.repeat(np.arange(N), dur)
        score = float(x[np.arange(M), path].sum())
        key = (-score, tuple(path[::-1]))
        if best is None or key < best[0]:
            best = (key, score, dur.astype(np.int64))
    return best[1], best[2]


def path_of(durations):
    return np.repeat(np.arange(len(durations)), np.asarray(durations, np.int64))


# ------------------------------------------------------------------ the model in plain torch
class TorchAligner(nn.Module):
    """``aligner.Aligner`` in torch modules, same state-dict keys: activations (B, T, C) there are
    (B, C, T) here."""

    def __init__(self, n_symbols, n_mels=80, channels=64, attn_dim=40):
        super().__init__()
        self.embedding = nn.Embedding(n_symbols, channels, padding_idx=0)
        self.key = nn.ModuleList([nn.Conv1d(channels, channels, 3, padding=1),
                                  nn.Conv1d(channels, attn_dim, 1)])
        self.query = nn.ModuleList([nn.Conv1d(n_mels, channels, 3, padding=1),
                                    nn.Conv1d(channels, channels, 1),
                                    nn.Conv1d(channels, attn_dim, 1)])

    def forward(self, texts, mels):
        """texts (B, T_s) int64, mels (B, T_m, n_mels) -> q (B, T_m, A), k (B, T_s, A)."""
        k = self.embedding(texts).transpose(1, 2)
        k = self.key[1](torch.relu(self.key[0](k)))
        q = mels.transpose(1, 2)
        q = self.query[2](torch.relu(self.query[1](torch.relu(self.query[0](q)))))
        return q.transpose(1, 2), k.transpose(1, 2)

    def logprob(self, texts, src_lens, mels, mel_lens, temperature, omega):
        q, k = self(texts, mels)
        return torch.stack([logprob(q[b], k[b], int(src_lens[b]), int(mel_lens[b]), temperature,
                                    omega) for b in range(len(texts))])

    def loss(self, texts, src_lens, mels, mel_lens, temperature, omega):
        """(1 / B) sum_b nll_b / M_b."""
        lp = self.logprob(texts, src_lens, mels, mel_lens, temperature, omega)
        nll = forward_sum_torch(lp, src_lens, mel_lens, lp.dtype)
        return (nll / torch.as_tensor(mel_lens, dtype=lp.dtype)).mean()

    def align(self, texts, src_lens, mels, mel_lens, temperature, omega):
        with torch.no_grad():
            lp = self.logprob(texts, src_lens, mels, mel_lens, temperature, omega).float().numpy()
        return [mas(lp[b], int(src_lens[b]), int(mel_lens[b])) for b in range(len(texts))]


# ------------------------------------------------------------------ the synthetic corpus
N_SYMBOLS, N_UTT, N_MELS = 12, 32, 80
CHANNELS, ATTN_DIM, TEMPERATURE, OMEGA, LR, BATCH, STEPS = 64, 40, 0.05, 1.0, 1e-3, 8, 100


def synth_corpus(seed):
    """12 symbols (ids 1..12, 0 is padding) with random 80-dimensional templates; 32 utterances of
    5-12 phonemes, no symbol twice in a row, 1-9 frames each; mel = template + 0.3 noise.  Padded
    arrays: texts (U, 12) int64, src_lens, mels (U, T_m, 80) f32, mel_lens, durations (U, 12)."""
    rng = np.random.default_rng(seed)
    templates = rng.standard_normal((N_SYMBOLS + 1, N_MELS)).astype(np.float32)
    utts = []
    for _ in range(N_UTT):
        n = int(rng.integers(5, 13))
        ids = []
        for _ in range(n):
            c = int(rng.integers(1, N_SYMBOLS + 1))
            while ids and c == ids[-1]:
                c = int(rng.integers(1, N_SYMBOLS + 1))
            ids.append(c)
        dur = rng.integers(1, 10, n)
        mel = templates[np.repeat(ids, dur)] + \
            0.3 * rng.standard_normal((int(dur.sum()), N_MELS)).astype(np.float32)
        utts.append((np.asarray(ids, np.int64), dur.astype(np.int64), mel.astype(np.float32)))
    T_s, T_m = 12, max(len(m) for _, _, m in utts)
    texts = np.zeros((N_UTT, T_s), np.int64)
    durations = np.zeros((N_UTT, T_s), np.int64)
    mels = np.zeros((N_UTT, T_m, N_MELS), np.float32)
    for u, (ids, dur, mel) in enumerate(utts):
        texts[u, :len(ids)], durations[u, :len(ids)], mels[u, :len(mel)] = ids, dur, mel
    return {"texts": texts, "src_lens": np.asarray([len(i) for i, _, _ in utts], np.int64),
            "mels": mels, "mel_lens": np.asarray([len(m) for _, _, m in utts], np.int64),
            "durations": durations}


def batch_order(seed, steps=STEPS, batch=BATCH, n=N_UTT):
    """The utterance indices of each training step: a fresh permutation per epoch."""
    rng = np.random.default_rng(1000 + seed)
    order, out = [], []
    for _ in range(steps):
        if len(order) < batch:
            order = list(rng.permutation(n))
        out.append(np.sort(np.asarray(order[:batch], np.int64)))
        order = order[batch:]
    return out


def take(corpus, idx):
    """One batch, cropped to its longest member: (texts, src_lens, mels, mel_lens) as torch."""
    sl, ml = corpus["src_lens"][idx], corpus["mel_lens"][idx]
    return (torch.from_numpy(corpus["texts"][idx][:, :sl.max()]), torch.from_numpy(sl),
            torch.from_numpy(corpus["mels"][idx][:, :ml.max()]), torch.from_numpy(ml))


def new_model(seed):
    torch.manual_seed(seed)
    return TorchAligner(N_SYMBOLS + 1, N_MELS, CHANNELS, ATTN_DIM)


def train(model, corpus, seed, steps=STEPS):
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    for idx in batch_order(seed, steps):
        opt.zero_grad()
        model.loss(*take(corpus, idx), TEMPERATURE, OMEGA).backward()
        opt.step()
    return model


def agreement(durations, corpus):
    """Fraction of frames whose phoneme on the given paths is the true one; ``durations`` is a
    list of per-utterance arrays (or a padded (U, T_s) array)."""
    hit = total = 0
    for u in range(len(corpus["src_lens"])):
        n = int(corpus["src_lens"][u])
        got, want = path_of(np.asarray(durations[u])[:n]), path_of(corpus["durations"][u, :n])
        hit += int((got == want).sum())
        total += len(want)
    return hit / total


def oracle_agreement(seed, steps=STEPS):
    """(untrained, trained) frame agreement of the torch model on ``synth_corpus(seed)``."""
    corpus = synth_corpus(seed)
    model = new_model(seed)
    everything = take(corpus, np.arange(N_UTT))
    before = agreement(model.align(*everything, TEMPERATURE, OMEGA), corpus)
    train(model, corpus, seed, steps)
    return before, agreement(model.align(*everything, TEMPERATURE, OMEGA), corpus)
