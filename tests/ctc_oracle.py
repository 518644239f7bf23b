"""Oracle of the phoneme-error-rate kernels (csrc/ctc.hip, recognizer.py): numpy / torch on the
CPU, written from the definitions and not from the kernels.

  ctc                  nll and d nll / d logits by explicit alpha / beta over the 2L + 1
                       blank-interleaved states, numpy fp64, with the rules for rows without a path
  greedy               per-frame arg-max (NaN never wins, ties to the lowest class, an all-NaN frame
                       is blank), repeats collapsed, blanks dropped
  edit_distance        the Levenshtein table with the traceback's tie order: diagonal, deletion,
                       insertion -> (distance, substitutions, deletions, insertions)
  edit_distance_plain  a second DP, two rows and no traceback, for the distance alone
  TorchRecognizer      the model in plain torch modules; ``train`` / ``per`` on
                       ``align_oracle.synth_corpus``
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import align_oracle as AO


# ------------------------------------------------------------------ CTC
def has_path(target, M, C, blank):
    target = [int(v) for v in target]
    if any(v < 0 or v >= C or v == blank for v in target):
        return False
    repeats = sum(1 for a, b in zip(target, target[1:]) if a == b)
    return M >= len(target) + repeats


def _lse(*xs):
    xs = np.stack(xs)
    m = xs.max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        safe = np.where(np.isfinite(m), m, 0.0)
        out = safe + np.log(np.exp(xs - safe).sum(0))
    return np.where(m == -np.inf, -np.inf, out)


def ctc(logits, target, M, C, blank=0):
    """logits (>= M, >= C) fp32 (or fp64), target a sequence of L labels -> ``(nll, grad (M, C) =
    d nll / d logits)``, numpy fp64.  The first M frames' first C columns are log-softmaxed; the
    states are z = [blank, target[0], blank, target[1], .., blank].  A row without a valid path
    (fewer frames than labels plus adjacent repeats, a label outside [0, C), a label equal to
    blank): ``(inf, zeros)``."""
    L = len(target)
    if not has_path(target, M, C, blank):
        return np.inf, np.zeros((M, C))
    x = np.asarray(logits, np.float64)[:M, :C]
    mx = x.max(1, keepdims=True)
    y = x - (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))
    S = 2 * L + 1
    z = np.full(S, blank, np.int64)
    z[1::2] = np.asarray(target, np.int64)
    e = y[:, z]  # (M, S)
    skip = np.zeros(S, bool)  # j-2 -> j: between two different labels
    skip[3::2] = z[3::2] != z[1:-2:2]
    ninf = -np.inf

    def shifted(v, k):  # v[j - k], -inf outside
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
        alpha[t] = e[t] + _lse(p, shifted(p, 1), np.where(skip, shifted(p, 2), ninf))
    skip_out = np.zeros(S, bool)
    skip_out[:S - 2] = skip[2:]
    beta = np.full((M, S), ninf)
    beta[M - 1, max(S - 2, 0):] = e[M - 1, max(S - 2, 0):]
    for t in range(M - 2, -1, -1):
        p = beta[t + 1]
        beta[t] = e[t] + _lse(p, shifted(p, -1), np.where(skip_out, shifted(p, -2), ninf))
    ll = float(_lse(alpha[M - 1, S - 1], alpha[M - 1, S - 2] if S > 1 else np.float64(ninf)))
    with np.errstate(invalid="ignore"):
        occ = np.exp(alpha + beta - e - ll)
    occ = np.where(np.isfinite(alpha) & np.isfinite(beta), occ, 0.0)
    gamma = np.zeros((M, C))
    for j in range(S):  # repeated labels land on the same column
        gamma[:, z[j]] += occ[:, j]
    return -ll, np.exp(y) - gamma


def ctc_torch(logits, targets, frame_lens, target_lens, C, blank=0):
    """``F.ctc_loss`` after ``F.log_softmax`` over the first C columns of a padded batch
    (B, T, ld): nll (B), differentiable in the logits."""
    y = F.log_softmax(logits[:, :, :C], dim=2).transpose(0, 1)
    return F.ctc_loss(y, torch.as_tensor(targets), torch.as_tensor(frame_lens),
                      torch.as_tensor(target_lens), blank=blank, reduction="none",
                      zero_infinity=False)


# ------------------------------------------------------------------ greedy decoding
def argmax_frames(logits, M, C, blank=0):
    x = np.asarray(logits, np.float32)[:M, :C]
    out = np.full(M, blank, np.int64)
    for t in range(M):
        valid = np.flatnonzero(~np.isnan(x[t]))  # a NaN never wins; none left: the blank
        if len(valid):
            out[t] = valid[np.argmax(x[t, valid])]  # the first of equal maxima: the lowest class
    return out


def greedy(logits, M, C, blank=0):
    """The labels (int64 array) of the greedy CTC transcription of the first M frames."""
    am = argmax_frames(logits, M, C, blank)
    keep = [int(am[t]) for t in range(M) if am[t] != blank and (t == 0 or am[t] != am[t - 1])]
    return np.asarray(keep, np.int64)


# ------------------------------------------------------------------ edit distance
def edit_distance(ref, hyp):
    """``(distance, substitutions, deletions, insertions)``: unit costs, one table, the
    predecessor at each cell preferred in the order diagonal (match or substitution), deletion (a
    reference symbol without a partner), insertion; traced back from the last cell."""
    R, H = len(ref), len(hyp)
    D = np.zeros((R + 1, H + 1), np.int64)
    step = np.zeros((R + 1, H + 1), np.int8)
    D[:, 0], D[0, :] = np.arange(R + 1), np.arange(H + 1)
    step[1:, 0], step[0, 1:] = 1, 2
    for i in range(1, R + 1):
        for j in range(1, H + 1):
            best, s = D[i - 1, j - 1] + (ref[i - 1] != hyp[j - 1]), 0
            if D[i - 1, j] + 1 < best:
                best, s = D[i - 1, j] + 1, 1
            if D[i, j - 1] + 1 < best:
                best, s = D[i, j - 1] + 1, 2
            D[i, j], step[i, j] = best, s
    i, j, sub, dele, ins = R, H, 0, 0, 0
    while i > 0 or j > 0:
        s = step[i, j]
        if s == 0:
            sub += int(ref[i - 1] != hyp[j - 1])
            i, j = i - 1, j - 1
        elif s == 1:
            dele, i = dele + 1, i - 1
        else:
            ins, j = ins + 1, j - 1
    return int(D[R, H]), sub, dele, ins


def edit_distance_plain(ref, hyp):
    """The Levenshtein distance alone: two rows over the hypothesis, no traceback."""
    prev = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        cur = [i]
        for j, h in enumerate(hyp, 1):
            cur.append(min(prev[j - 1] + (r != h), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


# ------------------------------------------------------------------ the model in plain torch
def padded_classes(n_symbols):
    return (n_symbols + 7) // 8 * 8


class TorchRecognizer(nn.Module):
    """``recognizer.PhonemeRecognizer`` in torch modules, same state-dict keys (the output layer
    padded to a multiple of 8 classes as there): activations (B, T, C) there are (B, C, T) here.
    With ``mel_lens`` the mel and every hidden layer are zeroed at and past each row's length."""

    def __init__(self, n_symbols, n_mels=80, channels=256, layers=4, kernel=5):
        super().__init__()
        self.n_symbols = n_symbols
        self.convs = nn.ModuleList([nn.Conv1d(n_mels if i == 0 else channels, channels, kernel,
                                              padding=kernel // 2) for i in range(layers)])
        self.out = nn.Conv1d(channels, padded_classes(n_symbols), 1)

    def forward(self, mels, mel_lens=None):
        """mels (B, T, n_mels) -> logits (B, T, ld)."""
        x = mels.transpose(1, 2)
        live = None
        if mel_lens is not None:
            live = (torch.arange(mels.shape[1])[None, :] < torch.as_tensor(mel_lens)[:, None])
            live = live[:, None, :]
            x = torch.where(live, x, torch.zeros_like(x))
        for c in self.convs:
            x = torch.relu(c(x))
            if live is not None:
                x = torch.where(live, x, torch.zeros_like(x))
        return self.out(x).transpose(1, 2)

    def loss(self, texts, src_lens, mels, mel_lens):
        """(1 / B) sum_b nll_b / M_b."""
        logits = self(mels, mel_lens)
        nll = ctc_torch(logits, texts, mel_lens, src_lens, self.n_symbols)
        return (nll / torch.as_tensor(mel_lens, dtype=logits.dtype)).mean()

    def transcribe(self, mels, mel_lens):
        with torch.no_grad():
            logits = self(mels, mel_lens).float().numpy()
        return [greedy(logits[b], int(mel_lens[b]), self.n_symbols) for b in range(len(mels))]


# ------------------------------------------------------------------ the synthetic corpus
CHANNELS, LAYERS, KERNEL, LR, STEPS = 64, 2, 3, 3e-3, 300
N_CLASSES = AO.N_SYMBOLS + 1  # ids 1..12 and the blank / padding 0


def new_model(seed):
    torch.manual_seed(seed)
    return TorchRecognizer(N_CLASSES, AO.N_MELS, CHANNELS, LAYERS, KERNEL)


def train(model, corpus, seed, steps=STEPS):
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    losses = []
    for idx in AO.batch_order(seed, steps):
        opt.zero_grad()
        loss = model.loss(*AO.take(corpus, idx))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def per_of(hyps, corpus, shift=0):
    """sum of distances / sum of reference lengths; ``shift``: utterance u's transcription is
    scored against the text of utterance u + shift."""
    U = len(corpus["src_lens"])
    dist = total = 0
    for u in range(U):
        r = (u + shift) % U
        ref = corpus["texts"][r, :int(corpus["src_lens"][r])]
        dist += edit_distance(ref, hyps[u])[0]
        total += len(ref)
    return dist / total


def synth(seed):
    corpus = AO.synth_corpus(seed)
    return corpus, AO.take(corpus, np.arange(AO.N_UTT))


def oracle_per(seed, steps=STEPS):
    """(untrained, trained, trained against the next utterance's text) PER of the torch model on
    ``synth_corpus(seed)``."""
    corpus, (_, _, mels, mel_lens) = synth(seed)
    model = new_model(seed)
    before = per_of(model.transcribe(mels, mel_lens), corpus)
    train(model, corpus, seed, steps)
    hyps = model.transcribe(mels, mel_lens)
    return before, per_of(hyps, corpus), per_of(hyps, corpus, shift=1)


def targets_with_repeats(rng, L, C, blank, repeats):
    """L labels in [0, C) \\ {blank}, adjacent ones distinct but for ``repeats`` forced pairs."""
    labels = [c for c in range(C) if c != blank]
    out = []
    for _ in range(L):
        c = labels[int(rng.integers(len(labels)))]
        while out and c == out[-1] and len(labels) > 1:
            c = labels[int(rng.integers(len(labels)))]
        out.append(c)
    for p in rng.choice(np.arange(1, L), size=repeats, replace=False) if repeats else []:
        out[int(p)] = out[int(p) - 1]
    return np.asarray(out, np.int64)
