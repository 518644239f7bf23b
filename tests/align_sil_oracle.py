"""Oracle of the aligner's optional positions (``fs2_forward_sum_opt``, ``fs2_mas_opt``,
``align.parse_phn`` with ``optional_sil``): numpy / torch on the CPU, written from the
definitions and not from the kernels.  A marked position may take no frame; a valid labelling
keeps every unmarked position, never omits two neighbours and never omits all.

  valid_subsets          the kept-position tuples of every valid labelling
  forward_sum_opt        the forward-sum loss over those labellings and its gradient by explicit
                         alpha / beta over the state pairs (bl[s], la[s]), numpy fp64
  forward_sum_opt_torch  the same recursion in torch fp64 for a padded batch, differentiable
  forward_sum_opt_brute  -logsumexp over the kept subsets of ``F.ctc_loss``
  mas_opt                monotonic alignment search with skips in numpy fp32
  mas_opt_brute          the same by enumeration of every kept subset and every split
  PARSE                  ``.phn`` lines and what ``parse_phn(optional_sil="sp")`` makes of them
  synth_corpus_sil       ``align_oracle.synth_corpus`` in words, with pauses and edge silence
  agreement / pause_accuracy, ``oracle_run`` (the torch model trained with and without the mask)
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import align_oracle as O

BLANK_SCORE = O.BLANK_SCORE
NEG = -1e30  # a closed edge in the torch recursion: finite, so no gradient is ever NaN


def valid_subsets(optional):
    """Every tuple of kept positions: all unmarked ones, no two neighbours omitted, not empty."""
    opt = [bool(o) for o in optional]
    N, out = len(opt), []
    marked = [s for s in range(N) if opt[s]]
    for r in range(len(marked) + 1):
        for drop in itertools.combinations(marked, r):
            if any(b - a == 1 for a, b in zip(drop, drop[1:])) or len(drop) == N:
                continue
            out.append(tuple(s for s in range(N) if s not in drop))
    return out


def _lse(*xs):
    """Elementwise log-sum-exp of fp64 arrays, -inf where all are."""
    x = np.stack([np.asarray(v, np.float64) for v in np.broadcast_arrays(*xs)])
    m = x.max(0)
    safe = np.where(m == -np.inf, 0.0, m)
    with np.errstate(divide="ignore"):
        out = safe + np.log(np.exp(x - safe).sum(0))
    return np.where(m == -np.inf, -np.inf, out)


def _shift(v, k):
    """v[s - k], -inf outside (k < 0: v[s + |k|]); same length."""
    out = np.full(len(v), -np.inf)
    if k == 0:
        return v.copy()
    if abs(k) >= len(v):
        return out
    if k > 0:
        out[k:] = v[:len(v) - k]
    else:
        out[:len(v) + k] = v[-k:]
    return out


# ------------------------------------------------------------------ forward-sum
def forward_sum_opt(logp, N, M, optional):
    """logp (>= M, >= N), optional (>= N) -> ``(nll, grad (M, N) = d nll / d logp)``, numpy fp64.
    States: bl[s], s = 0..N (the blank before label s) and la[s], s < N.  Omitting a marked label
    u omits (la[u], bl[u+1]).  No valid path: ``(inf, zeros)``."""
    x = np.asarray(logp, np.float64)[:M, :N]
    opt = np.asarray(optional)[:N].astype(bool)
    sc = np.concatenate([np.full((M, 1), BLANK_SCORE), x], 1)
    mx = sc.max(1, keepdims=True)
    y = sc - (mx + np.log(np.exp(sc - mx).sum(1, keepdims=True)))
    eb, el = y[:, 0], y[:, 1:]                       # (M), (M, N)
    ninf = -np.inf
    o_prev = np.concatenate([[False], opt[:-1]])     # optional[s-1] at label s
    head, tail = N >= 2 and opt[0], N >= 2 and opt[N - 1]

    def closed(v, gate):
        return np.where(gate, v, ninf)

    a_la, a_bl = np.full((M, N), ninf), np.full((M, N + 1), ninf)
    a_bl[0, 0], a_la[0, 0] = eb[0], el[0, 0]
    if head:
        a_la[0, 1] = el[0, 1]
    for t in range(1, M):
        pl, pb = a_la[t - 1], a_bl[t - 1]
        pl_full = np.concatenate([pl, [ninf]])       # la[s] at s = 0..N (la[N] closed)
        a_bl[t] = eb[t] + _lse(pb, _shift(pl_full, 1))
        a_la[t] = el[t] + _lse(pl, pb[:N], _shift(pl, 1), closed(_shift(pb[:N], 1), o_prev),
                               closed(_shift(pl, 2), o_prev))
    ends = [a_bl[M - 1, N], a_la[M - 1, N - 1]]
    if tail:
        ends += [a_la[M - 1, N - 2], a_bl[M - 1, N - 1]]
    ll = float(_lse(*ends))
    if ll == ninf:
        return np.inf, np.zeros((M, N))
    b_la, b_bl = np.full((M, N), ninf), np.full((M, N + 1), ninf)
    b_bl[M - 1, N], b_la[M - 1, N - 1] = eb[M - 1], el[M - 1, N - 1]
    if tail:
        b_la[M - 1, N - 2], b_bl[M - 1, N - 1] = el[M - 1, N - 2], eb[M - 1]
    o_next = np.concatenate([opt[1:], [False]])      # optional[s+1] at label s
    for t in range(M - 2, -1, -1):
        nl, nb = b_la[t + 1], b_bl[t + 1]
        nl_full = np.concatenate([nl, [ninf]])
        opt_full = np.concatenate([opt, [False]])
        # bl[s] -> bl[s], la[s], and over an omitted label s to la[s+1]
        b_bl[t] = eb[t] + _lse(nb, nl_full, closed(_shift(nl_full, -1), opt_full))
        # la[s] -> la[s], bl[s+1], la[s+1], and over an omitted label s+1 to la[s+2]
        b_la[t] = el[t] + _lse(nl, nb[1:], _shift(nl, -1), closed(_shift(nl, -2), o_next))
    with np.errstate(invalid="ignore"):
        occ = np.exp(a_la + b_la - el - ll)
    occ = np.where(np.isfinite(a_la) & np.isfinite(b_la), occ, 0.0)
    return -ll, np.exp(el) - occ


def frame_scores(logp, src_lens, dtype=torch.float64):
    """(B, T_m, T_s + 1): the frames' log-softmax over [blank, logp[:, :N]], classes past a row's
    N closed.  What ``F.ctc_loss`` and the recursion below consume."""
    B, T_m, T_s = logp.shape
    live = torch.arange(T_s)[None, None, :] < torch.as_tensor(src_lens)[:, None, None]
    x = F.pad(logp.to(dtype), (1, 0), value=BLANK_SCORE)
    mask = F.pad(live, (1, 0), value=True).expand(B, T_m, T_s + 1)
    return torch.log_softmax(x.masked_fill(~mask, NEG), dim=2)


def forward_sum_opt_torch(logp, src_lens, mel_lens, optional, dtype=torch.float64):
    """``nll`` (B) of a padded batch (B, T_m, T_s) with ``optional`` (B, T_s), differentiable:
    the alpha recursion of ``forward_sum_opt`` in torch, closed edges at ``NEG``.  A row without a
    path comes out near ``-NEG`` (not inf)."""
    B, T_m, T_s = logp.shape
    src, mel = torch.as_tensor(src_lens), torch.as_tensor(mel_lens)
    y = frame_scores(logp, src, dtype)
    eb, el = y[:, :, 0], y[:, :, 1:]
    opt = torch.as_tensor(np.asarray(optional)).bool() & (torch.arange(T_s)[None, :] < src[:, None])
    o_prev = F.pad(opt[:, :-1], (1, 0), value=False)
    neg = torch.full((B, 1), NEG, dtype=dtype)
    head = opt[:, 0] & (src >= 2)

    def closed(v, gate):
        return torch.where(gate, v, torch.full_like(v, NEG))

    la = torch.full((B, T_s), NEG, dtype=dtype)
    bl = torch.full((B, T_s + 1), NEG, dtype=dtype)
    first = torch.zeros(B, T_s, dtype=torch.bool)
    first[:, 0] = True
    if T_s > 1:
        first[:, 1] = head
    la = torch.where(first, el[:, 0], la)
    bl = torch.cat([eb[:, :1], bl[:, 1:]], 1)
    las, bls = [la], [bl]
    for t in range(1, T_m):
        pl1 = torch.cat([neg, la], 1)                 # la[s-1] at s = 0..T_s
        pl2 = torch.cat([neg, neg, la[:, :-1]], 1)    # la[s-2] at s = 0..T_s
        pb1 = torch.cat([neg, bl[:, :-1]], 1)         # bl[s-1] at s = 0..T_s
        nbl = eb[:, t, None] + torch.logsumexp(torch.stack([bl, pl1]), 0)
        nla = el[:, t] + torch.logsumexp(torch.stack(
            [la, bl[:, :T_s], pl1[:, :T_s], closed(pb1[:, :T_s], o_prev),
             closed(pl2[:, :T_s], o_prev)]), 0)
        la, bl = nla, nbl
        las.append(la), bls.append(bl)
    las, bls = torch.stack(las, 1), torch.stack(bls, 1)  # (B, T_m, .)
    r = torch.arange(B)
    la_end, bl_end = las[r, mel - 1], bls[r, mel - 1]    # (B, T_s), (B, T_s + 1)
    tail = opt[r, src - 1] & (src >= 2)
    s2 = (src - 2).clamp(min=0)
    ends = torch.stack([bl_end[r, src], la_end[r, src - 1], closed(la_end[r, s2], tail),
                        closed(bl_end[r, src - 1], tail)])
    return -torch.logsumexp(ends, 0)


def forward_sum_opt_brute(logp, N, M, optional):
    """``nll`` of one utterance: -logsumexp over the kept subsets of ``F.ctc_loss`` on the
    pre-normalised frame scores.  torch fp64, differentiable in ``logp`` (a torch tensor)."""
    y = frame_scores(logp[None, :M, :N], [N])[0]     # (M, N + 1)
    terms = []
    for kept in valid_subsets(np.asarray(optional)[:N]):
        if len(kept) > M:
            continue
        target = torch.tensor([[s + 1 for s in kept]])
        terms.append(-F.ctc_loss(y[:, None, :], target, torch.tensor([M]),
                                 torch.tensor([len(kept)]), blank=0, reduction="none",
                                 zero_infinity=False)[0])
    if not terms:
        return torch.tensor(np.inf, dtype=torch.float64)
    return -torch.logsumexp(torch.stack(terms), 0)


# ------------------------------------------------------------------ monotonic alignment search
def mas_opt(logp, N, M, optional):
    """Durations (N) int64, fp32, one add per cell.  V[0, 0] = logp[0, 0]; V[0, 1] = logp[0, 1]
    when optional[0] and N >= 2.  The diagonal wins a tie against staying; the skip over a marked
    s - 1 is taken only when strictly greater than that winner; the path ends at N - 2 only when
    optional[N-1] and V[M-1, N-2] is strictly greater.  No path: all zeros."""
    x = np.asarray(logp, np.float32)[:M, :N]
    opt = np.asarray(optional)[:N].astype(bool)
    ninf = np.float32(-np.inf)
    V = np.full((M, N), ninf, np.float32)
    step = np.zeros((M, N), np.int64)
    V[0, 0] = x[0, 0]
    if N >= 2 and opt[0]:
        V[0, 1] = x[0, 1]
    can_skip = np.zeros(N, bool)
    can_skip[2:] = opt[1:N - 1]
    for t in range(1, M):
        up = V[t - 1]
        dg = np.concatenate([[ninf], up[:-1]]).astype(np.float32)
        sk = np.concatenate([[ninf, ninf], up[:-2]]).astype(np.float32)[:N]
        diag = dg >= up
        best = np.where(diag, dg, up)
        skip = can_skip & (sk > best)
        best = np.where(skip, sk, best).astype(np.float32)
        step[t] = np.where(skip, 2, np.where(diag, 1, 0))
        V[t] = x[t] + best  # one IEEE fp32 add per cell
    dur = np.zeros(N, np.int64)
    s = N - 1
    if N >= 2 and opt[N - 1] and V[M - 1, N - 2] > V[M - 1, N - 1]:
        s = N - 2
    if V[M - 1, s] == ninf:
        return dur
    for t in range(M - 1, -1, -1):
        dur[s] += 1
        if t > 0:
            s -= int(step[t, s])
    assert s == 0 or (s == 1 and opt[0])
    return dur


def mas_opt_brute(logp, N, M, optional):
    """``(best score, durations)`` over every kept subset and every split of the M frames into
    runs of >= 1 frame, the score summed in fp64 (exact for small integers); ``(-inf, zeros)``
    without a path.  Among equal scores the path the tie rules reach: walking back from the last
    frame, the end N - 1 before N - 2, then at each step the diagonal before staying before the
    skip."""
    x = np.asarray(logp, np.float64)[:M, :N]
    best = None
    for kept in valid_subsets(np.asarray(optional)[:N]):
        n = len(kept)
        if n > M:
            continue
        for cuts in itertools.combinations(range(1, M), n - 1):
            runs = np.diff((0,) + cuts + (M,))
            path = np.repeat(np.asarray(kept), runs)
            score = float(x[np.arange(M), path].sum())
            back = path[::-1]
            rank = {1: 0, 0: 1, 2: 2}
            code = (int(N - 1 - back[0]),) + tuple(rank[int(d)] for d in back[:-1] - back[1:])
            key = (-score, code)
            if best is None or key < best[0]:
                dur = np.zeros(N, np.int64)
                dur[list(kept)] = runs
                best = (key, score, dur)
    if best is None:
        return -np.inf, np.zeros(N, np.int64)
    return best[1], best[2]


# ------------------------------------------------------------------ .phn lines with '|'
# line -> (phones, optional) under parse_phn(optional_sil="sp", edges=True), and with edges=False
PARSE = [
    ("a k | o i", (["sp", "a", "k", "sp", "o", "i", "sp"], [1, 0, 0, 1, 0, 0, 1]),
     (["a", "k", "sp", "o", "i"], [0, 0, 1, 0, 0])),
    ("{a | | k ||| o}", None, None),  # '|||' is not a token: an unknown symbol
    ("a | | k | o", (["sp", "a", "sp", "k", "sp", "o", "sp"], [1, 0, 1, 0, 1, 0, 1]),
     (["a", "sp", "k", "sp", "o"], [0, 1, 0, 1, 0])),
    ("a | sp k sp | o", (["sp", "a", "sp", "k", "sp", "o", "sp"], [1, 0, 0, 0, 0, 0, 1]),
     (["a", "sp", "k", "sp", "o"], [0, 0, 0, 0, 0])),
    ("sp a k | o sp", (["sp", "a", "k", "sp", "o", "sp"], [0, 0, 0, 1, 0, 0]),
     (["sp", "a", "k", "sp", "o", "sp"], [0, 0, 0, 1, 0, 0])),
    ("| a k |", (["sp", "a", "k", "sp"], [1, 0, 0, 1]), (["sp", "a", "k", "sp"], [1, 0, 0, 1])),
    ("| sp | a", (["sp", "a", "sp"], [0, 0, 1]), (["sp", "a"], [0, 0])),
    ("a", (["sp", "a", "sp"], [1, 0, 1]), (["a"], [0])),
    ("|", None, None),  # no phoneme at all
    ("| |", None, None),
]


# ------------------------------------------------------------------ the synthetic corpus
N_SYMBOLS, N_UTT, N_MELS = O.N_SYMBOLS, O.N_UTT, O.N_MELS
SP = N_SYMBOLS + 1           # the pause symbol's id; the table has N_SYMBOLS + 2 rows
T_S = 4 * 4 + 5
# The prior is off.  It is a pmf over the N positions, so it takes log N or more from every label
# and nothing from the blank (score -1): with it the blank explains a silent frame better than an
# optional label can, no path through a pause is ever reinforced, and the trained model omits
# nearly every optional position (measured: tests/test_align_sil_cpu.py).
TEMPERATURE, OMEGA, STEPS, SEED = O.TEMPERATURE, 0.0, 100, 1


def synth_corpus_sil(seed, pause=(2, 9), edge=(0, 7), explicit=0.3):
    """``align_oracle.synth_corpus`` in words: utterances of 2-4 words of 2-4 phonemes (ids
    1..12, no symbol twice in a row, 1-9 frames each); ``sp`` (id 13) has a template of its own.
    An optional ``sp`` position stands at the start, at every word boundary and at the end: a
    boundary holds a pause of 2-8 frames with probability 0.5, an edge 0-6 frames of silence (0:
    none).  A pause or edge silence that is there is written out in the transcription with
    probability ``explicit``: its position is then not optional.  Without any such position the
    torch model learned the pauses on some seeds and on others settled on giving every silent
    frame to the blank and omitting every optional position (pause accuracy 0.29-0.92 over seeds
    0-4); with 0.3 it learns them on all five.  mel = template + 0.3 noise.  Padded arrays as ``synth_corpus``, ``durations`` over all
    positions (0 at an omitted one), plus ``optional`` (U, T_s) uint8."""
    rng = np.random.default_rng(seed)
    templates = rng.standard_normal((N_SYMBOLS + 2, N_MELS)).astype(np.float32)
    utts = []
    for _ in range(N_UTT):
        ids, dur, opt, last = [], [], [], 0
        words = int(rng.integers(2, 5))
        for w in range(words):
            ids.append(SP), opt.append(1)
            if w == 0:
                dur.append(int(rng.integers(*edge)))
            else:
                dur.append(int(rng.integers(*pause)) if rng.random() < 0.5 else 0)
            if dur[-1] > 0 and rng.random() < explicit:
                opt[-1] = 0
            for _ in range(int(rng.integers(2, 5))):
                c = int(rng.integers(1, N_SYMBOLS + 1))
                while c == last:
                    c = int(rng.integers(1, N_SYMBOLS + 1))
                last = c
                ids.append(c), opt.append(0), dur.append(int(rng.integers(1, 10)))
        ids.append(SP), opt.append(1), dur.append(int(rng.integers(*edge)))
        dur = np.asarray(dur, np.int64)
        mel = templates[np.repeat(ids, dur)] + \
            0.3 * rng.standard_normal((int(dur.sum()), N_MELS)).astype(np.float32)
        utts.append((np.asarray(ids, np.int64), dur, np.asarray(opt, np.uint8),
                     mel.astype(np.float32)))
    T_m = max(len(u[3]) for u in utts)
    texts = np.zeros((N_UTT, T_S), np.int64)
    durations = np.zeros((N_UTT, T_S), np.int64)
    optional = np.zeros((N_UTT, T_S), np.uint8)
    mels = np.zeros((N_UTT, T_m, N_MELS), np.float32)
    for u, (ids, dur, opt, mel) in enumerate(utts):
        n = len(ids)
        texts[u, :n], durations[u, :n], optional[u, :n], mels[u, :len(mel)] = ids, dur, opt, mel
    return {"texts": texts, "src_lens": np.asarray([len(u[0]) for u in utts], np.int64),
            "mels": mels, "mel_lens": np.asarray([len(u[3]) for u in utts], np.int64),
            "durations": durations, "optional": optional}


def without_pauses(corpus):
    """The corpus with the optional positions taken out of the texts (what a transcription
    without pause marks gives), and ``kept`` (U, T_s): each remaining position's index in the full
    sequence, so that paths can be compared on the full positions."""
    U = len(corpus["src_lens"])
    texts, kept = np.zeros_like(corpus["texts"]), np.zeros_like(corpus["texts"])
    lens = np.zeros(U, np.int64)
    for u in range(U):
        n = int(corpus["src_lens"][u])
        keep = np.flatnonzero(corpus["optional"][u, :n] == 0)
        lens[u] = len(keep)
        texts[u, :len(keep)], kept[u, :len(keep)] = corpus["texts"][u, keep], keep
    return dict(corpus, texts=texts, src_lens=lens, optional=np.zeros_like(corpus["optional"])), kept


def take(corpus, idx):
    """One batch cropped to its longest member: (texts, src_lens, mels, mel_lens, optional)."""
    sl, ml = corpus["src_lens"][idx], corpus["mel_lens"][idx]
    return (torch.from_numpy(corpus["texts"][idx][:, :sl.max()]), torch.from_numpy(sl),
            torch.from_numpy(corpus["mels"][idx][:, :ml.max()]), torch.from_numpy(ml),
            torch.from_numpy(corpus["optional"][idx][:, :sl.max()]))


def new_model(seed):
    torch.manual_seed(seed)
    return O.TorchAligner(N_SYMBOLS + 2, N_MELS, O.CHANNELS, O.ATTN_DIM)


def loss(model, texts, src_lens, mels, mel_lens, optional, temperature=TEMPERATURE,
         omega=OMEGA):
    """(1 / B) sum_b nll_b / M_b with the mask."""
    lp = model.logprob(texts, src_lens, mels, mel_lens, temperature, omega)
    nll = forward_sum_opt_torch(lp, src_lens, mel_lens, optional, lp.dtype)
    return (nll / torch.as_tensor(mel_lens, dtype=lp.dtype)).mean()


def align(model, texts, src_lens, mels, mel_lens, optional, omega=OMEGA):
    with torch.no_grad():
        lp = model.logprob(texts, src_lens, mels, mel_lens, TEMPERATURE, omega).float().numpy()
    return [mas_opt(lp[b], int(src_lens[b]), int(mel_lens[b]), np.asarray(optional[b]))
            for b in range(len(texts))]


def train(model, corpus, seed, steps=STEPS, omega=OMEGA):
    opt = torch.optim.Adam(model.parameters(), lr=O.LR)
    for idx in O.batch_order(seed, steps):
        opt.zero_grad()
        loss(model, *take(corpus, idx), omega=omega).backward()
        opt.step()
    return model


def agreement(durations, corpus, kept=None):
    """Fraction of frames whose position on the given paths is the true one.  ``kept``: the paths
    run over a reduced sequence whose position p is the full sequence's ``kept[u, p]``."""
    hit = total = 0
    for u in range(len(corpus["src_lens"])):
        n = int(corpus["src_lens"][u])
        want = O.path_of(corpus["durations"][u, :n])
        d = np.asarray(durations[u])
        got = O.path_of(d[:n]) if kept is None else kept[u][O.path_of(d)]
        hit += int((got == want).sum())
        total += len(want)
    return hit / total


def pause_accuracy(durations, corpus):
    """The share of optional positions whose kept / omitted decision is the true one."""
    hit = total = 0
    for u in range(len(corpus["src_lens"])):
        n = int(corpus["src_lens"][u])
        o = corpus["optional"][u, :n] != 0
        got, want = np.asarray(durations[u])[:n] > 0, corpus["durations"][u, :n] > 0
        hit += int((got == want)[o].sum())
        total += int(o.sum())
    return hit / total


def oracle_run(seed, steps=STEPS, omega=OMEGA, unmasked=True):
    """The torch model on ``synth_corpus_sil(seed)``: ``untrained`` / ``trained`` agreement and
    ``pause`` accuracy with the mask, and ``unmasked``: the agreement of the same model trained and
    aligned on the texts without the pause positions.  Also the trained model's initial state."""
    corpus = synth_corpus_sil(seed)
    model = new_model(seed)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    everything = take(corpus, np.arange(N_UTT))
    dur = align(model, *everything, omega=omega)
    out = {"init": init, "untrained": agreement(dur, corpus),
           "untrained_pause": pause_accuracy(dur, corpus)}
    train(model, corpus, seed, steps, omega)
    dur = align(model, *everything, omega=omega)
    out["trained"], out["pause"] = agreement(dur, corpus), pause_accuracy(dur, corpus)
    if not unmasked:
        return out
    bare, kept = without_pauses(corpus)
    plain = new_model(seed)
    opt = torch.optim.Adam(plain.parameters(), lr=O.LR)
    for idx in O.batch_order(seed, steps):
        opt.zero_grad()
        plain.loss(*O.take(bare, idx), TEMPERATURE, omega).backward()
        opt.step()
    dur = plain.align(*O.take(bare, np.arange(N_UTT)), TEMPERATURE, omega)
    out["unmasked"] = agreement(dur, corpus, kept)
    return out


if __name__ == "__main__":  # the measurements recorded in the tests and in DESIGN.md
    import sys
    for seed in range(5):
        r = oracle_run(seed, *(float(a) if "." in a else int(a) for a in sys.argv[1:]))
        print(seed, {k: round(v, 3) for k, v in r.items() if k != "init"}, flush=True)
