"""Maps of speaker embeddings: ``visualize_embeddings`` of
``Multilingual-Speaker-Encoder-with-Domain-Adaptation/train_speech_embedder.py`` (311-385) on the
device.  The per-speaker mean embeddings are mapped to the plane by exact t-SNE with a PCA
initialisation -- scikit-learn's ``TSNE(2, perplexity=50, init='pca', method='exact')`` -- and
coloured by language: the check that the domain adaptation mixes the languages, and for the
mid-attribute side the picture of where generated and interpolated speakers fall.

``TSNE`` runs on ``csrc/tsne.hip``: the perplexity search and the joint probabilities, then the
descent as two plain launches per iteration (row sums, then gradient + gains + update) and one
small control launch per check.  The stopping rules of ``_gradient_descent`` and the two stages of
``TSNE._tsne`` live in a device record, so all the iterations are queued without a
synchronisation and the record is read once at the end; iterations after the descent has ended
return at once.  Nothing is captured into a graph.

Left out: Barnes-Hut, ``n_components != 2``, other metrics, scikit-learn's random
initialisation and the PCA plot.  The final coordinates are not those of scikit-learn (its PCA
is a randomised SVD and the descent is chaotic); the objective is comparable.
"""
import random
import time

import numpy as np
import torch

from . import kernels as K
from .embedder_data import decode_filename

MARKERS, COLORS = "ox^*", "rbyg"  # visualize_embeddings:371-372


class TSNE:
    """Exact t-SNE to 2 components, Euclidean metric.  ``fit_transform`` sets
    ``embedding_`` (N, 2) on the device, ``kl_divergence_`` and ``n_iter_`` as scikit-learn
    reports them (the last evaluated error; the last iteration's index, 999 for a full run),
    and ``stage2_start_``, the first iteration without early exaggeration."""

    def __init__(self, perplexity=50.0, early_exaggeration=12.0, learning_rate="auto",
                 max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7,
                 exploration_iter=250, device="cuda"):
        self.perplexity = float(perplexity)
        self.early_exaggeration = float(early_exaggeration)
        self.learning_rate = learning_rate
        self.max_iter = int(max_iter)
        self.n_iter_without_progress = int(n_iter_without_progress)
        self.min_grad_norm = float(min_grad_norm)
        self.exploration_iter = int(exploration_iter)
        self.device = torch.device(device)
        if self.exploration_iter < 1 or self.max_iter < 1:
            raise ValueError(f"max_iter = {self.max_iter} and exploration_iter = "
                             f"{self.exploration_iter} must be at least 1")
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = None

    def _x(self, X):
        X = torch.as_tensor(X, dtype=torch.float32, device=self.device).contiguous()
        if X.dim() != 2:
            raise ValueError(f"X is (N, D), got {tuple(X.shape)}")
        if self.perplexity >= X.shape[0]:
            raise ValueError(f"perplexity = {self.perplexity} must be less than the number of "
                             f"points = {X.shape[0]}")
        return X

    def lr(self, n):
        if self.learning_rate == "auto":
            return max(n / self.early_exaggeration / 4.0, 50.0)
        return float(self.learning_rate)

    def pca_init(self, X):
        """Y0 (N, 2): the two leading principal components, the first with std 1e-4."""
        return K.tsne_pca_init(self._x(X))

    def affinities(self, X, want64=False):
        """The joint probabilities P (N, N); with ``want64`` (P, beta (N) f64, P (N, N) f64)."""
        return K.tsne_affinities(self._x(X), self.perplexity, want64=want64)

    def kl(self, Y, P, exaggeration=1.0):
        """The objective of Y under ``exaggeration * P`` (a float; one host read)."""
        return K.tsne_kl(P, Y.contiguous(), exaggeration).item()

    def step(self, Y, update, gains, P, exaggeration, momentum, learning_rate=None):
        """One iteration on explicit state: returns ``(Y', kl, grad_norm)`` with kl (the
        objective of Y) and ||gains * grad|| as 0-dim f64 device tensors; ``update`` and
        ``gains`` are advanced in place."""
        lr = self.lr(Y.shape[0]) if learning_rate is None else learning_rate
        Y1, kl_rows, gn_rows = K.tsne_step(P, Y, update, gains, exaggeration, momentum, lr)
        return Y1, kl_rows.sum(), gn_rows.sum().sqrt()

    def fit_transform(self, X, init=None):
        """X (N, D) -> Y (N, 2) on the device.  ``init``: an (N, 2) start instead of the PCA."""
        X = self._x(X)
        n = X.shape[0]
        dev = X.device
        P = K.tsne_affinities(X, self.perplexity)
        if init is None:
            Y = K.tsne_pca_init(X)
        else:
            Y = torch.as_tensor(init, dtype=torch.float32, device=dev).clone().contiguous()
            if tuple(Y.shape) != (n, 2):
                raise ValueError(f"init is ({n}, 2), got {tuple(Y.shape)}")
        state = K.tsne_state(n, self.perplexity, self.max_iter, self.exploration_iter,
                             self.n_iter_without_progress, self.early_exaggeration, self.lr(n),
                             self.min_grad_norm, dev)
        buf = (Y, torch.empty_like(Y))  # iteration i reads buf[i & 1] and writes the other
        update, gains = K.zeros((n, 2), dev), K.fill_(torch.empty_like(Y), 1.0)
        rowsum, kl_rows, gn_rows = (K.empty_f64(n, dev) for _ in range(3))
        t0 = time.perf_counter()
        # stage 1 may run to exploration_iter whatever max_iter is, as scikit-learn's does
        for i in range(max(self.max_iter, self.exploration_iter)):
            K.tsne_rowsum(buf[i & 1], state, rowsum)
            K.tsne_update(P, buf[i & 1], buf[~i & 1], update, gains, i, state, rowsum, kl_rows,
                          gn_rows)
            if (i + 1) % 50 == 0 or i in (self.exploration_iter - 1, self.max_iter - 1):
                K.tsne_control(state, n, i, kl_rows, gn_rows)
        self.queue_seconds_ = time.perf_counter() - t0  # host time to queue the descent
        record = state.tolist()  # the one host read
        self.n_iter_ = int(record[5])
        self.stage2_start_ = int(record[7])  # the iteration after stage 1's last one
        self.kl_divergence_ = record[6]
        self.embedding_ = buf[(self.n_iter_ + 1) & 1]
        return self.embedding_


def select_speakers(names, da_on="language", spkr_per_lang=300, rng=random):
    """Lines 336-355: group the file names by ``decode_filename(name)[da_on]`` in order of first
    appearance, ``rng.sample`` at most ``spkr_per_lang`` of each group in that order, codes from
    the sorted label set.  Returns (indices into ``names``, their labels, ``lang2code``)."""
    groups = {}
    for k, name in enumerate(names):
        groups.setdefault(decode_filename(name)[da_on], []).append(k)
    indices, labels = [], []
    for label, members in groups.items():
        picked = rng.sample(members, min(spkr_per_lang, len(members)))
        indices.extend(picked)
        labels.extend([label] * len(picked))
    lang2code = {label: code for code, label in enumerate(sorted(set(labels)))}
    return indices, labels, lang2code


def _fit(X, tsne):
    t = TSNE(device=X.device, **tsne)
    Y = t.fit_transform(X)
    return K.tsne_finish(Y), t


def map_embeddings(X, labels=None, **tsne):
    """The map of any (N, D) device tensor (FS2 speaker embeddings, GMM samples, interpolated
    speakers): ``{coords (N, 2) in [0, 1], codes, lang2code, kl, n_iter}``; ``labels`` (N
    hashables, optional) give the codes, from the sorted label set."""
    coords, t = _fit(X, tsne)
    labels = [0] * X.shape[0] if labels is None else list(labels)
    if len(labels) != X.shape[0]:
        raise ValueError(f"{len(labels)} labels for {X.shape[0]} points")
    lang2code = {label: code for code, label in enumerate(sorted(set(labels)))}
    return {"coords": coords, "codes": [lang2code[l] for l in labels], "lang2code": lang2code,
            "kl": t.kl_divergence_, "n_iter": t.n_iter_}


def speaker_map(spkr2embedding, da_on="language", emb_per_spkr=400, spkr_per_lang=300, rng=random,
                **tsne):
    """visualize_embeddings up to the figure: ``spkr2embedding`` is ``{file name: (count, D)
    embeddings}`` on the device (``EmbedderTrainer.spkr2embedding``).  Each selected speaker's
    point is the mean of its first ``emb_per_spkr`` embeddings.  Returns ``{names, coords (n, 2)
    in [0, 1], codes, lang2code, kl, n_iter}``."""
    names = list(spkr2embedding)
    indices, labels, lang2code = select_speakers(names, da_on, spkr_per_lang, rng)
    rows = [spkr2embedding[names[k]] for k in indices]
    seg_start = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int64)
    embs = torch.cat([r.detach().float() for r in rows]).contiguous()
    seg = torch.from_numpy(seg_start).to(embs.device)
    coords, t = _fit(K.tsne_points(embs, seg, emb_per_spkr), tsne)
    return {"names": [names[k] for k in indices], "coords": coords,
            "codes": [lang2code[l] for l in labels], "lang2code": lang2code,
            "kl": t.kl_divergence_, "n_iter": t.n_iter_}


def plot_speaker_map(m, path):
    """The scatter of lines 368-384: one marker and colour per code, legend; written to
    ``path``."""
    from matplotlib.figure import Figure
    coords = m["coords"].detach().cpu().numpy()
    codes = np.asarray(m["codes"])
    if len(m["lang2code"]) > len(MARKERS):
        raise ValueError(f"{len(m['lang2code'])} groups, markers and colours for {len(MARKERS)}")
    fig = Figure(figsize=(9.84, 7.47))
    ax = fig.add_subplot()
    ax.tick_params(labelsize=28)
    handles = []
    for label, code in m["lang2code"].items():
        sel = codes == code
        ax.scatter(coords[sel, 0], coords[sel, 1], marker=MARKERS[code], s=32,
                   color=COLORS[code], alpha=0.6)
        handles.append(ax.plot([], [], marker=MARKERS[code], ls="", mec=None, color=COLORS[code],
                               label=label, alpha=0.6, ms=18)[0])
    ax.legend(handles=handles, loc="upper right", bbox_to_anchor=(1, 1), prop={"size": 18})
    fig.savefig(path)
    return path
