"""Training the speaker encoder: the loop body of
``Multilingual-Speaker-Encoder-with-Domain-Adaptation/train_speech_embedder.py`` (optimisers
104-113, batch step 154-192, classifier subroutine 249-277) over flat parameter buffers.

``EmbedderTrainer`` holds a ``SpeechEmbedder(weight_grads=True)``, a ``GE2ELoss`` and the
reference's three ``torch.optim.Adam`` optimisers as ``fs2_adam_l2_step`` over one arena each:

  main   LSTM stack + projection   lr 1e-3, weight_decay 1e-6, clipped at 3.0
  ge2e   GE2ELoss.w, .b            lr 1e-3,                    clipped at 1.0
  da     the domain classifier     lr 1e-3, weight_decay 1e-6, clipped at 3.0

``train_step`` makes no host synchronisation: the reference's host-side test
``da_loss < -log(1/2) N M or progress <= da_startpoint`` becomes a device gate that scales the
classifier loss's upstream gradient and switches the optimiser steps it guards, so a step is a
fixed launch sequence.  Where the reference skips ``da_loss.backward()`` its parameters have no
gradient: ``clip_grad_norm_`` then returns 0 and Adam leaves parameters, moments and step count
alone; the gate reproduces exactly that.

``ge2e_backward=False`` is the reference as shipped: its ``loss.backward`` is commented out at
line 181 (the model is named ``...woGE2E``), so only the domain loss trains the encoder and
``w``, ``b`` never move.  ``True`` is that line live.

Not ported: the per-batch random shuffle / unshuffle of lines 160-172 -- the embedder treats
the rows independently, so it only changes the order in which the gradient sums run; the
dataset and mel extraction (librosa), the ``rescnn`` architecture, the EER ``test()``, the
t-SNE plots, DDP of the embedder, and the joint ``train_ganlike.py`` loop.
"""
import math

import torch

from . import kernels as K
from .ge2e import GE2ELoss, SpeechEmbedder, _BCESumFn
from .model import ParamArena

ANNEAL_EPOCHS = (800, 1400, 1800, 2200)  # config/config.yaml train.anneal_epochs
BETAS, EPS = (0.9, 0.999), 1e-8          # torch.optim.Adam defaults


class _Adam:
    """One ``torch.optim.Adam(params, lr, weight_decay)`` over a ``ParamArena``."""

    def __init__(self, params, lr, weight_decay, device):
        self.arena = ParamArena(params, device)
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        n = self.arena.numel
        self.m = torch.zeros(n, dtype=torch.float32, device=device)
        self.v = torch.zeros(n, dtype=torch.float32, device=device)
        self.step_count = torch.zeros(1, dtype=torch.int64, device=device)
        self._hyper = torch.zeros(3, dtype=torch.float32, device=device)
        self.norm_coef = None

    def zero_grad(self):
        self.arena.zero_grad()
        self.norm_coef = None

    def clip_grad_norm_(self, max_norm):
        """The pre-clip norm (0-dim device tensor); the clip itself is applied by ``step``."""
        self.norm_coef = torch.empty(2, dtype=torch.float32, device=self.arena.grad.device)
        K.grad_norm(self.arena.grad, float(max_norm), self.norm_coef)
        return self.norm_coef[0]

    def step(self, gate=None):
        K.adam_l2_step(self.arena.flat, self.arena.grad, self.m, self.v, self.norm_coef, self.lr,
                       BETAS[0], BETAS[1], EPS, self.weight_decay, self.step_count, self._hyper,
                       gate)
        self.norm_coef = None


class EmbedderTrainer:
    def __init__(self, embedder=None, criterion=None, device="cuda", n_utt=10, lr=1e-3,
                 weight_decay=1e-6, da_startpoint=0.0):
        """n_utt: utterances per speaker in a batch (hp.train.M)."""
        self.device = torch.device(device)
        self.n_utt = int(n_utt)
        self.embedder = embedder if embedder is not None else SpeechEmbedder(device, True)
        self.embedder.weight_grads = True
        self.criterion = criterion if criterion is not None else GE2ELoss(device)
        self.da_startpoint = float(da_startpoint)
        e = self.embedder
        self.optimizers = {
            "main": _Adam(e.main_parameters(), lr, weight_decay, self.device),
            "ge2e": _Adam(list(self.criterion.parameters()), lr, 0.0, self.device),
            "da": _Adam(e.da_parameters(), 1e-3, weight_decay, self.device)}
        e._key = None  # the parameters moved into the arenas
        self._zero = torch.zeros((), dtype=torch.float32, device=self.device)

    def _weights_changed(self):
        self.embedder._key = None  # kernel-layout copies are rebuilt at the next forward

    def train_step(self, mels, langs, progress, ge2e_backward=False):
        """One batch of train_speech_embedder.py:167-191.  mels (N * n_utt, T, 80), speaker-major;
        langs (N * n_utt) in {0, 1}.  Returns (loss, da_loss, norm_main, norm_ge2e, norm_da) as
        0-dim device tensors; a norm the reference does not compute is 0."""
        opt, n_utt = self.optimizers, self.n_utt
        rows = mels.shape[0]
        if rows % n_utt:
            raise ValueError(f"{rows} rows are not a multiple of n_utt = {n_utt}")
        for o in opt.values():
            o.zero_grad()
        out = self.embedder(mels)
        emb = out["embeddings"].view(rows // n_utt, n_utt, -1)
        _, loss, da_loss = self.criterion(emb, out["da_lang_logits"], langs)
        gate = None  # None: da_pretrain, the domain loss always trains
        if progress > self.da_startpoint:
            gate = K.gate_lt(da_loss.detach(), -math.log(1 / 2) * rows)
        if ge2e_backward:
            loss.backward(retain_graph=True)
        da_loss.backward(gradient=gate)  # d da_loss = gate (None = 1)
        n_main = opt["main"].clip_grad_norm_(3.0)
        n_ge2e = opt["ge2e"].clip_grad_norm_(1.0) if ge2e_backward else self._zero
        # without loss.backward the encoder's only gradient is the gated domain loss's
        opt["main"].step(gate=None if ge2e_backward else gate)
        if ge2e_backward:
            opt["ge2e"].step()
        n_da = opt["da"].clip_grad_norm_(3.0)  # 0 when the gate is shut: no gradient arrived
        opt["da"].step(gate=gate)
        self._weights_changed()
        return loss.detach(), da_loss.detach(), n_main, n_ge2e, n_da

    def da_classifier_step(self, mels, langs):
        """One batch of da_classifier_subroutine (249-277): the classifier alone, on a detached
        embedding.  Same 5-tuple as ``train_step`` with 0 where that loop has no such scalar."""
        opt = self.optimizers["da"]
        opt.zero_grad()
        out = self.embedder(mels, detach=True)
        da_loss = _BCESumFn.apply(out["da_lang_logits"].contiguous(), langs.contiguous().float())
        da_loss.backward()
        n_da = opt.clip_grad_norm_(3.0)
        opt.step()
        self._weights_changed()
        return self._zero, da_loss.detach(), self._zero, self._zero, n_da

    def anneal(self, epoch):
        """lr_schedule (83-95): halve the lr of ``main`` and ``ge2e`` at the anneal epochs."""
        if epoch in ANNEAL_EPOCHS:
            for k in ("main", "ge2e"):
                self.optimizers[k].lr /= 2

    def state_dict(self):
        """The reference's checkpoint form (train_speech_embedder.py:221)."""
        return {"embedder_net": {k: v.detach().clone() for k, v in
                                 self.embedder.state_dict().items()},
                "ge2e": {k: v.detach().clone() for k, v in self.criterion.state_dict().items()}}

    def load_state_dict(self, sd):
        self.embedder.load_state_dict(sd["embedder_net"])
        self.criterion.load_state_dict(sd["ge2e"])
        self._weights_changed()
