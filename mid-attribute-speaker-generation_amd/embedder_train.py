"""Training the speaker encoder: the loop body of
``Multilingual-Speaker-Encoder-with-Domain-Adaptation/train_speech_embedder.py`` (optimisers
104-113, batch step 154-192, classifier subroutine 249-277) over flat parameter buffers.

``EmbedderTrainer`` holds a ``SpeechEmbedder(weight_grads=True)``, a ``GE2ELoss`` and the
reference's three ``torch.optim.Adam`` optimisers as ``fs2_adam_l2_step`` over one arena each:

  main   encoder + projection      lr 1e-3, weight_decay 1e-6, clipped at 3.0
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

Around the step (``embedder_data.SpeakerBatcher`` supplies the batches, cut on the device):
``train_epoch`` is the epoch loop of lines 146-216 with the loss, da_loss and da accuracy sums
kept on the device and read once per epoch, ``da_subroutine`` lines 249-287 (one read per pass),
``evaluate_eer`` the EER ``test()`` of 401-455 scored by ``fs2_ge2e_eer``, ``dvector`` the
d-vector of 49-54 and 75-78 from a mel spectrogram, ``dvector_from_wav`` the same from a
waveform through the mel front end (``audio.py``), ``spkr2embedding`` lines 289-309,
``visualize_embeddings`` the t-SNE map of 311-385 (``embedding_map.py``).

Not ported: the per-batch random shuffle / unshuffle of lines 160-172 is drawn by the batcher
(to keep Python's generator in step with the reference) but not applied -- the embedder treats
the rows independently, so it only changes the order in which the gradient sums run; the
silence split of ``process_dvector_wav`` (``librosa.effects.split``), DDP of the embedder, and
the joint ``train_ganlike.py`` loop.

``EmbedderTrainer(loss='contrast')`` trains with the reference's other ``hp.model.loss``
(``utils.get_contrast_loss``, ``fs2_ge2e_contrast``); ``'softmax'`` is the default.

Either architecture of the encoder trains here: pass
``SpeechEmbedder(device, True, architecture='rescnn')`` as ``embedder`` for the residual CNN;
the "main" arena then holds its 48 convolution and BatchNorm parameters and the projection.
"""
import contextlib
import math

import numpy as np
import torch

from . import kernels as K
from .ge2e import NMELS, GE2ELoss, SpeechEmbedder, _BCESumFn
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
                 weight_decay=1e-6, da_startpoint=0.0, loss="softmax"):
        """n_utt: utterances per speaker in a batch (hp.train.M); loss: hp.model.loss,
        ``'softmax'`` or ``'contrast'``, for the ``GE2ELoss`` made here (a ``criterion`` passed
        in keeps its own)."""
        self.device = torch.device(device)
        self.n_utt = int(n_utt)
        self.embedder = embedder if embedder is not None else SpeechEmbedder(device, True)
        self.embedder.weight_grads = True
        self.criterion = criterion if criterion is not None else GE2ELoss(device, loss=loss)
        self.loss = getattr(self.criterion, "loss", None)  # None: a criterion that names none
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
        self.last_logits = out["da_lang_logits"].detach()  # for the epoch's accuracy
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
        self.last_logits = out["da_lang_logits"].detach()
        da_loss = _BCESumFn.apply(out["da_lang_logits"].contiguous(), langs.contiguous().float())
        da_loss.backward()
        n_da = opt.clip_grad_norm_(3.0)
        opt.step()
        self._weights_changed()
        return self._zero, da_loss.detach(), self._zero, self._zero, n_da

    # -- epoch statistics: sums kept on the device, read once ---------------------------------
    def _stats_new(self):
        return K.zeros(4, self.device)

    def _stats_add(self, totals, loss, da_loss, langs):
        """totals += [loss, da_loss, accuracy (%) of the last step's logits, 1]."""
        K.epoch_stats_add(totals, loss, da_loss, self.last_logits, langs.contiguous().float())

    def _stats_read(self, totals):
        return totals.tolist()  # the host read

    def train_epoch(self, batcher, epoch, epochs, ge2e_backward=False):
        """One epoch of train_speech_embedder.py:146-216 over ``batcher``
        (``embedder_data.SpeakerBatcher``): a ``train_step`` per batch at ``progress = epoch /
        epochs``, the sums of loss, da_loss and da accuracy kept on the device and read once
        when the batches are queued, ``anneal(epoch)``, and past ``da_startpoint`` the
        classifier subroutine (its pass averages are left in ``last_da_passes``).  Returns the
        epoch's averages ``{"loss", "da_loss", "da_acc"}`` (accuracy in percent)."""
        progress = float(epoch) / epochs
        totals = self._stats_new()
        for _ in range(batcher.batches_per_epoch):
            mels, langs = batcher.next_batch()
            loss, da_loss = self.train_step(mels, langs, progress, ge2e_backward)[:2]
            self._stats_add(totals, loss, da_loss, langs)
        self.anneal(epoch)
        t = self._stats_read(totals)
        stats = {"loss": t[0] / t[3], "da_loss": t[1] / t[3], "da_acc": t[2] / t[3]}
        self.last_da_passes = None
        if progress > self.da_startpoint:
            self.last_da_passes = self.da_subroutine(batcher)
        return stats

    def da_subroutine(self, batcher, max_passes=10, floor=20.0):
        """da_classifier_subroutine (249-287): passes of ``da_classifier_step`` over an epoch's
        batches until a pass's average loss is below ``floor`` or above the previous pass's;
        one host read per pass.  Returns the pass averages."""
        prev, passes = float("inf"), []
        for _ in range(max_passes):
            totals = self._stats_new()
            for _ in range(batcher.batches_per_epoch):
                mels, langs = batcher.next_batch()
                da_loss = self.da_classifier_step(mels, langs)[1]
                self._stats_add(totals, None, da_loss, langs)
            t = self._stats_read(totals)
            avg = t[1] / t[3]
            passes.append(avg)
            if avg < floor or avg > prev:
                break
            prev = avg
        return passes

    @contextlib.contextmanager
    def _eval(self):
        """The embedder in eval mode without autograd; its mode is restored after."""
        was = self.embedder.training
        self.embedder.eval()
        try:
            with torch.no_grad():
                yield
        finally:
            self.embedder.train(was)

    def evaluate_eer(self, batches, epochs=1):
        """test() (401-455): the average EER over ``epochs`` passes.  ``batches`` is a
        ``SpeakerBatcher`` (an epoch of ``next_batch()`` per pass, M = its ``n_utt``) or a
        sequence of ``(N, M, T, 80)`` device tensors.  Each batch's first M / 2 utterances per
        speaker enrol, the rest verify (M even); both halves are embedded in eval mode and scored
        by ``fs2_ge2e_eer``; the EERs are averaged on the device and read once at the end.  The
        reference's permutation of the verification rows is undone before scoring and so leaves
        the result alone; it is not drawn here."""
        total = K.zeros(1, self.device)
        with self._eval():
            for _ in range(epochs):
                if hasattr(batches, "next_batch"):
                    it = (batches.next_batch()[0].view(batches.n_spk, batches.n_utt, -1, NMELS)
                          for _ in range(batches.batches_per_epoch))
                else:
                    it = iter(batches)
                acc, n = K.zeros(1, self.device), 0
                for mels in it:
                    N, M, T, C = mels.shape
                    if M % 2 or M < 4:
                        raise ValueError(f"M = {M}: enrolment and verification halves need an "
                                         "even M >= 4")
                    emb = self.embedder.compute_embedding(mels.contiguous().view(N * M, T, C))
                    emb = emb["embeddings"].view(N, M, -1)
                    enroll, verify = emb[:, :M // 2].contiguous(), emb[:, M // 2:].contiguous()
                    result = K.ge2e_eer(enroll, verify)[2]
                    K.add(acc, result[0:1], out=acc)
                    n += 1
                if n == 0:
                    raise ValueError("evaluate_eer: no batch")
                K.scale_(acc, 1.0 / n)
                K.add(total, acc, out=total)
        return total.item() / epochs

    def dvector(self, mel, seg=130):
        """generate_dvector (49-54, 75-78) from a mel spectrogram: ``mel`` (80, F) on the device
        gives the unit-length mean (64,) of the embeddings of its windows ``[s, s + seg)``,
        ``s = 0, seg // 2, ...`` while ``s + seg <= F``; a list of mels gives (len, 64) from one
        embedder call.  ``F < seg`` raises ``ValueError`` (the reference pads the waveform there:
        ``dvector_from_wav``)."""
        single = torch.is_tensor(mel)
        mels = [mel] if single else list(mel)
        off, stride, start, seg_start, base = [], [], [], [0], 0
        for m in mels:
            c, f = m.shape
            if f < seg:
                raise ValueError(f"{f} frames, fewer than one window of {seg}")
            for s in range(0, f - seg + 1, seg // 2):
                off.append(base)
                stride.append(f)
                start.append(s)
            seg_start.append(len(off))
            base += c * f
        n_mels = mels[0].shape[0]
        store = mels[0].contiguous().view(-1) if single else \
            torch.cat([m.contiguous().view(-1) for m in mels])
        dev = store.device

        def up(a, dt):
            return torch.from_numpy(np.asarray(a, dt)).pin_memory().to(dev, non_blocking=True)

        windows = K.mel_crop_gather(store.float(), up(off, np.int64), up(stride, np.int32),
                                    up(start, np.int32), n_mels, seg)
        with self._eval():
            emb = self.embedder.compute_embedding(windows)["embeddings"]
            out = K.rows_mean_unit(emb.contiguous(), up(seg_start, np.int64))
        return out[0] if single else out

    @staticmethod
    def _check_wav_lens(lens, rows, samples):
        if len(lens) != rows or any(not 1 <= n <= samples for n in lens):
            raise ValueError(f"lengths {lens} for {rows} waveforms of {samples} samples")

    def dvector_from_wav(self, wav, lens=None, seg=130):
        """generate_dvector (27-81) from a waveform on the device: the mel front end
        (``audio.MelFrontEnd``), then the window cut, embedder and unit-length mean of
        ``dvector``.  ``wav`` is (S,) -> (64,), (B, S) with ``lens`` -> (B, 64), or a list of 1-D
        waveforms -> (len, 64).  ``lens`` as a list costs no synchronisation; as a device tensor
        it is read once (the window descriptors are built on the host).

        A waveform shorter than ``seg * hop + 1024`` samples is zero-extended to that length
        first, which is what ``process_dvector_wav`` lines 29-47 intend.  As shipped, that
        function multiplies a hop that is already in samples by the sample rate, so its bound is
        7.6e8 samples and it zero-pads every input to that length.  ``librosa.effects.split(
        top_db=100)`` is not built: the whole utterance is one interval, which is what that call
        returns for any signal with no stretch 100 dB below its peak."""
        from .audio import MelFrontEnd, N_FFT
        if getattr(self, "_front_end", None) is None:
            self._front_end = MelFrontEnd(device=self.device)
        front_end = self._front_end
        hop, need = front_end.hop, seg * front_end.hop + N_FFT
        single = torch.is_tensor(wav) and wav.dim() == 1
        if torch.is_tensor(wav):
            w = wav[None] if single else wav
            if lens is None:
                lens = [w.shape[1]] * w.shape[0]
            elif torch.is_tensor(lens):
                lens = lens.tolist()
            lens = [int(n) for n in lens]
            self._check_wav_lens(lens, w.shape[0], w.shape[1])
            short = any(n < need for n in lens)
            if w.shape[1] < need:
                w = torch.nn.functional.pad(w.float(), (0, need - w.shape[1]))
            elif short:
                w = w.float().clone()
        else:
            rows = list(wav)
            lens = [int(r.numel()) for r in rows]
            self._check_wav_lens(lens, len(rows), max(lens))
            w = torch.zeros((len(rows), max(max(lens), need)), dtype=torch.float32,
                            device=rows[0].device)
            for b, r in enumerate(rows):
                w[b, :lens[b]] = r
            short = False  # the rows are zero past their lengths already
        if short:
            for b, n in enumerate(lens):
                if n < need:
                    w[b, n:need] = 0.0
        lens = [max(n, need) for n in lens]
        mel, _, _ = front_end(w, lens=lens)
        B, n_mels, f_max = mel.shape
        off, stride, start, seg_start = [], [], [], [0]
        for b, n in enumerate(lens):
            for s in range(0, 1 + n // hop - seg + 1, seg // 2):
                off.append(b * n_mels * f_max)
                stride.append(f_max)
                start.append(s)
            seg_start.append(len(off))
        dev = mel.device

        def up(a, dt):
            return torch.from_numpy(np.asarray(a, dt)).pin_memory().to(dev, non_blocking=True)

        windows = K.mel_crop_gather(mel.view(-1), up(off, np.int64), up(stride, np.int32),
                                    up(start, np.int32), n_mels, seg)
        with self._eval():
            emb = self.embedder.compute_embedding(windows)["embeddings"]
            out = K.rows_mean_unit(emb.contiguous(), up(seg_start, np.int64))
        return out[0] if single else out

    def spkr2embedding(self, batcher, utter_num=400):
        """get_spkr2embedding (289-309): ``{file name: (utter_num, 64) embeddings}`` of every
        file of the batcher's store, in eval mode."""
        out = {}
        with self._eval():
            for k, name in enumerate(batcher.store.files):
                mels, _ = batcher.speaker_batch(k, utter_num)
                out[name] = self.embedder.compute_embedding(mels)["embeddings"]
        return out

    def visualize_embeddings(self, source, path=None, **kw):
        """visualize_embeddings (311-385): the t-SNE map of the speakers' mean embeddings,
        coloured by language.  ``source`` is a batcher (``spkr2embedding`` runs on it) or a ready
        ``{file name: embeddings}`` dict; ``kw`` goes to ``embedding_map.speaker_map``.  Returns
        the map and, given ``path``, writes the figure there."""
        from . import embedding_map
        if not isinstance(source, dict):
            source = self.spkr2embedding(source)
        m = embedding_map.speaker_map(source, **kw)
        if path is not None:
            embedding_map.plot_speaker_map(m, path)
        return m

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
