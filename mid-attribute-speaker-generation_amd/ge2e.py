"""The ``--use_clf`` language discriminator on the HIP path.

Mirrors ``Multilingual-Speaker-Encoder-with-Domain-Adaptation/speech_embedder_net.py``:

* ``SpeechEmbedder()`` -- 3-layer ``nn.LSTM(80, 256, batch_first)`` (``LSTM_stack``), last
  frame, ``projection`` (LinearNorm 256 -> 64), L2 normalisation, and the domain classifier
  ``da_classifier.classifier`` (MultiLayerNN 64 -> [64, 64, 1], dropout 0.2, ReLU); same
  state-dict keys and shapes; ``forward(x)`` returns ``{'embeddings', 'da_lang_logits'}``
  (``speech_embedder_net.py:126-146``, config/config.yaml: hidden 256, 3 layers, proj 64,
  da on language).
* ``GE2ELoss(device)`` -- ``forward(embeddings, lang_logits, langs, **kw)`` returns
  ``(loss + da_loss, loss, da_loss)`` with ``da_loss = BCEWithLogitsLoss(reduction='sum')``
  (``speech_embedder_net.py:165-186``).  ``train.py:190`` only back-propagates ``da_loss``;
  the GE2E similarity term there has M = 1 utterance per "speaker", for which the
  reference's exclude-self centroid divides by M - 1 = 0 (``utils.py:36``) -- it is NaN and
  returned as NaN here as well.  For M > 1, the speaker-encoder training loss, the softmax
  GE2E loss is one kernel forward and one backward (``fs2_ge2e_softmax``), and so is the
  'contrast' variant (``GE2ELoss(loss='contrast')``, ``hp.model.loss``; ``fs2_ge2e_contrast``).
* ``SpeechEmbedder(architecture='rescnn')`` -- the reference's other feature extractor
  (``hp.model.architecture``, ``speech_embedder_net.py:19-63,79-81``): a 2-D residual CNN over
  the (mel, time) plane, 640 features, the same head behind a 640-wide projection
  (``rescnn.py``, ``csrc/rescnn.hip``).  Same interface, the reference's state-dict keys.

Kernels (``csrc/lstm.hip``): the 3-layer stack runs as a wavefront -- launch s computes
layer l at step s - l, all layers in one launch (T + 2 launches instead of 3T), with the
inputs of layers 1-2 folded into their step kernels; layer 0's input projection is one GEMM.
The backward is the same in reverse plus one GEMM for the input gradient.  The head (projection .. logit) is one kernel,
one wave per sequence, forward and backward.  ``train.py`` never steps the discriminator (its
parameters are set ``requires_grad`` but no optimiser holds them), so by default only the
gradient into FastSpeech2's mel output is computed.  ``SpeechEmbedder(weight_grads=True)``
also forms the discriminator's own weight gradients, for ``embedder_train.EmbedderTrainer``:
the LSTM's from the saved ``h`` and the backward's ``dgates`` in one split-row f32-MFMA GEMM
per layer (``csrc/lstm_wgrad.hip``), the head's in ``fs2_clf_head_wgrad``.
"""
import math

import torch
import torch.nn as nn

from . import kernels as K
from ._lib import lib

HIDDEN, LAYERS, PROJ, NMELS, CHUNK = 256, 3, 64, 80, 150  # config/config.yaml
DA_DROPOUT = 0.2  # module.py:24 via speech_embedder_net.py:152


def _p(t):
    return t.data_ptr()


class _EmbedderFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, x, emb_mod, seed, detach, anchor):
        N, T, D = x.shape
        dev = x.device
        w = emb_mod._prep()
        st, rows = w["stack"], N * T
        gx = torch.empty(rows, 4 * HIDDEN, device=dev)
        h = torch.empty(LAYERS, rows, HIDDEN, device=dev)
        c = torch.empty(LAYERS, rows, HIDDEN, device=dev)
        act = torch.empty(LAYERS, rows, 4 * HIDDEN, device=dev)
        xc = x.contiguous()
        lib.fs2_lstm_stack_fwd(_p(xc), N, T, D, HIDDEN, LAYERS, _p(st["w_ih0"]),
                               _p(st["w_ih_up"]), _p(st["w_hh"]), _p(st["bias"]), _p(gx), _p(h),
                               _p(c), _p(act), K.stream())
        del gx
        saved, inp = (c, act), h[LAYERS - 1]
        emb = torch.empty(N, PROJ, device=dev)
        logit = torch.empty(N, device=dev)
        hd = w["head"]
        p = emb_mod.da_dropout if emb_mod.training else 0.0
        last = _p(inp) + (T - 1) * HIDDEN * 4  # h[n*T + T-1], row stride T*H
        lib.fs2_clf_head(last, T * HIDDEN, N, *hd, p, _p(seed) if p > 0 else None,
                         emb_mod.site, _p(emb), _p(logit), None, None, None, 0, K.stream())
        fctx.emb_mod, fctx.saved, fctx.h_top, fctx.seed = emb_mod, saved, inp, seed
        fctx.shape, fctx.p = (N, T, D), p
        # weight gradients (train_speech_embedder.py): the backward also needs x and every
        # layer's h; detach = the reference's detach=True (classifier gradients only)
        fctx.wgrad = (xc, h, detach) if emb_mod.weight_grads else None
        return emb, logit

    @staticmethod
    def backward(fctx, demb, dlogit):
        N, T, D = fctx.shape
        dev = fctx.h_top.device
        w = fctx.emb_mod._prep()
        last_in = _p(fctx.h_top) + (T - 1) * HIDDEN * 4
        demb = demb.contiguous() if demb is not None else None
        dlogit = dlogit.contiguous() if dlogit is not None else None
        if fctx.wgrad is not None:
            fctx.emb_mod._head_wgrad(last_in, T * HIDDEN, N, w, fctx.p, fctx.seed, demb, dlogit,
                                     fctx.wgrad[2])
            if fctx.wgrad[2]:  # detached embedding: nothing reaches the LSTM
                return None, None, None, None, None
        dh = K.zeros((N * T, HIDDEN), dev)
        last_out = _p(dh) + (T - 1) * HIDDEN * 4
        lib.fs2_clf_head(last_in, T * HIDDEN, N, *w["head"], fctx.p,
                         _p(fctx.seed) if fctx.p > 0 else None, fctx.emb_mod.site, None, None,
                         _p(demb) if demb is not None else None,
                         _p(dlogit) if dlogit is not None else None, last_out, T * HIDDEN,
                         K.stream())
        c, act = fctx.saved
        st = w["stack"]
        dgates = torch.empty(LAYERS, N * T, 4 * HIDDEN, device=dev)
        dc = torch.empty(LAYERS * 2 * N * HIDDEN, device=dev)
        dx = torch.empty(N * T, D, device=dev) if fctx.needs_input_grad[0] else None
        lib.fs2_lstm_stack_bwd(_p(dh), N, T, D, HIDDEN, LAYERS, _p(st["w_ih0_t"]),
                               _p(st["w_ih_up_t"]), _p(st["w_hh_t"]), _p(act), _p(c), _p(dgates),
                               _p(dc), K.ptr(dx), K.stream())
        if fctx.wgrad is not None:
            fctx.emb_mod._lstm_wgrad(fctx.wgrad[0], fctx.wgrad[1], dgates, N, T)
        dh = dx
        return (dh.view(N, T, D) if dh is not None else None), None, None, None, None


class _Module(nn.Module):
    pass


def _linear_norm(in_dim, out_dim, dev):
    m = _Module()
    m.linear_layer = nn.Linear(in_dim, out_dim, device=dev)
    return m


class SpeechEmbedder(nn.Module):
    """``speech_embedder_net.py:65-146`` (language DA head); ``architecture`` is
    ``hp.model.architecture``: ``'LSTM'`` (``LSTM_stack``) or ``'rescnn'`` (``_feat_extractor``,
    ``hp.model.hidden`` = 640).

    ``weight_grads=False`` is the ``--use_clf`` discriminator: the backward gives the input
    gradient only and no parameter gets a ``.grad``.  With ``True`` the backward also
    accumulates every parameter's gradient into ``.grad`` (``embedder_train.EmbedderTrainer``),
    and ``forward(x, detach=True)`` back-propagates into the classifier alone."""

    def __init__(self, device="cuda", weight_grads=False, architecture="LSTM"):
        super().__init__()
        if architecture not in ("LSTM", "rescnn"):
            raise ValueError(f"architecture {architecture!r}: 'LSTM' or 'rescnn'")
        self.architecture = architecture
        self.weight_grads = bool(weight_grads)
        dev = torch.device(device)
        if architecture == "LSTM":
            self.LSTM_stack = nn.LSTM(NMELS, HIDDEN, num_layers=LAYERS, batch_first=True,
                                      device=dev)
            self.hidden = HIDDEN
        else:
            from . import rescnn
            self._feat_extractor = rescnn.ResCNN(dev)
            self.hidden = rescnn.FEATURES
            self.feat_dropout = rescnn.FEAT_DROPOUT
            self.site_feat = 0x5E2F  # dropout stream of the pooled features
        self.projection = _linear_norm(self.hidden, PROJ, dev)
        self.da_classifier = _Module()
        self.da_classifier.classifier = _Module()
        self.da_classifier.classifier.layer = nn.Sequential()
        for i, o in enumerate((PROJ, PROJ, 1)):
            self.da_classifier.classifier.layer.add_module(f"linear_{i}", _linear_norm(PROJ, o, dev))
        self.da_dropout = DA_DROPOUT
        self.site = 0x5E2E  # dropout stream of the classifier
        self._key = None
        self._seed_state = None
        self.seed(0x6E2E)

    def seed(self, s):
        """Dropout streams (the classifier's and, for 'rescnn', the pooled features'; one key,
        two sites): call k draws key splitmix64(s, k) on the device."""
        self._seed_base = int(s) & (2 ** 63 - 1)
        self._seed_state = None

    def _prep(self):
        """Kernel-layout weights: combined LSTM biases, transposes (fs2_conv_weight_prep's
        w_bwd of a taps = 1 weight is its transpose); rebuilt when a weight changes."""
        key = tuple(p._version for p in self.parameters())
        if self._key == key:
            return self._cache
        dev = self.projection.linear_layer.weight.device

        def t(w):  # (out, in) -> (in, out)
            o, i = w.shape
            wt = torch.empty(i, o, device=dev)
            K.weight_prep(w.detach().contiguous(), o, i, 1, w_bwd=wt)
            return wt

        if self.architecture == "rescnn":
            from . import rescnn
            self._cache = {"conv": rescnn.prep(self._feat_extractor)}
            self._cache.update(self._prep_head(t))
            self._key = key
            return self._cache
        lstm = []
        for l in range(LAYERS):
            w_ih = getattr(self.LSTM_stack, f"weight_ih_l{l}").detach().contiguous()
            w_hh = getattr(self.LSTM_stack, f"weight_hh_l{l}").detach().contiguous()
            bias = K.add(getattr(self.LSTM_stack, f"bias_ih_l{l}").detach().contiguous(),
                         getattr(self.LSTM_stack, f"bias_hh_l{l}").detach().contiguous())
            lstm.append({"w_ih": w_ih, "w_ih_t": t(w_ih), "w_hh": w_hh, "w_hh_t": t(w_hh),
                         "bias": bias})
        stack = {
            "w_ih0": lstm[0]["w_ih"], "w_ih0_t": lstm[0]["w_ih_t"],
            "w_ih_up": torch.stack([lstm[l]["w_ih"] for l in range(1, LAYERS)]),
            "w_ih_up_t": torch.stack([lstm[l]["w_ih_t"] for l in range(1, LAYERS)]),
            "w_hh": torch.stack([lstm[l]["w_hh"] for l in range(LAYERS)]),
            "w_hh_t": torch.stack([lstm[l]["w_hh_t"] for l in range(LAYERS)]),
            "bias": torch.stack([lstm[l]["bias"] for l in range(LAYERS)]),
        }
        self._cache = {"lstm": lstm, "stack": stack}
        self._cache.update(self._prep_head(t))
        self._key = key
        return self._cache

    def _prep_head(self, t):
        L = self._head_layers()
        wts = [l.weight.detach().contiguous() for l in L]
        bs = [l.bias.detach().contiguous() for l in L]
        keep = (wts[0], t(wts[0]), bs[0], wts[1], t(wts[1]), bs[1], wts[2], t(wts[2]), bs[2],
                wts[3], bs[3])
        return {"head": tuple(_p(a) for a in keep), "keep": keep}

    def forward(self, x, detach=False):
        """x (N, 150, 80) fp32 on the GPU -> {'embeddings': (N, 64), 'da_lang_logits': (N,)}."""
        fn = _EmbedderFn
        drops = self.da_dropout
        if self.architecture == "rescnn":
            from .rescnn import _ResCNNEmbedderFn as fn
            if x.dim() != 3 or x.shape[2] != NMELS:
                raise ValueError(f"rescnn embedder: input {tuple(x.shape)}, expected (N, T, "
                                 f"{NMELS})")
            drops = max(self.da_dropout, self.feat_dropout)
        if self._seed_state is None:
            self._seed_state = torch.tensor([self._seed_base, 0, 0], dtype=torch.int64,
                                            device=x.device)
        if self.training and drops > 0:
            K.seed_next(self._seed_state)  # a fresh dropout key per call
        seed = self._seed_state[2:3].clone()  # this call's key (the backward re-reads it)
        if self.weight_grads:
            # the parameters are not inputs of the function (their gradients are accumulated
            # by hand); one of them rides along so that autograd runs the backward
            emb, logit = fn.apply(x.float(), self, seed, bool(detach),
                                  self.projection.linear_layer.bias)
        else:
            emb, logit = fn.apply(x.float(), self, seed, False, None)
        if detach:
            emb = emb.detach()
        return {"embeddings": emb, "da_lang_logits": logit}

    # -- speech_embedder_net.py:97-118 -------------------------------------------------------
    def _head_layers(self):
        return [self.projection.linear_layer] + [
            getattr(self.da_classifier.classifier.layer, f"linear_{i}").linear_layer
            for i in range(3)]

    def da_parameters(self):
        return list(self.da_classifier.parameters())

    def main_parameters(self):
        feat = self.LSTM_stack if self.architecture == "LSTM" else self._feat_extractor
        return list(feat.parameters()) + list(self.projection.parameters())

    def compute_embedding(self, x):
        """``{'embeddings': (N, 64)}`` without the classifier's output."""
        return {"embeddings": self.forward(x)["embeddings"]}

    # -- weight gradients (weight_grads=True) ----------------------------------------------
    @staticmethod
    def _acc(p, g):
        """p.grad += g, like autograd's accumulation (p.grad may be a view of a flat arena)."""
        if p.grad is None:
            p.grad = K.zeros(p.shape, g.device)
        K.add(p.grad, g, out=p.grad)

    def _head_wgrad(self, last, ldx, n, w, p, seed, demb, dlogit, detach):
        dev = seed.device
        sizes = [PROJ * self.hidden, PROJ, PROJ * PROJ, PROJ, PROJ * PROJ, PROJ, PROJ, 1]
        buf = torch.empty(sum((s + 3) // 4 * 4 for s in sizes), device=dev)
        outs, o = [], 0
        for s in sizes:
            outs.append(buf[o:o + s])
            o += (s + 3) // 4 * 4
        tail = (*w["head"], p, _p(seed) if p > 0 else None, self.site, K.ptr(demb), K.ptr(dlogit),
                *[_p(t) for t in outs], 0)
        if self.architecture == "LSTM":
            nb = lib.fs2_clf_head_wgrad_ws_bytes(n)
            ws = K.ws(nb, dev)
            lib.fs2_clf_head_wgrad(last, ldx, n, *tail, _p(ws), nb, K.stream())
        else:
            nb = lib.fs2_clf_head_w_wgrad_ws_bytes(n)
            ws = K.ws(nb, dev)
            lib.fs2_clf_head_w_wgrad(last, ldx, n, self.hidden, *tail, _p(ws), nb, K.stream())
        for i, lin in enumerate(self._head_layers()):
            if i == 0 and detach:  # the classifier saw a detached embedding
                continue
            self._acc(lin.weight, outs[2 * i].view(lin.weight.shape))
            self._acc(lin.bias, outs[2 * i + 1].view(lin.bias.shape))

    def _lstm_wgrad(self, x, h, dgates, n_seq, steps):
        dev, G = x.device, 4 * HIDDEN
        dw_ih0 = torch.empty(G, NMELS, device=dev)
        dw_ih_up = torch.empty(LAYERS - 1, G, HIDDEN, device=dev)
        dw_hh = torch.empty(LAYERS, G, HIDDEN, device=dev)
        db = torch.empty(LAYERS, G, device=dev)
        K.lstm_stack_wgrad(x.view(n_seq * steps, NMELS), h, dgates, n_seq, steps, dw_ih0, dw_ih_up,
                           dw_hh, db, beta=0)
        for l in range(LAYERS):
            P = lambda n: getattr(self.LSTM_stack, f"{n}_l{l}")
            self._acc(P("weight_ih"), dw_ih0 if l == 0 else dw_ih_up[l - 1])
            self._acc(P("weight_hh"), dw_hh[l])
            self._acc(P("bias_ih"), db[l])  # b_ih and b_hh enter the gates as their sum
            self._acc(P("bias_hh"), db[l])


class _BCESumFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, logit, y):
        n = logit.shape[0]
        rows = torch.empty(n, 1, device=logit.device)
        lib.fs2_bce_logits(_p(logit), _p(y), n, _p(rows), None, 1.0, None, K.stream())
        out = torch.zeros(1, device=logit.device)
        K.colsum(rows, n, 1, out)  # fixed-order sum (reduction='sum')
        fctx.save_for_backward(logit, y)
        return out.view(())

    @staticmethod
    def backward(fctx, g):
        logit, y = fctx.saved_tensors
        d = torch.empty_like(logit)
        lib.fs2_bce_logits(_p(logit), _p(y), logit.shape[0], None, _p(g.contiguous().view(1)),
                           1.0, _p(d), K.stream())
        return d, None


class _GE2ESoftmaxFn(torch.autograd.Function):
    """``get_similarity`` + ``get_softmax_loss`` (utils.py:77-90, 126-135) with ``w sim + b``
    (speech_embedder_net.py:177), one kernel forward and one backward."""

    @staticmethod
    def forward(fctx, emb, w, b):
        fctx.save_for_backward(emb, w, b)
        return K.ge2e_softmax(emb, w.detach(), b.detach())

    @staticmethod
    def backward(fctx, g):
        emb, w, b = fctx.saved_tensors
        _, demb, dw, db = K.ge2e_softmax(emb, w.detach(), b.detach(), g=g.contiguous(),
                                         grads=True)
        return demb, dw, db


class _GE2EContrastFn(torch.autograd.Function):
    """``get_similarity`` + ``get_contrast_loss`` (utils.py:77-90, 106-124) with ``w sim + b``
    (speech_embedder_net.py:177), one kernel forward and one backward."""

    @staticmethod
    def forward(fctx, emb, w, b):
        fctx.save_for_backward(emb, w, b)
        return K.ge2e_contrast(emb, w.detach(), b.detach())

    @staticmethod
    def backward(fctx, g):
        emb, w, b = fctx.saved_tensors
        _, demb, dw, db = K.ge2e_contrast(emb, w.detach(), b.detach(), g=g.contiguous(),
                                          grads=True)
        return demb, dw, db


class GE2ELoss(nn.Module):
    """``speech_embedder_net.py:165-186`` (softmax or contrast GE2E + BCE domain loss);
    ``loss`` is ``hp.model.loss``."""

    _FNS = {"softmax": _GE2ESoftmaxFn, "contrast": _GE2EContrastFn}

    def __init__(self, device="cuda", loss="softmax"):
        super().__init__()
        if loss not in self._FNS:
            raise ValueError(f"loss {loss!r}: 'softmax' or 'contrast'")
        self.w = nn.Parameter(torch.tensor(10.0, device=device))
        self.b = nn.Parameter(torch.tensor(-5.0, device=device))
        self.loss = loss  # hp.model.loss

    def forward(self, embeddings, lang_logits, langs, **kwargs):
        N, M, _ = embeddings.shape
        if M != 1:
            loss = self._FNS[self.loss].apply(embeddings.contiguous(), self.w, self.b)
        else:  # utils.py:36, M - 1 = 0
            loss = torch.full((), float("nan"), device=embeddings.device)
        da = _BCESumFn.apply(lang_logits.contiguous(), langs.contiguous().float()) \
            if lang_logits is not None else torch.zeros((), device=embeddings.device)
        return loss + da, loss, da


class _RepadFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, x, t_dst):
        B, T, C = x.shape
        y = torch.empty(B, t_dst, C, device=x.device)
        lib.fs2_rows_repad(_p(x.contiguous()), B, T, t_dst, C, _p(y), K.stream())
        fctx.shape = (B, T, C, t_dst)
        return y

    @staticmethod
    def backward(fctx, dy):
        B, T, C, t_dst = fctx.shape
        dx = torch.empty(B, T, C, device=dy.device)
        lib.fs2_rows_repad(_p(dy.contiguous()), B, t_dst, T, C, _p(dx), K.stream())
        return dx, None


def chunk_mels(mel, chunk=CHUNK):
    """``train.py:178-183``: (B, T, 80) -> (B * (T // chunk + 1), chunk, 80), zero-padded
    (a full zero chunk when T is a multiple of ``chunk``, as the reference's ``// + 1``)."""
    B, T, C = mel.shape
    r = T // chunk + 1
    return _RepadFn.apply(mel, r * chunk).view(B * r, chunk, C), r


def chunk_langs(speaker_meta, rep, col=2):
    """``train.py:184``: ``speaker_meta[:, 2]`` repeated once per chunk."""
    B, ld = speaker_meta.shape
    y = torch.empty(B * rep, device=speaker_meta.device)
    m = speaker_meta.contiguous().float()
    lib.fs2_repeat_col(_p(m), B, ld, col, rep, _p(y), K.stream())
    return y


def da_coefficient(step, total_step):
    """``train.py:194``: 2 / (1 + exp(-10 p)) - 1 at p = step / total_step."""
    return 2 / (1 + math.exp(-10 * (step / total_step))) - 1
