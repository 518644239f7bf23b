"""The ``rescnn`` feature extractor of the speaker encoder on the HIP path.

Mirrors ``Multilingual-Speaker-Encoder-with-Domain-Adaptation/speech_embedder_net.py:19-63``
(``ResCNN``) and ``module.py:59-117`` (``ConvNorm2D``, ``ResBlock``): four stages of
``Conv2d(k5, s2) + BatchNorm2d + ReLU`` and a residual block of two ``Conv2d(k3) + BatchNorm2d``
over the (mel, time) plane, the mean over time, ``Dropout(0.5)`` and the channel-major flatten
to 640 features.  The modules here only hold the parameters and buffers under the reference's
state-dict keys (its ``nn.Sequential`` registers the twelve ConvNorm2D modules a second time
under ``conv_layer.*``; the tensors are shared).  The arithmetic is ``csrc/rescnn.hip``, driven
by ``_ResCNNEmbedderFn``: channels-last activations with time as the outer axis, so the input
``(N, T, 80)`` is read as it is.

Training mode (which the ``--use_clf`` loop of ``train.py`` never leaves) normalises with batch
statistics and moves the running buffers; eval mode folds the running statistics into the conv
epilogue, one launch per conv layer.  The backward exists for training mode only.
"""
import torch
import torch.nn as nn

from . import kernels as K
from ._lib import lib

WIDTHS = (16, 32, 64, 128)
FEATURES = 5 * WIDTHS[-1]  # 80 mel bins halved four times, times the last width
FEAT_DROPOUT = 0.5         # speech_embedder_net.py:23
PROJ = 64


def _p(t):
    return t.data_ptr()


class ConvNorm2D(nn.Module):
    def __init__(self, c_in, c_out, kernel_size, stride, dev):
        super().__init__()
        self.conv = nn.Conv2d(c_in, c_out, kernel_size, stride, kernel_size // 2, device=dev)
        nn.init.xavier_uniform_(self.conv.weight, gain=nn.init.calculate_gain("relu"))
        self.bn = nn.BatchNorm2d(c_out, device=dev)


class ResBlock(nn.Module):
    def __init__(self, c, dev):
        super().__init__()
        self.conv1 = ConvNorm2D(c, c, 3, 1, dev)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = ConvNorm2D(c, c, 3, 1, dev)


class ResCNN(nn.Module):
    """Parameter container with the reference's module tree; ``layers()`` lists the twelve
    ConvNorm2D modules in execution order as ``(module, is_block_end)``."""

    def __init__(self, dev):
        super().__init__()
        self.dropout = nn.Dropout(FEAT_DROPOUT)
        self.relu = nn.ReLU(inplace=True)
        c_in, seq = 1, []
        for i, c in enumerate(WIDTHS, 1):
            conv, res = ConvNorm2D(c_in, c, 5, 2, dev), ResBlock(c, dev)
            setattr(self, f"conv{i}", conv)
            setattr(self, f"res{i}", res)
            seq += [conv, self.relu, res]
            c_in = c
        self.avgpool = nn.AdaptiveAvgPool2d((None, 1))
        self.conv_layer = nn.Sequential(*seq)

    def layers(self):
        out = []
        for i in range(1, len(WIDTHS) + 1):
            res = getattr(self, f"res{i}")
            out += [(getattr(self, f"conv{i}"), False), (res.conv1, False), (res.conv2, True)]
        return out


def _geom(m, n, w, h):
    """(n, w, h, c_in, c_out, k, stride, pad) of a ConvNorm2D on an (n, w, h, c_in) input and
    its output extents."""
    c = m.conv
    k, s, pad = c.kernel_size[0], c.stride[0], c.padding[0]
    g = (n, w, h, c.in_channels, c.out_channels, k, s, pad)
    return g, (w + 2 * pad - k) // s + 1, (h + 2 * pad - k) // s + 1


def prep(net):
    """Kernel-layout conv weights, one ``(w_fwd, w_bwd)`` pair per layer."""
    out = []
    for m, _ in net.layers():
        w = m.conv.weight.detach().contiguous()
        wf, wb = torch.empty_like(w), torch.empty_like(w)
        lib.fs2_conv2d_weight_prep(_p(w), w.shape[0], w.shape[1], w.shape[2], _p(wf), _p(wb),
                                   K.stream())
        out.append((wf, wb))
    return out


def _conv(x, g, wf, bias, scale=None, shift=None, res=None, relu=0):
    n, w, h, ci, co, k, s, pad = g
    wo, ho = (w + 2 * pad - k) // s + 1, (h + 2 * pad - k) // s + 1
    y = torch.empty(n, wo, ho, co, device=x.device)
    lib.fs2_conv2d_fwd(_p(x), n, w, h, ci, _p(wf), K.ptr(bias), co, k, s, pad, K.ptr(scale),
                       K.ptr(shift), K.ptr(res), relu, _p(y), K.stream())
    return y


def folded(net, cache):
    """The eval-mode per-channel (scale, shift) of every layer, kept in ``cache['fold']`` beside
    the prepared weights.  Rebuilt when the weights are (``SpeechEmbedder._prep``), after a
    training-mode forward (which moves the running statistics in place and drops the entry) and
    when a BatchNorm buffer's version changes (``load_state_dict``)."""
    key = tuple(b._version for m, _ in net.layers() for b in (m.bn.running_mean, m.bn.running_var))
    if cache.get("fold") is None or cache["fold"][0] != key:
        out = []
        for m, _ in net.layers():
            bn, c = m.bn, m.conv.out_channels
            fold = torch.empty(2, c, device=bn.weight.device)
            lib.fs2_bn2d_fold(_p(bn.weight.detach()), _p(bn.bias.detach()), _p(bn.running_mean),
                              _p(bn.running_var), bn.eps, c, _p(fold[0]), _p(fold[1]), K.stream())
            out.append(fold)
        cache["fold"] = (key, out)
    return cache["fold"][1]


def features_eval(net, x, wk, folds):
    """Eval-mode feature map (N, W', 5, 128): BatchNorm folded into the conv epilogue, one
    launch per conv layer."""
    n, w, h = x.shape
    act, skip = x, None
    for (m, end), (wf, _), fold in zip(net.layers(), wk, folds):
        g, wo, ho = _geom(m, n, w, h)
        out = _conv(act, g, wf, m.conv.bias.detach(), fold[0], fold[1], skip if end else None, 1)
        if g[6] == 2:  # the stage's strided conv: its output is the residual of the block
            skip = out
        act, w, h = out, wo, ho
    return act


def features_train(net, x, wk):
    """Training-mode feature map and what the backward needs per layer:
    ``(geometry, input, z, out, mean, rstd)``."""
    n, w, h = x.shape
    dev = x.device
    act, skip, saved = x, None, []
    for (m, end), (wf, _) in zip(net.layers(), wk):
        g, wo, ho = _geom(m, n, w, h)
        bn, co = m.bn, g[4]
        z = _conv(act, g, wf, m.conv.bias.detach())
        rows = n * wo * ho
        stats = torch.empty(2, co, device=dev)
        out = torch.empty_like(z)
        nb = lib.fs2_bn2d_ws_bytes(rows, co)
        ws = K.ws(nb, dev)
        lib.fs2_bn2d_fwd(_p(z), rows, co, _p(bn.weight.detach()), _p(bn.bias.detach()), bn.eps,
                         bn.momentum, _p(bn.running_mean), _p(bn.running_var),
                         _p(bn.num_batches_tracked), _p(stats[0]), _p(stats[1]),
                         K.ptr(skip if end else None), 1, _p(out), _p(ws), nb, K.stream())
        saved.append((g, act, z, out, stats))
        if g[6] == 2:
            skip = out
        act, w, h = out, wo, ho
    return act, saved


def features_backward(net, wk, saved, dact, acc, want_dx):
    """Back-propagates ``dact`` (the gradient of the last feature map) through the twelve
    layers.  ``acc(param, grad)`` receives every parameter gradient (``None``: none is
    formed); returns the gradient of the input (N, T, 80) when ``want_dx``."""
    layers = net.layers()
    dev = dact.device
    g_skip = None  # gradient of the block's residual input, added where the block begins
    for i in range(len(layers) - 1, -1, -1):
        (m, end), (_, wb) = layers[i], wk[i]
        g, x_in, z, out, stats = saved[i]
        n, w, h, ci, co, k, s, pad = g
        rows = z.numel() // co
        gbuf, dz = torch.empty_like(z), torch.empty_like(z)
        dgb = torch.empty(2, co, device=dev)
        nb = lib.fs2_bn2d_ws_bytes(rows, co)
        ws = K.ws(nb, dev)
        lib.fs2_bn2d_bwd(_p(dact), _p(out), _p(z), _p(stats[0]), _p(stats[1]),
                         _p(m.bn.weight.detach()), rows, co, 1, _p(gbuf), _p(dz), _p(dgb[0]),
                         _p(dgb[1]), _p(ws), nb, K.stream())
        if end:
            g_skip = gbuf
        del out, dact
        if acc is not None:
            dw, db = torch.empty_like(m.conv.weight), torch.empty(co, device=dev)
            nb = lib.fs2_conv2d_wgrad_ws_bytes(n, w, h, ci, co, k, s, pad)
            ws = K.ws(nb, dev)
            lib.fs2_conv2d_wgrad(_p(x_in), _p(dz), n, w, h, ci, co, k, s, pad, _p(dw), _p(db), 0,
                                 _p(ws), nb, K.stream())
            acc(m.conv.weight, dw)
            acc(m.conv.bias, db)
            acc(m.bn.weight, dgb[0])
            acc(m.bn.bias, dgb[1])
        if i == 0 and not want_dx:
            return None
        # the layer after a strided conv opens a residual block: its input also feeds the skip
        add = g_skip if (s == 1 and not end) else None
        dact = torch.empty(n, w, h, ci, device=dev)
        lib.fs2_conv2d_dgrad(_p(dz), n, w, h, ci, _p(wb), co, k, s, pad, K.ptr(add), _p(dact),
                             K.stream())
    return dact.view(n, w, h)


def pool_drop(act, p, seed, site):
    n, w, h, c = act.shape
    out = torch.empty(n, c * h, device=act.device)
    lib.fs2_pool_drop_fwd(_p(act), n, w, h, c, p, _p(seed) if p > 0 else None, site, _p(out),
                          K.stream())
    return out


def pool_drop_bwd(dfeat, shape, p, seed, site):
    n, w, h, c = shape
    dx = torch.empty(shape, device=dfeat.device)
    lib.fs2_pool_drop_bwd(_p(dfeat), n, w, h, c, p, _p(seed) if p > 0 else None, site, _p(dx),
                          K.stream())
    return dx


class _ResCNNEmbedderFn(torch.autograd.Function):
    """``SpeechEmbedder.forward`` for ``architecture='rescnn'``: feature extractor, pool +
    dropout + flatten, the 640-wide head."""

    @staticmethod
    def forward(fctx, x, emb_mod, seed, detach, anchor):
        N, T, D = x.shape
        dev = x.device
        w = emb_mod._prep()
        net = emb_mod._feat_extractor
        xc = x.contiguous()
        train = emb_mod.training
        if train:
            w["fold"] = None  # the running statistics move
            act, saved = features_train(net, xc, w["conv"])
        else:
            act, saved = features_eval(net, xc, w["conv"], folded(net, w)), None
        pf = emb_mod.feat_dropout if train else 0.0
        feat = pool_drop(act, pf, seed, emb_mod.site_feat)
        emb = torch.empty(N, PROJ, device=dev)
        logit = torch.empty(N, device=dev)
        p = emb_mod.da_dropout if train else 0.0
        lib.fs2_clf_head_w(_p(feat), FEATURES, N, FEATURES, *w["head"], p,
                           _p(seed) if p > 0 else None, emb_mod.site, _p(emb), _p(logit), None,
                           None, None, 0, K.stream())
        fctx.emb_mod, fctx.saved, fctx.feat, fctx.seed = emb_mod, saved, feat, seed
        fctx.act_shape, fctx.p, fctx.pf, fctx.detach = tuple(act.shape), p, pf, detach
        fctx.wgrad = emb_mod.weight_grads
        return emb, logit

    @staticmethod
    def backward(fctx, demb, dlogit):
        mod, feat = fctx.emb_mod, fctx.feat
        N, dev = feat.shape[0], feat.device
        w = mod._prep()
        demb = demb.contiguous() if demb is not None else None
        dlogit = dlogit.contiguous() if dlogit is not None else None
        if fctx.saved is None and not (fctx.wgrad and fctx.detach):
            # before anything is accumulated: no parameter's .grad is touched
            raise NotImplementedError("the rescnn encoder's backward is built for training mode "
                                      "only (eval mode folds BatchNorm into the conv epilogue)")
        if fctx.wgrad:
            mod._head_wgrad(_p(feat), FEATURES, N, w, fctx.p, fctx.seed, demb, dlogit,
                            fctx.detach)
            if fctx.detach:  # detached embedding: nothing reaches the feature extractor
                return None, None, None, None, None
        dfeat = torch.empty(N, FEATURES, device=dev)
        lib.fs2_clf_head_w(_p(feat), FEATURES, N, FEATURES, *w["head"], fctx.p,
                           _p(fctx.seed) if fctx.p > 0 else None, mod.site, None, None,
                           K.ptr(demb), K.ptr(dlogit), _p(dfeat), FEATURES, K.stream())
        dact = pool_drop_bwd(dfeat, fctx.act_shape, fctx.pf, fctx.seed, mod.site_feat)
        dx = features_backward(mod._feat_extractor, w["conv"], fctx.saved, dact,
                               mod._acc if fctx.wgrad else None, fctx.needs_input_grad[0])
        return dx, None, None, None, None
