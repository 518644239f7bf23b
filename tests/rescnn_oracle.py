"""Plain-torch restatement of the speaker encoder's ``rescnn`` architecture, for the tests
(a helper, not a test).  Written from the network's description, on the CPU, in float64 with
a float32 switch; gradients come from autograd.

  x (N, T, 80) -> (N, 1, H = 80 mel, W = T)
  four stages  conv(k5, s2, p2) BN ReLU | block: relu(BN(conv3(relu(BN(conv3(y))))) + y)
  with 16, 32, 64, 128 channels; mean over W; dropout; flatten (feature c * 5 + h);
  Linear(640 -> 64); L2 norm = embedding; Linear 64-64 drop ReLU, 64-64 drop ReLU, 64-1 = logit

The convolution is written as unfold (im2col) + matmul and BatchNorm from its formulas, so
that ``torch.nn.Conv2d`` / ``BatchNorm2d`` stay an independent check of this file
(``test_rescnn_cpu.py``).  Tensors here are NCHW; ``to_nwhc`` / ``from_nwhc`` convert to the
kernels' channels-last layout with time as the outer axis.
"""
import torch

WIDTHS = (16, 32, 64, 128)
EPS, MOMENTUM = 1e-5, 0.1
FE = "_feat_extractor."


def layer_names():
    """The twelve conv+BN layers in execution order: (state-dict prefix, k, stride, closes a
    residual block)."""
    out = []
    for i in range(1, 5):
        out += [(f"{FE}conv{i}.", 5, 2, False), (f"{FE}res{i}.conv1.", 3, 1, False),
                (f"{FE}res{i}.conv2.", 3, 1, True)]
    return out


def to_nwhc(t):
    """NCHW -> the kernels' (N, W, H, C)."""
    return t.permute(0, 3, 2, 1).contiguous()


def from_nwhc(t):
    return t.permute(0, 3, 2, 1).contiguous()


def conv2d(x, w, b, stride, pad):
    """x (N, C, H, W), w (O, C, k, k), b (O) or None."""
    N, C, H, W = x.shape
    O, _, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = torch.nn.functional.unfold(x, k, padding=pad, stride=stride)  # (N, C k k, Ho Wo)
    y = w.reshape(O, C * k * k) @ cols
    if b is not None:
        y = y + b[None, :, None]
    return y.reshape(N, O, Ho, Wo)


def batchnorm_train(z, gamma, beta, eps=EPS):
    """Batch statistics per channel over N, H, W.  Returns (out, mean, biased var)."""
    mean = z.mean(dim=(0, 2, 3))
    var = ((z - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
    out = (z - mean[None, :, None, None]) / torch.sqrt(var + eps)[None, :, None, None]
    return out * gamma[None, :, None, None] + beta[None, :, None, None], mean, var


def batchnorm_eval(z, gamma, beta, rm, rv, eps=EPS):
    out = (z - rm[None, :, None, None]) / torch.sqrt(rv + eps)[None, :, None, None]
    return out * gamma[None, :, None, None] + beta[None, :, None, None]


def pool_flatten(a):
    """(N, C, H, W) -> (N, C * H): mean over W, feature index c * H + h."""
    return a.mean(dim=3).reshape(a.shape[0], -1)


def ge2e_softmax(emb, w, b):
    """emb (N, M, D): the GE2E softmax loss with the exclude-self centroid on the diagonal."""
    N, M, D = emb.shape
    tot = emb.sum(1)
    cen, exc = tot / M, (tot[:, None, :] - emb) / (M - 1)

    def cos(a, c):
        return (a * c).sum(-1) / (a.norm(dim=-1).clamp(min=1e-8) * c.norm(dim=-1).clamp(min=1e-8))

    sim = cos(emb[:, :, None, :], cen[None, None, :, :])
    same = cos(emb, exc)
    eye = torch.eye(N, dtype=torch.bool)[:, None, :].expand(N, M, N)
    sim = torch.where(eye, same[:, :, None].expand(N, M, N), sim)
    S = w * sim + b
    pos = (S * eye).sum(-1)
    return (torch.log(torch.exp(S).sum(-1) + 1e-6) - pos).sum()


def bce_sum(logit, y):
    return torch.nn.functional.binary_cross_entropy_with_logits(logit, y.to(logit.dtype),
                                                                reduction="sum")


class Oracle:
    """The whole embedder from a state dict (the module's or the reference's).  Parameters are
    leaf tensors in ``dtype`` that require grad; ``buf`` holds the BatchNorm buffers, updated
    by training-mode forwards as ``torch.nn.BatchNorm2d`` updates them."""

    HEAD = ["projection.linear_layer."] + [
        f"da_classifier.classifier.layer.linear_{i}.linear_layer." for i in range(3)]

    def __init__(self, state_dict, dtype=torch.float64, device="cpu"):
        self.dtype, self.device = dtype, torch.device(device)
        self.par, self.buf = {}, {}
        for pre, _, _, _ in layer_names():
            for k in ("conv.weight", "conv.bias", "bn.weight", "bn.bias"):
                self.par[pre + k] = self._leaf(state_dict[pre + k])
            for k in ("bn.running_mean", "bn.running_var"):
                self.buf[pre + k] = state_dict[pre + k].detach().to(self.device, dtype).clone()
            self.buf[pre + "bn.num_batches_tracked"] = \
                state_dict[pre + "bn.num_batches_tracked"].detach().to(self.device).clone()
        for pre in self.HEAD:
            for k in ("weight", "bias"):
                self.par[pre + k] = self._leaf(state_dict[pre + k])

    def _leaf(self, t):
        return t.detach().to(self.device, self.dtype).clone().requires_grad_()

    def main_parameters(self):
        return [v for k, v in self.par.items() if not k.startswith("da_classifier")]

    def da_parameters(self):
        return [v for k, v in self.par.items() if k.startswith("da_classifier")]

    def features(self, x, training=True):
        """x (N, T, 80) -> the last feature map (N, 128, 5, W')."""
        P, B = self.par, self.buf
        a = x.to(self.dtype).transpose(1, 2).unsqueeze(1)
        skip = None
        for pre, k, stride, end in layer_names():
            z = conv2d(a, P[pre + "conv.weight"], P[pre + "conv.bias"], stride, k // 2)
            if training:
                y, mean, var = batchnorm_train(z, P[pre + "bn.weight"], P[pre + "bn.bias"])
                n = z.numel() // z.shape[1]
                with torch.no_grad():
                    B[pre + "bn.running_mean"].mul_(1 - MOMENTUM).add_(MOMENTUM * mean)
                    B[pre + "bn.running_var"].mul_(1 - MOMENTUM).add_(
                        MOMENTUM * var * (n / (n - 1) if n > 1 else 1.0))
                    B[pre + "bn.num_batches_tracked"] += 1
            else:
                y = batchnorm_eval(z, P[pre + "bn.weight"], P[pre + "bn.bias"],
                                   B[pre + "bn.running_mean"], B[pre + "bn.running_var"])
            if end:
                y = y + skip
            a = torch.relu(y)
            if stride == 2:
                skip = a
        return a

    def head(self, feat, detach=False):
        P, H = self.par, self.HEAD
        lin = lambda v, pre: v @ P[pre + "weight"].t() + P[pre + "bias"]  # noqa: E731
        p = lin(feat, H[0])
        emb = p / p.norm(dim=1, keepdim=True)
        e = emb.detach() if detach else emb
        h = torch.relu(lin(torch.relu(lin(e, H[1])), H[2]))
        return emb, lin(h, H[3]).squeeze(-1)

    def forward(self, x, training=True, detach=False, keep=None):
        """The classifier's dropout off; ``keep`` (N, 640) is the pooled features' keep-scale
        (0 or 1 / (1 - p)), None for no dropout."""
        feat = pool_flatten(self.features(x, training))
        if keep is not None:
            feat = feat * keep.to(feat)
        emb, logit = self.head(feat, detach)
        return {"embeddings": emb, "da_lang_logits": logit, "features": feat}
