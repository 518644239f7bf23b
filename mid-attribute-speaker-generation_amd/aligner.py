"""Phoneme durations without an outside aligner: the alignment learning framework (Badlani et
al., "One TTS Alignment To Rule Them All", 2021) as a stand-alone model.  Not in the reference,
whose corpora come aligned by the Montreal Forced Aligner (its ``jdit`` branch is not ported;
DESIGN.md §8).

  Aligner          phoneme embedding -> key encoder, log-mel -> query encoder; the soft alignment
                   is ``log_softmax_s(-temperature |q_t - k_s|^2)`` plus a beta-binomial prior
  AlignerTrainer   the CTC-style forward-sum loss, Adam, and monotonic alignment search for the
                   hard durations

Everything runs on the fp32 kernels: the convolutions are ``K.conv_gemm`` (forward and data
gradient, the ReLUs in its epilogues) and ``K.conv_wgrad``, the embedding ``K.embedding_fwd`` /
``K.embedding_bwd``, the alignment ``K.align_logprob`` / ``K.forward_sum`` / ``K.mas``
(csrc/align.hip).  Activations are (B * T, C) rows as everywhere in this package.
"""
import torch
import torch.nn as nn

from . import kernels as K
from .model import Conv1d, Embedding, ParamArena

BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam defaults


def _grad_of(p):
    """Where a parameter's gradient accumulates: its ``ParamArena`` view, else a fresh buffer."""
    g = getattr(p, "_fs2_grad", None)
    return (g, True) if g is not None else (K.zeros(p.shape, p.device), False)


class _ConvFn(torch.autograd.Function):
    """One Conv1d over (rows, c_in) rows; ``relu``: ReLU in the epilogue; ``in_relu``: the input
    is itself a ReLU output, so the data gradient is masked by it in the same epilogue."""

    @staticmethod
    def forward(ctx, x, weight, bias, seq_len, relu, in_relu):
        c_out, c_in, taps = weight.shape
        rows = x.shape[0]
        wf = torch.empty((c_out, taps * c_in), dtype=torch.float32, device=x.device)
        K.weight_prep(weight.detach(), c_out, c_in, taps, w_fwd=wf)
        y = K.conv_gemm(x, wf, rows, seq_len, c_in, c_out, taps, taps // 2, bias=bias.detach(),
                        flags=K.EPI_RELU if relu else 0)
        ctx.save_for_backward(x, weight, bias)
        ctx.geo = (rows, seq_len, c_in, c_out, taps, in_relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        rows, seq_len, c_in, c_out, taps, in_relu = ctx.geo
        dy = dy.contiguous()
        (dw, dw_own), (db, db_own) = _grad_of(weight), _grad_of(bias)
        K.conv_wgrad(dy, x, dw, rows, seq_len, c_in, c_out, taps, taps // 2, db=db)
        dx = None
        if ctx.needs_input_grad[0]:
            wb = torch.empty((c_in, taps * c_out), dtype=torch.float32, device=x.device)
            K.weight_prep(weight.detach(), c_out, c_in, taps, w_bwd=wb)
            dx = K.conv_gemm(dy, wb, rows, seq_len, c_out, c_in, taps, taps // 2,
                             flags=K.EPI_RELU_MASK_AUX if in_relu else 0,
                             aux=x if in_relu else None)
        return dx, None if dw_own else dw, None if db_own else db, None, None, None


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, table, padding_idx):
        ctx.save_for_backward(ids, table)
        ctx.padding_idx = padding_idx
        return K.embedding_fwd(ids, table.detach())

    @staticmethod
    def backward(ctx, dout):
        ids, table = ctx.saved_tensors
        dt, own = _grad_of(table)
        K.embedding_bwd(dout.contiguous(), ids, dt, ctx.padding_idx)
        return None, None if own else dt, None


class _LogProbFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, src_lens, mel_lens, temperature, omega):
        ctx.save_for_backward(q, k, src_lens, mel_lens)
        ctx.temperature = temperature
        return K.align_logprob(q, k, src_lens, mel_lens, temperature, omega)

    @staticmethod
    def backward(ctx, g):
        q, k, src_lens, mel_lens = ctx.saved_tensors
        dq, dk = K.align_logprob_bwd(q, k, g.contiguous(), src_lens, mel_lens, ctx.temperature)
        return dq, dk, None, None, None, None


class Aligner(nn.Module):
    """``forward(texts, mels)`` -> ``(q (B, T_m, attn_dim), k (B, T_s, attn_dim))``; texts
    (B, T_s) int64 symbol ids with 0 as padding, mels (B, T_m, n_mels) f32 log-mels, zero past
    each length.  ``channels`` and ``attn_dim`` are multiples of 8 (``attn_dim`` <= 128)."""

    def __init__(self, n_symbols, n_mels=80, channels=64, attn_dim=40, device="cuda"):
        super().__init__()
        if channels % 8 or attn_dim % 8 or n_mels % 8 or not 8 <= attn_dim <= K.ALIGN_MAX_WIDTH:
            raise ValueError(f"n_mels {n_mels}, channels {channels} and attn_dim {attn_dim} are "
                             f"multiples of 8, attn_dim at most {K.ALIGN_MAX_WIDTH}")
        self.n_symbols, self.n_mels, self.channels, self.attn_dim = n_symbols, n_mels, channels, \
            attn_dim
        self.embedding = Embedding(n_symbols, channels, padding_idx=0)
        self.key = nn.ModuleList([Conv1d(channels, channels, 3, 1), Conv1d(channels, attn_dim, 1, 0)])
        self.query = nn.ModuleList([Conv1d(n_mels, channels, 3, 1), Conv1d(channels, channels, 1, 0),
                                    Conv1d(channels, attn_dim, 1, 0)])
        self.to(device)

    @staticmethod
    def _stack(x, convs, seq_len):
        for i, c in enumerate(convs):
            x = _ConvFn.apply(x, c.weight, c.bias, seq_len, i + 1 < len(convs), i > 0)
        return x

    def forward(self, texts, mels):
        if texts.dim() != 2 or mels.dim() != 3 or mels.shape[0] != texts.shape[0] or \
                mels.shape[2] != self.n_mels:
            raise ValueError(f"texts is (B, T_s), mels (B, T_m, {self.n_mels})")
        (B, T_s), T_m = texts.shape, mels.shape[1]
        e = _EmbedFn.apply(texts.contiguous().view(-1), self.embedding.weight,
                           self.embedding.padding_idx)
        k = self._stack(e, self.key, T_s)
        q = self._stack(mels.contiguous().view(B * T_m, self.n_mels), self.query, T_m)
        return q.view(B, T_m, self.attn_dim), k.view(B, T_s, self.attn_dim)


class AlignerTrainer:
    """Adam on ``(1 / B) sum_b nll_b / M_b`` of the forward-sum loss; ``align`` gives the hard
    durations.  The lengths are device int64 tensors and are not read back; ``host_lens`` =
    (src, mel) lists, where the caller has them, lets a row with fewer frames than phonemes
    raise before anything is launched."""

    def __init__(self, model, lr=1e-3, temperature=0.05, omega=1.0):
        self.model = model
        self.device = next(model.parameters()).device
        self.lr, self.temperature, self.omega = float(lr), float(temperature), float(omega)
        self.arena = ParamArena(list(model.parameters()), self.device)
        self.m = K.zeros(self.arena.numel, self.device)
        self.v = K.zeros(self.arena.numel, self.device)
        self.step = 0

    def logprob(self, texts, src_lens, mels, mel_lens):
        q, k = self.model(texts, mels)
        return _LogProbFn.apply(q, k, src_lens, mel_lens, self.temperature, self.omega)

    def backward(self, texts, src_lens, mels, mel_lens, host_lens=None, optional=None):
        """The device loss, its parameter gradients left in ``arena.grad`` (``train_step`` without
        the update).  The forward-sum kernel returns the loss's gradient with the loss, so the
        graph is entered at ``logp`` with it.  ``optional`` (B, T_s) uint8 on the device marks
        positions that may take no frame (``K.forward_sum``); ``host_lens`` then carries the
        mask's host copy as its third member."""
        self.arena.zero_grad()
        w = (1.0 / texts.shape[0]) / mel_lens.clamp(1, mels.shape[1]).to(torch.float32)
        logp = self.logprob(texts, src_lens, mels, mel_lens)
        nll, grad = K.forward_sum(logp.detach(), src_lens, mel_lens, w, host_lens, optional)
        logp.backward(grad)
        return torch.dot(nll, w)

    def train_step(self, texts, src_lens, mels, mel_lens, host_lens=None, optional=None):
        loss = self.backward(texts, src_lens, mels, mel_lens, host_lens, optional)
        self.step += 1
        bc1, bc2 = 1.0 - BETAS[0] ** self.step, 1.0 - BETAS[1] ** self.step
        K.adam_step(self.arena.flat, self.arena.grad, self.m, self.v, None, self.lr, BETAS[0],
                    BETAS[1], EPS, bc1, bc2 ** 0.5)
        return loss

    def align(self, texts, src_lens, mels, mel_lens, host_lens=None, optional=None):
        """durations (B, T_s) int64 on the device: frames per phoneme, 0 past a row's phonemes
        and at an ``optional`` position that the path omits."""
        with torch.no_grad():
            return K.mas(self.logprob(texts, src_lens, mels, mel_lens), src_lens, mel_lens,
                         host_lens, optional)

    def fit(self, batches, steps):
        """``steps`` updates over ``batches``, an iterable of ``(texts, src_lens, mels, mel_lens)``
        or, with optional positions, ``(texts, src_lens, mels, mel_lens, optional)`` (cycled when
        it is a list); returns the device losses."""
        losses, it = [], None
        while len(losses) < steps:
            if it is None:
                it = iter(batches)
            try:
                batch = next(it)
            except StopIteration:
                if not losses:
                    raise ValueError("no batches") from None
                it = None
                continue
            losses.append(self.train_step(*batch[:4], optional=batch[4] if len(batch) > 4 else None))
        return losses

    def save(self, path):
        m = self.model
        torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()},
                    "m": self.m.cpu(), "v": self.v.cpu(), "step": self.step, "lr": self.lr,
                    "temperature": self.temperature, "omega": self.omega,
                    "shape": [m.n_symbols, m.n_mels, m.channels, m.attn_dim]}, path)

    def load(self, path):
        ck = torch.load(path, map_location="cpu")
        m = self.model
        if list(ck["shape"]) != [m.n_symbols, m.n_mels, m.channels, m.attn_dim]:
            raise ValueError(f"{path}: an aligner of shape {ck['shape']}")
        m.load_state_dict(ck["model"])  # copies into the arena's views
        self.m.copy_(ck["m"])
        self.v.copy_(ck["v"])
        self.step, self.temperature, self.omega = int(ck["step"]), float(ck["temperature"]), \
            float(ck["omega"])
        return self
