"""A small CTC phoneme recogniser over log-mels, for the phoneme error rate (PER) of synthesised
speech against its input phonemes.  Not in the reference, which judges synthesis by
ear.

  PhonemeRecognizer    ``layers`` Conv1d + ReLU over the log-mel rows, then a k = 1 Conv1d to the
                       classes: logits (B, T, ld); the mel and every hidden layer are zeroed
                       past each row's length, so a row's result does not depend on its padding
  RecognizerTrainer    the CTC loss (``K.ctc_loss``), Adam, greedy transcription
                       (``K.ctc_greedy``) and the edit-distance records (``K.edit_distance``)

Symbol id 0 is the padding of every text and never a target, so class 0 is the CTC blank and the
classes are the ``n_symbols`` ids.  The convolutions are ``K.conv_gemm`` / ``K.conv_wgrad`` through
the aligner's conv autograd function; they need ``c_out % 8 == 0``, so the output layer is padded
to the next multiple of 8 (429 -> 432) and ``ld`` is passed to the kernels: the pad columns are
never read and their gradient is exactly 0, which keeps those weights inert.

What the PER is: that of THIS recogniser, trained on the same corpus.  It compares runs that share
a recogniser checkpoint; it is no word error rate, no substitute for a listening test, and says
nothing across recognisers.
"""
import torch
import torch.nn as nn

from . import kernels as K
from .aligner import BETAS, EPS, _ConvFn
from .model import Conv1d, ParamArena


class PhonemeRecognizer(nn.Module):
    """``forward(mels, mel_lens)`` -> logits (B, T, ld) f32, ``ld`` = ``n_symbols`` rounded up to
    a multiple of 8; mels (B, T, n_mels) f32 log-mels, whatever they hold past each length.
    ``n_mels`` and ``channels`` are multiples of 8, ``kernel`` is odd."""

    def __init__(self, n_symbols, n_mels=80, channels=256, layers=4, kernel=5, device="cuda"):
        super().__init__()
        if n_mels % 8 or channels % 8 or kernel % 2 != 1 or layers < 1:
            raise ValueError(f"n_mels {n_mels} and channels {channels} are multiples of 8, kernel "
                             f"{kernel} is odd, layers {layers} at least 1")
        if not 2 <= n_symbols <= K.CTC_MAX_CLASSES:
            raise ValueError(f"n_symbols {n_symbols}: 2..{K.CTC_MAX_CLASSES}")
        self.n_symbols, self.n_mels, self.channels = int(n_symbols), int(n_mels), int(channels)
        self.layers, self.kernel = int(layers), int(kernel)
        self.ld = (self.n_symbols + 7) // 8 * 8
        self.convs = nn.ModuleList([Conv1d(n_mels if i == 0 else channels, channels, kernel,
                                           kernel // 2) for i in range(layers)])
        self.out = Conv1d(channels, self.ld, 1, 0)
        self.to(device)

    def shape(self):
        return [self.n_symbols, self.n_mels, self.channels, self.layers, self.kernel]

    def forward(self, mels, mel_lens=None):
        """``mel_lens`` (B) device int64 (None: every frame is live): the mel and every hidden
        layer are zeroed at ``t >= mel_lens[b]`` before the next convolution reads them, so a
        row's logits below its length depend neither on what the caller left in the padding (a
        free-running PostNet mel is not zero there) nor on how far the batch pads it."""
        if mels.dim() != 3 or mels.shape[2] != self.n_mels:
            raise ValueError(f"mels is (B, T, {self.n_mels})")
        B, T = mels.shape[:2]
        x = mels.contiguous().view(B * T, self.n_mels)
        live = None
        if mel_lens is not None:
            frames = torch.arange(T, device=mels.device)
            live = (frames[None, :] < mel_lens.view(B, 1)).view(B * T, 1)
            x = torch.where(live, x, torch.zeros_like(x))
        for i, c in enumerate(self.convs):
            x = _ConvFn.apply(x, c.weight, c.bias, T, True, i > 0)
            if live is not None:
                # still a ReLU output (>= 0, 0 where masked): the next layer's data gradient is
                # masked by it as before, and the mask's own backward zeroes the dead frames
                x = torch.where(live, x, torch.zeros_like(x))
        x = _ConvFn.apply(x, self.out.weight, self.out.bias, T, False, True)
        return x.view(B, T, self.ld)


class RecognizerTrainer:
    """Adam on ``(1 / B) sum_b nll_b / M_b`` of the CTC loss over the rows with a finite nll.  The
    lengths are device int64 tensors and are not read back; ``host_lens`` = (src, mel) lists,
    where the caller has them, lets a row with fewer frames than phonemes raise before anything
    is launched."""

    def __init__(self, model, lr=1e-3):
        self.model = model
        self.device = next(model.parameters()).device
        self.lr = float(lr)
        self.arena = ParamArena(list(model.parameters()), self.device)
        self.m = K.zeros(self.arena.numel, self.device)
        self.v = K.zeros(self.arena.numel, self.device)
        self.step = 0

    def backward(self, texts, src_lens, mels, mel_lens, host_lens=None):
        """The device loss, its parameter gradients left in ``arena.grad`` (``train_step`` without
        the update).  The CTC kernel returns the loss's gradient with the loss, so the graph is
        entered at the logits with it."""
        self.arena.zero_grad()
        m = self.model
        live = mel_lens.clamp(1, mels.shape[1])
        w = (1.0 / texts.shape[0]) / live.to(torch.float32)
        logits = m(mels, live)
        nll, grad = K.ctc_loss(logits.detach(), texts.contiguous(), mel_lens, src_lens, w,
                               n_classes=m.n_symbols, blank=0, host_lens=host_lens)
        logits.backward(grad)
        return torch.dot(torch.where(torch.isfinite(nll), nll, torch.zeros_like(nll)), w)

    def train_step(self, texts, src_lens, mels, mel_lens, host_lens=None):
        loss = self.backward(texts, src_lens, mels, mel_lens, host_lens)
        self.step += 1
        bc1, bc2 = 1.0 - BETAS[0] ** self.step, 1.0 - BETAS[1] ** self.step
        K.adam_step(self.arena.flat, self.arena.grad, self.m, self.v, None, self.lr, BETAS[0],
                    BETAS[1], EPS, bc1, bc2 ** 0.5)
        return loss

    def fit(self, batches, steps):
        """``steps`` updates over ``batches``, an iterable of ``(texts, src_lens, mels, mel_lens)``
        (cycled when it is a list); returns the device losses."""
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
            losses.append(self.train_step(*batch))
        return losses

    def transcribe(self, mels, mel_lens):
        """``(ids (B, T) int64, 0 past the length, lens (B) int64)`` on the device: the greedy CTC
        transcription of each utterance."""
        with torch.no_grad():
            lens = mel_lens.to(torch.int64).clamp(1, mels.shape[1]).contiguous()
            logits = self.model(mels.float(), lens)  # frames past a length are masked there
            return K.ctc_greedy(logits, lens, n_classes=self.model.n_symbols, blank=0)

    def errors(self, mels, mel_lens, texts, src_lens):
        """(B, 4) int64 on the device: [distance, substitutions, deletions, insertions] of each
        transcription against ``texts`` (B, T_s) int64 with lengths ``src_lens``."""
        ids, lens = self.transcribe(mels, mel_lens)
        return K.edit_distance(texts.to(torch.int64).contiguous(),
                               src_lens.to(torch.int64).contiguous(), ids, lens)

    def save(self, path):
        m = self.model
        torch.save({"model": {k: v.cpu() for k, v in m.state_dict().items()},
                    "m": self.m.cpu(), "v": self.v.cpu(), "step": self.step, "lr": self.lr,
                    "shape": m.shape()}, path)

    def load(self, path, ck=None):
        """``ck``: the checkpoint where the caller has read ``path`` already."""
        ck = torch.load(path, map_location="cpu") if ck is None else ck
        m = self.model
        if list(ck["shape"]) != m.shape():
            raise ValueError(f"{path}: a recogniser of shape {ck['shape']}")
        m.load_state_dict(ck["model"])  # copies into the arena's views
        self.m.copy_(ck["m"])
        self.v.copy_(ck["v"])
        self.step = int(ck["step"])
        return self


def load_recognizer(path, device="cuda"):
    """A ``RecognizerTrainer`` around the recogniser saved at ``path`` (``RecognizerTrainer.save``),
    its shape taken from the checkpoint."""
    ck = torch.load(path, map_location="cpu")
    if not isinstance(ck, dict) or "shape" not in ck or len(ck["shape"]) != 5:
        raise ValueError(f"{path}: not a recogniser checkpoint")
    return RecognizerTrainer(PhonemeRecognizer(*[int(v) for v in ck["shape"]], device=device)
                             ).load(path, ck)
