"""ORACLE -- TEST INFRASTRUCTURE ONLY.  Plain torch / numpy, CPU: the vocoder's hand-written
kernels restated with their documented rounding points, for tests/test_gpu_vocoder_kernels.py
(checked itself, without a GPU, by tests/test_vocoder_oracle_cpu.py).

* ``resblock1``: one HiFi-GAN ResBlock1 (hifigan/models.py:21-53) on (rows, C) rows with the
  rounding points of csrc/resblock.hip's header -- bf16 conv operands, fp32 residual stream,
  the stage's running sum folded in -- and the conv accumulation in fp64 or fp32.
* ``conv_post`` / ``pcm_of``: conv_post + tanh in fp64 and the int16 rule of fs2_vocoder_post.
* ``lattice``: inputs on which every fp32 partial sum of every conv is exactly representable,
  so the summation order (MFMA, per-conv launches, fp32, fp64) cannot matter and a kernel can
  be compared bitwise.  ``resblock1(..., spans=[])`` records what that claim needs.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

F32 = torch.float32


def _bf16(t):
    """Round to bf16 (nearest even), keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def _lrelu(v, alpha):
    """fp32 leaky ReLU as the kernels write it: v >= 0 ? v : alpha * v, alpha an fp32."""
    return torch.where(v >= 0, v, v * torch.tensor(alpha, dtype=F32))


def _lsb(t):
    """Smallest lowest-set-bit value over the nonzero elements of an fp32 tensor (inf if none)."""
    a = t.detach().to(F32).reshape(-1).numpy()
    a = a[a != 0]
    if a.size == 0:
        return math.inf
    bits = a.view(np.int32).astype(np.int64)
    exp = (bits >> 23) & 0xFF
    assert exp.min() > 0, "denormal operand"
    mant = (bits & 0x7FFFFF) | 0x800000
    tz = np.log2((mant & -mant).astype(np.float64)).astype(np.int64)
    return float(2.0 ** (exp - 150 + tz).min())


def _conv(xop, w, k, d, T, dtype, spans, bias):
    """Conv1d over time of (rows, C) rows (utterances of T rows, zero padding at their
    edges), accumulated in ``dtype``; the result as fp32."""
    rows, C = xop.shape
    xb = xop.view(rows // T, T, C).transpose(1, 2)
    y = F.conv1d(xb.to(dtype), w.to(dtype), None, padding=(k - 1) // 2 * d, dilation=d)
    if spans is not None:  # largest sum of magnitudes over the smallest bit any term can set
        top = F.conv1d(xb.double().abs(), w.double().abs(), None, padding=(k - 1) // 2 * d,
                       dilation=d).max().item() + bias.abs().max().item()
        spans.append(top / (_lsb(xop) * _lsb(w)))
    return y.transpose(1, 2).reshape(rows, C).to(F32)


def resblock1(x, w1, w2, b1, b2, k, dil, *, T, acc_in=None, scale=1.0, alpha2=None,
              dtype=torch.float64, bf16=True, spans=None):
    """x (rows, C) fp32; w1 / w2: three (C, C, k) conv weights each, b1 / b2 three (C,) biases.
    Returns (v, hc): v = fp32(fp32(out + acc_in) * scale) -- the kernel's xs -- and
    hc = bf16(lrelu(v, alpha2)) when alpha2 is given, else None.

    Rounding points (csrc/resblock.hip): conv operands bf16(lrelu_fp32(cur, 0.1f)) and
    bf16(lrelu_fp32(conv1 + b1, 0.1f)), bf16 weights, the residual stream
    cur = fp32((conv2 + b2) + cur).  ``dtype`` is the convs' accumulation type; ``bf16=False``
    switches the bf16 roundings off (the plain fp32 network).  ``spans`` (a list) receives,
    per conv, max(sum |w||x| + |b|) / (lowest bit a product can set): below 2**24 every
    partial sum is exact in fp32."""
    rnd = _bf16 if bf16 else (lambda t: t)
    cur = x.to(F32)
    for m in range(3):
        a = rnd(_lrelu(cur, 0.1))
        t = _conv(a, rnd(w1[m].to(F32)), k, dil[m], T, dtype, spans, b1[m]) + b1[m].to(F32)
        t = rnd(_lrelu(t, 0.1))
        c2 = _conv(t, rnd(w2[m].to(F32)), k, 1, T, dtype, spans, b2[m])
        cur = (c2 + b2[m].to(F32)) + cur
    v = cur
    if acc_in is not None:
        v = v + acc_in.to(F32)
    v = v * torch.tensor(scale, dtype=F32)
    hc = None
    if alpha2 is not None:
        hc = _lrelu(v, alpha2)
        hc = hc.to(torch.bfloat16) if bf16 else hc
    return v, hc


def pcm_of(wav_f32, max_wav):
    """fs2_vocoder_post's int16 rule: the fp32 product wav * max_wav, truncated toward zero to
    int32, of which the low 16 bits are kept (so +1.0 * 32768 wraps to -32768)."""
    p = np.asarray(wav_f32, dtype=np.float32) * np.float32(max_wav)
    assert p.dtype == np.float32
    i32 = np.trunc(p).astype(np.int32)
    low = i32 & np.int32(0xFFFF)
    return np.where(low >= 0x8000, low - 0x10000, low).astype(np.int16)


def conv_post(x, w, b, *, T, max_wav, lens=None):
    """conv_post (c_in -> 1, k = 7, zero padding per utterance of T rows) + tanh in fp64 on
    x (rows, c_in), w (1, c_in, 7), b (1,).  Returns (wav fp64 (rows,), pcm int16 of
    fp32(wav), mag): mag = sum |w * x| per sample, what the fp32 dot product's error bound
    scales with.  Rows t >= lens[b] are 0."""
    rows, c_in = x.shape
    xb = x.double().view(rows // T, T, c_in).transpose(1, 2)
    v = F.conv1d(xb, w.double(), b.double(), padding=3).reshape(rows)
    mag = F.conv1d(xb.abs(), w.double().abs(), None, padding=3).reshape(rows)
    wav = torch.tanh(v)
    if lens is not None:
        t = torch.arange(rows) % T
        keep = t < torch.as_tensor(lens, dtype=torch.int64).repeat_interleave(T)
        wav = torch.where(keep, wav, torch.zeros_like(wav))
    return wav, pcm_of(wav.to(F32).numpy(), max_wav), mag


def _wexp(C, k):
    """Exponent e of the lattice weights {0, 2**-e, 2**-(e+1)}: twice the channels, half the
    weights, so the sums keep their size (64 channels, k = 11 with e = 8 needed 24 bits)."""
    return 8 if C == 32 else 9


def lattice(C, k, seed, rows, wexp=None):
    """Exact-lattice ResBlock1 inputs, all non-negative (leaky ReLU is the identity inside the
    chain): x integers in [1, 8], weights per element from {0, 2**-e, 2**-(e+1)}, biases
    integers in {1, 2, 3}.  Returns (x (rows, C), w1, w2, b1, b2) as fp32 tensors."""
    g = torch.Generator().manual_seed(seed)
    e = _wexp(C, k) if wexp is None else wexp
    x = torch.randint(1, 9, (rows, C), generator=g).to(F32)
    vals = torch.tensor([0.0, 2.0 ** -e, 2.0 ** -(e + 1)], dtype=F32)
    W = lambda: [vals[torch.randint(0, 3, (C, C, k), generator=g)] for _ in range(3)]
    Bs = lambda: [torch.randint(1, 4, (C,), generator=g).to(F32) for _ in range(3)]
    w1, w2 = W(), W()
    b1, b2 = Bs(), Bs()
    return x, w1, w2, b1, b2


def tile_rows(C):
    """Rows per tile of fs2_resblock1_fused (R): 256 at 32 channels, 128 at 64."""
    return 256 if C == 32 else 128


def lattice_cases(n_cu=256):
    """Every (C, B, T, k, dilations) the GPU tests run on lattice inputs; ``n_cu`` (the
    device's compute units) sizes the persistent case at n_cu + 44 tiles."""
    cases = []
    for C, B, T in ((32, 2, 512), (64, 3, 256)):
        cases += [(C, B, T, k, (1, 3, 5)) for k in (3, 5, 7, 9, 11)]
    for C in (32, 64):
        R = tile_rows(C)
        cases += [(C, 2, 2 * R, 9, (1, 5, 7)), (C, 2, 2 * R, 3, (21, 20, 20)),
                  (C, 2, 2 * R, 5, (5, 1, 3)),   # radius
                  (C, 4, R, 11, (1, 3, 5)),      # one tile per utterance
                  (C, 2, 2 * R, 7, (1, 3, 5)),   # epilogue modes, three-way check
                  (C, 4, 4 * R, 7, (1, 3, 5)),   # lens
                  persistent_case(C, n_cu)]
    return cases


def persistent_case(C, n_cu):
    """n_cu + 44 tiles: utterances of four tiles when that divides, else of one."""
    R, tiles = tile_rows(C), n_cu + 44
    return (C, tiles // 4, 4 * R, 3, (1, 3, 5)) if tiles % 4 == 0 else (C, tiles, R, 3, (1, 3, 5))


def lattice_for(case):
    """The lattice inputs of one entry of ``lattice_cases`` (seeded by its shape)."""
    C, B, T, k, dil = case
    return lattice(C, k, 100 * C + 10 * k + dil[0], B * T)
