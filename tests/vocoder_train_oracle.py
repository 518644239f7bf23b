"""ORACLE -- TEST INFRASTRUCTURE ONLY.  Plain torch on the CPU, any float dtype: what the
vocoder's training kernels compute, with gradients by autograd.

* ``generator``: the HiFi-GAN generator exactly as hifigan/models.py:155-171 reads --
  ``conv1d`` / ``conv_transpose1d`` / ``leaky_relu`` 0.1, and 0.01 before ``conv_post`` / ``tanh``.
* ``mel``: a differentiable log-mel built from ``melspec_oracle``'s window, filterbank and the
  kernel's index rule (reflection against the row's own length, then the clamp).
* ``mel_l1``, ``adam_trajectory``: the loss and the trainer's Adam steps.
* ``conv_wgrad``, ``head``, ``lrelu_bwd``, ``phase_weight`` / ``fold``: the single kernels.

Every function takes ``dtype``: float64 is the oracle, float32 the same formulation as the
reference would run it on the CPU.  ``tol(f32, f64)`` = 4 x their largest difference, the factor
``melspec_oracle.bounds`` uses, is the tolerance the GPU tests allow.
"""
import numpy as np
import torch
import torch.nn.functional as F

import melspec_oracle as mo

FACTOR = 4.0
SLOPE = 0.1


def tol(f32, f64, factor=FACTOR):
    """factor x max |f32 - f64|: the fp32 CPU evaluation's own error on this input."""
    return factor * float((torch.as_tensor(f32).double() - torch.as_tensor(f64).double()).abs().max())


def get_padding(k, d=1):
    return int((k * d - d) / 2)


# ---------------------------------------------------------------------------- generator
def init_state(h, seed=0, scale=1.0):
    """A random folded state dict with the generator's keys and shapes (fp64), sized so that
    activations stay O(1) through the stack."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, c_out, c_in, k, fan=None):
        fan = fan or c_in * k
        sd[name + ".weight"] = torch.randn(c_out, c_in, k, generator=g, dtype=torch.float64) * scale / fan ** 0.5
        sd[name + ".bias"] = torch.randn(c_out, generator=g, dtype=torch.float64) * 0.1

    ch = h["upsample_initial_channel"]
    conv("conv_pre", ch, 80, 7)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        ci, co = ch // 2 ** i, ch // 2 ** (i + 1)
        sd[f"ups.{i}.weight"] = torch.randn(ci, co, k, generator=g, dtype=torch.float64) * scale / (ci * 2) ** 0.5
        sd[f"ups.{i}.bias"] = torch.randn(co, generator=g, dtype=torch.float64) * 0.1
    n = 0
    for i in range(len(h["upsample_rates"])):
        c = ch // 2 ** (i + 1)
        for k in h["resblock_kernel_sizes"]:
            for name in ("convs1", "convs2"):
                for m in range(3):
                    conv(f"resblocks.{n}.{name}.{m}", c, c, k, fan=4 * c * k)
            n += 1
    conv("conv_post", 1, ch // 2 ** len(h["upsample_rates"]), 7)
    return sd


def resblock(sd, n, k, dil, x):
    """ResBlock1 number ``n`` (hifigan/models.py:44-53) on x (B, C, T)."""
    for m, d in enumerate(dil):
        xt = F.leaky_relu(x, SLOPE)
        xt = F.conv1d(xt, sd[f"resblocks.{n}.convs1.{m}.weight"], sd[f"resblocks.{n}.convs1.{m}.bias"],
                      padding=get_padding(k, d), dilation=d)
        xt = F.leaky_relu(xt, SLOPE)
        xt = F.conv1d(xt, sd[f"resblocks.{n}.convs2.{m}.weight"], sd[f"resblocks.{n}.convs2.{m}.bias"],
                      padding=get_padding(k, 1))
        x = xt + x
    return x


def generator(sd, h, mel):
    """mel (B, 80, T) -> waveform (B, T * prod(upsample_rates)); dtype of ``mel``; ``sd`` tensors
    of that dtype (leaves that require grad receive the gradients)."""
    nk = len(h["resblock_kernel_sizes"])
    x = F.conv1d(mel, sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, SLOPE)
        x = F.conv_transpose1d(x, sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=u,
                               padding=(k - u) // 2)
        xs = None
        for j in range(nk):
            y = resblock(sd, i * nk + j, h["resblock_kernel_sizes"][j],
                         h["resblock_dilation_sizes"][j], x)
            xs = y if xs is None else xs + y
        x = xs / nk
    x = F.leaky_relu(x)  # 0.01
    x = F.conv1d(x, sd["conv_post.weight"], sd["conv_post.bias"], padding=3)
    return torch.tanh(x)[:, 0]


def generator_grads(sd64, h, mel64, cot64, dtype):
    """(wav, {name: grad}, d_mel) of <wav, cot> evaluated in ``dtype``."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd64.items()}
    mel = mel64.to(dtype).clone().requires_grad_(True)
    wav = generator(sd, h, mel)
    (wav * cot64.to(dtype)).sum().backward()
    return wav.detach(), {k: v.grad for k, v in sd.items()}, mel.grad


# ---------------------------------------------------------------------------- mel
def reflect_index(p, length):
    """fft.hpp's rule on an int array: reflected once at each end, then clamped."""
    p = np.abs(p)
    p = np.where(p > length - 1, 2 * (length - 1) - p, p)
    return np.clip(p, 0, length - 1)


def mel(wav, hop, length=None):
    """wav (S,) torch, differentiable -> log-mel (80, 1 + length // hop) of its first ``length``
    samples, in wav's dtype; zero gradient where filterbank . mag <= 1e-5."""
    length = int(wav.shape[0] if length is None else length)
    nf = mo.n_frames(length, hop)
    pos = np.arange(nf)[:, None] * hop - mo.N_FFT // 2 + np.arange(mo.N_FFT)[None, :]
    idx = torch.from_numpy(reflect_index(pos, length).astype(np.int64))
    dt = wav.dtype
    frames = wav[idx.reshape(-1)].reshape(nf, mo.N_FFT) * torch.from_numpy(mo.hann()).to(dt)
    mag = torch.fft.rfft(frames, dim=1).abs().transpose(0, 1)
    m = torch.from_numpy(mo.filterbank32()).to(dt) @ mag
    floor = torch.full_like(m, mo.CLAMP)
    return torch.log(torch.where(m > mo.CLAMP, m, floor))


def mel_batch(wav, hop, lens=None):
    """wav (B, S) -> (B, 80, 1 + S // hop), zeros past each row's frames."""
    B, S = wav.shape
    Fm = mo.n_frames(S, hop)
    out = []
    for b in range(B):
        m = mel(wav[b], hop, None if lens is None else lens[b])
        out.append(F.pad(m, (0, Fm - m.shape[1])))
    return torch.stack(out)


def mel_l1(a, b):
    return (a - b).abs().mean()


# ---------------------------------------------------------------------------- kernels
def conv_wgrad(dy, x, T, taps, pad, dil, dtype):
    """dy (rows, c_out), x (rows, c_in), utterances of T rows -> (dw (c_out, c_in, taps), db)
    as autograd gives them for conv1d(x, w, padding=pad, dilation=dil) in ``dtype``."""
    rows, c_in = x.shape
    c_out = dy.shape[1]
    xb = x.to(dtype).view(rows // T, T, c_in).transpose(1, 2)
    w = torch.zeros(c_out, c_in, taps, dtype=dtype, requires_grad=True)
    b = torch.zeros(c_out, dtype=dtype, requires_grad=True)
    y = F.conv1d(xb, w, b, padding=pad, dilation=dil)
    g = dy.to(dtype).view(rows // T, T, c_out).transpose(1, 2)
    (y * g).sum().backward()
    return w.grad, b.grad


def head(x, w, b, d_wav, T, dtype):
    """conv_post + tanh on x (rows, c_in): (wav, dx, dw (c_in * 7), db) in ``dtype``."""
    rows, c_in = x.shape
    xb = x.to(dtype).clone().requires_grad_(True)
    wv = w.to(dtype).clone().requires_grad_(True)
    bv = b.to(dtype).clone().requires_grad_(True)
    y = torch.tanh(F.conv1d(xb.view(rows // T, T, c_in).transpose(1, 2), wv.view(1, c_in, 7), bv,
                            padding=3)).reshape(rows)
    (y * d_wav.to(dtype)).sum().backward()
    return y.detach(), xb.grad, wv.grad.reshape(-1), bv.grad


def lrelu_bwd(v, dy, alpha, dtype):
    """dy * (v > 0 ? 1 : alpha), torch's convention at 0."""
    x = v.to(dtype).clone().requires_grad_(True)
    F.leaky_relu(x, alpha).backward(dy.to(dtype))
    return x.grad


def phase_weight(w, s):
    """fs2_convT_weight_prep's map: (c_in, c_out, 2 s) -> (s * c_out, c_in, 3)."""
    c_in, c_out, k = w.shape
    wc = w.new_zeros(s * c_out, c_in, 3)
    for ph in range(s):
        for d in (-1, 0, 1):
            tap = ph + s // 2 - s * d
            if 0 <= tap < k:
                wc[ph * c_out:(ph + 1) * c_out, :, d + 1] = w[:, :, tap].transpose(0, 1)
    return wc


def fold(dwc, dbc, c_in, c_out, s):
    """The inverse index map: (s * c_out, c_in, 3) -> (c_in, c_out, 2 s), bias summed over phases."""
    dw = dwc.new_zeros(c_in, c_out, 2 * s)
    for ph in range(s):
        for d in (-1, 0, 1):
            tap = ph + s // 2 - s * d
            if 0 <= tap < 2 * s:
                dw[:, :, tap] = dwc[ph * c_out:(ph + 1) * c_out, :, d + 1].transpose(0, 1)
    db = None
    if dbc is not None:
        db = dbc.new_zeros(c_out)
        for ph in range(s):
            db = db + dbc[ph * c_out:(ph + 1) * c_out]
    return dw, db


def phase_conv(x, wc, bc, s):
    """The 3-tap phase conv on x (B, c_in, T): (B, c_out, s T), what conv_transpose1d gives."""
    B, _, T = x.shape
    y = F.conv1d(x, wc, bc, padding=1)                     # (B, s * c_out, T)
    c_out = wc.shape[0] // s
    return y.view(B, s, c_out, T).permute(0, 2, 3, 1).reshape(B, c_out, T * s)


# ---------------------------------------------------------------------------- trainer
def adam_trajectory(sd64, h, segments, hop, steps, lr, betas, eps, dtype):
    """The trainer's steps on a fixed batch: segments (B, S) -> [loss_1 .. loss_steps] in
    ``dtype``.  Target: the segments' own mel; input: its first S // hop frames."""
    seg = segments.to(dtype)
    T = seg.shape[1] // hop
    with torch.no_grad():
        target = mel_batch(seg, hop)
    p = {k: v.to(dtype).clone() for k, v in sd64.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    losses = []
    for t in range(1, steps + 1):
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        wav = generator(leaves, h, target[:, :, :T])
        loss = mel_l1(mel_batch(wav, hop), target)
        loss.backward()
        losses.append(float(loss.detach()))
        for k in p:
            g = leaves[k].grad
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g
            v2[k] = betas[1] * v2[k] + (1 - betas[1]) * g * g
            den = v2[k].sqrt() / (1 - betas[1] ** t) ** 0.5 + eps
            p[k] = p[k] - lr / (1 - betas[0] ** t) * m[k] / den
    return losses
