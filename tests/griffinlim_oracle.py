"""Oracles of Griffin-Lim (fs2_istft, fs2_griffin_lim_step, fs2_mel_to_linear).  The reference
cannot run without librosa, so it is restated here from its sources (nothing is copied):

  common/stft.py:52-75, 107-137          STFT.inverse: conv_transpose of [mag cos, mag sin] with
      the windowed pinv(scale * fourier_basis).T, stride hop; divided by the float32 window
      sum-square where that exceeds tiny; times n_fft / hop; 512 samples trimmed at both ends
  common/stft.py:77-105                  STFT.transform, phase = atan2(imag, real)
  common/audio_processing.py:34-102      window_sumsquare; griffin_lim's loop
  common/layers.py:125-141               _mel_to_linear = clamp(pinverse(mel_basis) @ mel, 1e-10)

``oracle64`` is the definition in float64 (numpy rfft / irfft); ``ref32_conv`` is the reference's
own float32 formulation on the CPU and ``ref32_fft`` the same arithmetic through
torch.fft.rfft / irfft.  The GPU tests take their tolerance from the distance of those two from
``oracle64`` on the same inputs (``pooled_bound``).
"""
import numpy as np
import torch

import melspec_oracle as MO

N_FFT, BINS = MO.N_FFT, MO.BINS
HALF = N_FFT // 2
FRAMES = (4, 9, 12, 17)  # live frames of the ragged batch; frames = 17
HOPS = (256, 200)
_CACHE = {}


def n_samples(frames, hop):
    return hop * (frames - 1) if frames > 1 else 0


def stft64(x, hop):
    """The centred STFT (513, 1 + len // hop) in complex128."""
    x = np.asarray(x, np.float64)
    pad = np.pad(x, HALF, mode="reflect")
    nf = MO.n_frames(len(x), hop)
    frames = np.stack([pad[f * hop:f * hop + N_FFT] for f in range(nf)])
    return np.fft.rfft(frames * MO.hann()[None, :], axis=1).T


def window_sumsquare64(frames, hop):
    out = np.zeros(N_FFT + hop * (frames - 1))
    w2 = MO.hann() ** 2
    for f in range(frames):
        out[f * hop:f * hop + N_FFT] += w2
    return out


class oracle64:
    """The definitions in float64."""

    @staticmethod
    def stft(x, hop):
        return stft64(x, hop)

    @staticmethod
    def istft(mag, phase, hop):
        """mag, phase (513, F) -> (hop (F - 1),); phase None = zero.  A zero magnitude with any
        phase is a zero bin; bins 0 and 512 contribute their real parts only."""
        mag = np.asarray(mag, np.float64)
        spec = mag * np.exp(1j * (np.zeros_like(mag) if phase is None else np.asarray(phase, np.float64)))
        spec[0].imag = 0.0
        spec[BINS - 1].imag = 0.0
        F = mag.shape[1]
        fr = np.fft.irfft(spec.T, n=N_FFT, axis=1) * MO.hann()[None, :]
        y = np.zeros(N_FFT + hop * (F - 1))
        for f in range(F):
            y[f * hop:f * hop + N_FFT] += fr[f]
        keep = slice(HALF, HALF + n_samples(F, hop))
        return y[keep] / window_sumsquare64(F, hop)[keep]

    @staticmethod
    def gl_step(x, mag, hop):
        """One loop body: the phase of STFT(x) (0 at a zero bin, as atan2(0, 0)) under mag."""
        return oracle64.istft(mag, np.angle(stft64(x, hop)), hop)

    @staticmethod
    def griffin_lim(mag, angles, hop, iters):
        """{k: the waveform after k iterations} for the k in ``iters``."""
        x = oracle64.istft(mag, angles, hop)
        out = {0: x} if 0 in iters else {}
        for k in range(1, max(iters) + 1):
            x = oracle64.gl_step(x, mag, hop)
            if k in iters:
                out[k] = x
        return out

    @staticmethod
    def inv_basis():
        if "pinv64" not in _CACHE:
            _CACHE["pinv64"] = np.linalg.pinv(MO.filterbank32().astype(np.float64))
        return _CACHE["pinv64"]

    @staticmethod
    def mel_to_linear(logmel):
        return np.maximum(oracle64.inv_basis() @ np.exp(np.asarray(logmel, np.float64)), 1e-10)


def sc(x, mag, hop):
    """Spectral convergence ||abs(STFT(x)) - M||_F / ||M||_F in float64."""
    mag = np.asarray(mag, np.float64)
    return float(np.linalg.norm(np.abs(stft64(x, hop)) - mag) / np.linalg.norm(mag))


# ------------------------------------------------------------------ the fp32 formulations
def fourier_basis64():
    if "four" not in _CACHE:
        four = np.fft.fft(np.eye(N_FFT))[:BINS]
        _CACHE["four"] = np.vstack([four.real, four.imag])
    return _CACHE["four"]


def _win32():
    return torch.from_numpy(MO.hann().astype(np.float32))


def _window_sum32(frames, hop):
    """window_sumsquare with dtype float32: float64 squares added into a float32 array."""
    out = np.zeros(N_FFT + hop * (frames - 1), np.float32)
    w2 = MO.hann() ** 2
    for f in range(frames):
        out[f * hop:f * hop + N_FFT] += w2
    return out


def _normalise32(y, frames, hop):
    """stft.py:118-135 on y (n_fft + hop (F - 1),) float32."""
    ws = _window_sum32(frames, hop)
    idx = torch.from_numpy(np.where(ws > np.finfo(np.float32).tiny)[0])
    y = y.clone()
    y[idx] = y[idx] / torch.from_numpy(ws)[idx]
    y = y * (float(N_FFT) / hop)
    return y[HALF:-HALF]


def _pad32(x):
    x = torch.from_numpy(np.asarray(x, np.float32))[None, None, :]
    return torch.nn.functional.pad(x.unsqueeze(1), (HALF, HALF, 0, 0), mode="reflect").squeeze(1)


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))


class _Ref32:
    @classmethod
    def gl_step(cls, x, mag, hop):
        _, phase = cls.transform(x, hop)
        return cls.istft(mag, phase, hop)

    @classmethod
    def griffin_lim(cls, mag, angles, hop, iters):
        x = cls.istft(mag, angles, hop)
        out = {0: x} if 0 in iters else {}
        for k in range(1, max(iters) + 1):
            x = cls.gl_step(x, mag, hop)
            if k in iters:
                out[k] = x
        return out

    @staticmethod
    def mel_to_linear(logmel):
        """layers.py:125-134: exp, torch.pinverse in fp32, matmul, clamp."""
        inv = torch.pinverse(torch.from_numpy(MO.filterbank32()))
        return torch.clamp(torch.matmul(inv, torch.exp(_t32(logmel))), min=1e-10).numpy()


class ref32_conv(_Ref32):
    """The reference's own: conv1d / conv_transpose2d with the windowed bases."""

    @staticmethod
    def bases(hop):
        if ("bases", hop) not in _CACHE:
            four = fourier_basis64()
            fwd = torch.from_numpy(four[:, None, :].astype(np.float32)) * _win32()
            inv = np.linalg.pinv((N_FFT / hop) * four).T[:, None, :].astype(np.float32)
            _CACHE["bases", hop] = (fwd, torch.from_numpy(inv) * _win32())
        return _CACHE["bases", hop]

    @staticmethod
    def transform(x, hop):
        ft = torch.nn.functional.conv1d(_pad32(x), ref32_conv.bases(hop)[0], stride=hop)[0]
        re, im = ft[:BINS], ft[BINS:]
        return torch.sqrt(re ** 2 + im ** 2).numpy(), torch.atan2(im, re).numpy()

    @staticmethod
    def istft(mag, phase, hop):
        mag = _t32(mag)
        phase = torch.zeros_like(mag) if phase is None else _t32(phase)
        rec = torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], dim=0)[None]
        y = torch.nn.functional.conv_transpose2d(rec.unsqueeze(-1),
                                                 ref32_conv.bases(hop)[1].unsqueeze(-1),
                                                 stride=(hop, 1), padding=(0, 0)).squeeze(-1)[0, 0]
        return _normalise32(y, mag.shape[1], hop).numpy()


class ref32_fft(_Ref32):
    """The same arithmetic through torch.fft.rfft / irfft in float32."""

    @staticmethod
    def transform(x, hop):
        fr = _pad32(x)[0, 0].unfold(0, N_FFT, hop) * _win32()
        ft = torch.fft.rfft(fr, dim=1).T
        return torch.sqrt(ft.real ** 2 + ft.imag ** 2).numpy(), torch.atan2(ft.imag, ft.real).numpy()

    @staticmethod
    def istft(mag, phase, hop):
        mag = _t32(mag)
        phase = torch.zeros_like(mag) if phase is None else _t32(phase)
        re, im = mag * torch.cos(phase), mag * torch.sin(phase)
        im[0] = im[BINS - 1] = 0.0  # the reference's real basis takes none from bins 0 and 512
        spec = torch.complex(re, im)
        F = mag.shape[1]
        fr = torch.fft.irfft(spec.T.contiguous(), n=N_FFT, dim=1) * _win32()
        y = torch.zeros(N_FFT + hop * (F - 1), dtype=torch.float32)
        for f in range(F):
            y[f * hop:f * hop + N_FFT] += fr[f]
        # the hop / n_fft of the pinv basis and the later n_fft / hop, in the reference's order
        return _normalise32(y * (float(hop) / N_FFT), F, hop).numpy()


REFS = (ref32_conv, ref32_fft)


def pooled_bound(pairs, factor=4.0):
    """factor x the largest |ref32 - oracle64| over ``pairs`` of (fp32 result, float64 result):
    both formulations, every row and every iteration count of a test go into one pool."""
    dev = max(float(np.abs(np.asarray(r, np.float64) - w).max()) for r, w in pairs if np.size(w))
    return factor * dev


# ------------------------------------------------------------------ the shared inputs
def batch(hop):
    """The ragged batch of the GPU tests, computed once: per row the signal ``x``, its float64
    STFT ``X``, ``M = |X|`` and the initial ``angles``; ``mag`` / ``phase`` (4, 513, 17) float32
    with noise in the dead frames."""
    if ("batch", hop) in _CACHE:
        return _CACHE["batch", hop]
    frames = max(FRAMES)
    rng = np.random.default_rng(hop)
    mag = np.abs(rng.standard_normal((len(FRAMES), BINS, frames))).astype(np.float32)
    phase = rng.standard_normal((len(FRAMES), BINS, frames)).astype(np.float32)
    rows = []
    for b, F in enumerate(FRAMES):
        x = MO.fixture(hop * (F - 1), 100 + F)
        X = stft64(x, hop)
        assert X.shape == (BINS, F)
        M = np.abs(X).astype(np.float32)
        ang = np.angle(np.exp(2j * np.pi * np.random.default_rng(F).random(M.shape))).astype(np.float32)
        mag[b, :, :F], phase[b, :, :F] = M, ang
        rows.append({"F": F, "x": x, "X": X, "M": M, "angles": ang})
    out = {"rows": rows, "mag": mag, "phase": phase, "n_frames": np.asarray(FRAMES, np.int64),
           "frames": frames, "samples": hop * (frames - 1)}
    _CACHE["batch", hop] = out
    return out


def loop_results(hop, iters):
    """(want, refs): per row ``{k: oracle64 waveform}`` and, per formulation, the same of
    ref32 -- Griffin-Lim from (M, angles), computed once per (hop, iters)."""
    key = ("loop", hop, tuple(iters))
    if key not in _CACHE:
        rows = batch(hop)["rows"]
        want = [oracle64.griffin_lim(r["M"], r["angles"], hop, iters) for r in rows]
        refs = [[R.griffin_lim(r["M"], r["angles"], hop, iters) for r in rows] for R in REFS]
        _CACHE[key] = (want, refs)
    return _CACHE[key]


def loop_bound(hop, iters):
    want, refs = loop_results(hop, iters)
    return pooled_bound([(ref[b][k], want[b][k]) for ref in refs for b in range(len(want))
                         for k in iters])


def logmels(hop):
    """Log-mels of the batch's signals from oracle64: (4, 80, 17) float32, noise in dead frames."""
    if ("logmel", hop) not in _CACHE:
        bt = batch(hop)
        mel = np.random.default_rng(7).standard_normal((len(FRAMES), MO.N_MELS, bt["frames"]))
        mel = mel.astype(np.float32)
        for b, r in enumerate(bt["rows"]):
            mel[b, :, :r["F"]] = MO.oracle64(r["x"], hop)[1].astype(np.float32)
        _CACHE["logmel", hop] = mel
    return _CACHE["logmel", hop]


def edge_cases():
    """F = 6: (name, mag (513, 6), phase (513, 6)) float32 -- bin 0 only, bin 512 only, bin 256
    only with phases at bins 0 and 512 that must be ignored; and, beyond those three, bins 0 and
    512 both live under non-zero phases, of which only the real parts count."""
    rng = np.random.default_rng(11)
    both = np.zeros((BINS, 6), np.float32), np.zeros((BINS, 6), np.float32)
    both[0][0], both[0][BINS - 1] = 0.7, 0.4
    both[1][0], both[1][BINS - 1] = 1.0, 2.0
    out = [("real_parts",) + both]
    for name, k in (("bin0", 0), ("bin512", BINS - 1), ("bin256", 256)):
        mag = np.zeros((BINS, 6), np.float32)
        mag[k] = (0.5 + rng.random(6)).astype(np.float32)
        phase = np.zeros((BINS, 6), np.float32)
        if k == 256:
            phase[256] = rng.uniform(-3.0, 3.0, 6).astype(np.float32)
            phase[0] = phase[BINS - 1] = 1.0
        out.append((name, mag, phase))
    return out
