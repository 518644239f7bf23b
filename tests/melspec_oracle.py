"""Oracles of the mel front end.  Neither reference front end can run without librosa /
torchaudio, so both are restated here from their sources (nothing is copied):

  preprocessor/preprocessor.py:44-59, 330-336   torchaudio Spectrogram(power=1, center=True) ->
      MelScale(norm="slaney", mel_scale="slaney") -> log(clamp_min(., 1e-5)); energy =
      torch.norm(magspec, dim=0); the audio clipped to [-1, 1] first
  common/stft.py:53-101                         STFT.transform: reflect pad of n_fft / 2, conv1d of
      stride hop with the windowed Fourier basis (rows of np.fft.fft(np.eye(n_fft)), real parts
      then imaginary parts of bins 0..n_fft/2), magnitude sqrt(re^2 + im^2)
  common/layers.py:81-83, 101-123               mel_basis = librosa.filters.mel(sr, n_fft, n_mels,
      fmin, fmax); mel = log(clamp(mel_basis @ mag, 1e-5))

``oracle64`` is the definition in float64 (numpy rfft); ``ref32`` is the reference's own float32
formulation on the CPU.  Their difference on an input is the reference's own rounding error there,
which is what the GPU tests scale their tolerance from.
"""
import numpy as np
import torch

SR, N_FFT, N_MELS, FMIN, FMAX = 22050, 1024, 80, 0.0, 8000.0
BINS = N_FFT // 2 + 1
CLAMP = 1e-5


def hann():
    """scipy.signal.get_window("hann", 1024, fftbins=True): the periodic Hann window."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)


def slaney_filterbank(sr=SR, n_fft=N_FFT, n_mels=N_MELS, fmin=FMIN, fmax=FMAX):
    """librosa.filters.mel (htk=False, norm="slaney") one triangle at a time, in float64."""
    step, knee, knee_mel, logstep = 200.0 / 3.0, 1000.0, 15.0, np.log(6.4) / 27.0

    def to_mel(f):
        return f / step if f < knee else knee_mel + np.log(f / knee) / logstep

    def to_hz(m):
        return m * step if m < knee_mel else knee * np.exp(logstep * (m - knee_mel))

    lo, hi = to_mel(fmin), to_mel(fmax)
    edges = [to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    out = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        left, centre, right = edges[m], edges[m + 1], edges[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * (sr / 2.0) / (n_fft // 2)
            tri = min((f - left) / (centre - left), (right - f) / (right - centre))
            out[m, k] = max(0.0, tri) * 2.0 / (right - left)
    return out


_FB = {}


def filterbank32():
    if "fb" not in _FB:
        _FB["fb"] = slaney_filterbank().astype(np.float32)
    return _FB["fb"]


def n_frames(length, hop):
    return 1 + length // hop


def oracle64(x, hop):
    """x (len,) -> mag (513, F), logmel (80, F), energy (F,) in float64; the float32-rounded
    filterbank applied in float64."""
    x = np.asarray(x, np.float64)
    pad = np.pad(x, N_FFT // 2, mode="reflect")
    nf = n_frames(len(x), hop)
    frames = np.stack([pad[f * hop:f * hop + N_FFT] for f in range(nf)])
    mag = np.abs(np.fft.rfft(frames * hann()[None, :], axis=1)).T
    mel = filterbank32().astype(np.float64) @ mag
    return mag, np.log(np.maximum(mel, CLAMP)), np.sqrt((mag * mag).sum(0))


def _basis32():
    if "basis" not in _FB:
        four = np.fft.fft(np.eye(N_FFT))[:BINS]
        basis = np.vstack([four.real, four.imag]).astype(np.float32) * hann().astype(np.float32)[None, :]
        _FB["basis"] = torch.from_numpy(basis[:, None, :])
    return _FB["basis"]


def ref32(x, hop):
    """The reference's formulation in float32 on the CPU: conv1d STFT, sqrt(re^2 + im^2),
    torch.matmul(mel_basis, mag), log(clamp(., 1e-5)), torch.norm(mag, dim=0)."""
    x = torch.from_numpy(np.asarray(x, np.float32))[None, None, :]
    pad = torch.nn.functional.pad(x.unsqueeze(1), (N_FFT // 2, N_FFT // 2, 0, 0),
                                  mode="reflect").squeeze(1)
    ft = torch.nn.functional.conv1d(pad, _basis32(), stride=hop)[0]
    mag = torch.sqrt(ft[:BINS] ** 2 + ft[BINS:] ** 2)
    mel = torch.log(torch.clamp(torch.matmul(torch.from_numpy(filterbank32()), mag), min=CLAMP))
    return mag.numpy(), mel.numpy(), torch.norm(mag, dim=0).numpy()


def bounds(x, hop, factor=4.0):
    """(oracle64 triple, per-output tolerance): factor x max|ref32 - oracle64| on this input."""
    want = oracle64(x, hop)
    ref = ref32(x, hop)
    return want, tuple(factor * float(np.abs(r - w).max()) for r, w in zip(ref, want))


def fixture(length, seed, kind="speech"):
    """A structured part plus white noise of standard deviation 1e-2 (which keeps every mel value
    well above the clamp), clipped to [-1, 1]; float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(length, dtype=np.float64)
    noise = 1e-2 * rng.standard_normal(length)
    if kind == "speech":  # a few harmonics with a slow envelope and a chirp
        f0 = 110.0 + 40.0 * rng.random()
        x = sum(0.3 / h * np.sin(2 * np.pi * h * f0 * t / SR + rng.random()) for h in (1, 2, 3, 5, 8))
        x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t / SR))
        x = x + 0.1 * np.sin(2 * np.pi * (500.0 + 2000.0 * t / max(length, 1)) * t / SR)
    elif kind == "dc":
        x = np.full(length, 0.5)
    elif kind == "nyquist":
        x = 0.5 * (-1.0) ** np.arange(length)
    elif kind == "impulse":
        x = np.zeros(length)
        x[700] = 0.9
    elif kind == "tone7600":
        x = 0.5 * np.sin(2 * np.pi * 7600.0 * t / SR)
    else:
        raise ValueError(kind)
    return np.clip(x + noise, -1.0, 1.0).astype(np.float32)
