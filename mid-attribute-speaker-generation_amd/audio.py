"""The mel front end: waveform -> log-mel spectrogram, frame energy, linear spectrogram.

One kernel (``fs2_melspec``) serves the three places the reference computes them:

  preprocessor/preprocessor.py:330-336   ``calc_spectrogram`` (torchaudio Spectrogram + MelScale;
                                         clip to [-1, 1], log-mel and the L2 frame energy)
  common/layers.py:101-123               ``TacotronSTFT.mel_spectrogram`` / ``linear_spectrogram``
                                         of the speaker encoder (librosa filterbank, conv STFT)
  train_speech_embedder.py:27-81         ``generate_dvector``'s mel of a wav
                                         (``EmbedderTrainer.dvector_from_wav``)

They are the same arithmetic: periodic Hann window of 1024, hop 256, centred frames with reflect
padding of 512, the magnitude of the 513 bins, the Slaney mel filterbank (80 filters, 0-8000 Hz at
22 050 Hz, area normalised) and ``log(clamp(., 1e-5))``.  Everything on the host here is table
construction (fp64, rounded to fp32); the arithmetic on samples runs in the kernel.

``GriffinLim`` is the way back (``TacotronSTFT.inv_mel_spectrogram`` / ``inv_linear_spectrogram``,
common/layers.py:125-141): mel inversion, inverse STFT and the Griffin-Lim loop on the same
tables, and a ``forward_rows`` that stands in for the vocoder where no checkpoint exists.

Beside it: ``PitchExtractor`` (YIN or pYIN F0 on the same frames), ``SilenceSplitter``
(``librosa.effects.split``, the speaker encoder's data_preprocess.py:46) and ``Resampler``
(``librosa.load``'s rate conversion).
"""
import math

import numpy as np
import torch

from . import kernels as K
from .config import load_configs

N_FFT = 1024  # compiled into the kernel (n_fft = win_length)
N_BINS = N_FFT // 2 + 1


def _hz_to_mel(f):
    """Slaney's scale: 200/3 Hz per mel below 1 kHz, ln(6.4)/27 per mel above."""
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3.0))


def mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """The Slaney filterbank (n_mels, n_fft // 2 + 1) that ``librosa.filters.mel`` (defaults:
    ``htk=False``, area norm) and ``torchaudio.transforms.MelScale(norm="slaney",
    mel_scale="slaney")`` both build: triangles between consecutive mel points over
    ``linspace(0, sr / 2, n_fft // 2 + 1)``, each scaled by ``2 / (f[m + 2] - f[m])``; fp64,
    rounded to fp32."""
    freqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    diff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower = -ramps[:-2] / diff[:-1, None]
    upper = ramps[2:] / diff[1:, None]
    fb = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]
    return fb.astype(np.float32)


def compress_filterbank(dense):
    """A dense (n_mels, bins) matrix as ``(first, count, offset, weights)``: filter ``c`` weighs
    bins ``first[c] .. first[c] + count[c] - 1`` (its first to its last non-zero column) with
    ``weights[offset[c]:offset[c] + count[c]]``.  int32 x 3 and float32; an all-zero row has
    count 0."""
    dense = np.asarray(dense, np.float32)
    first, count, off, w = [], [], [], []
    for row in dense:
        nz = np.flatnonzero(row)
        lo, n = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        first.append(lo)
        count.append(n)
        off.append(sum(count[:-1]))
        w.append(row[lo:lo + n])
    weights = np.concatenate(w) if w else np.zeros(0, np.float32)
    return (np.asarray(first, np.int32), np.asarray(count, np.int32), np.asarray(off, np.int32),
            weights.astype(np.float32))


def expand_filterbank(first, count, off, weights, bins=N_BINS):
    """The dense matrix of a compressed filterbank (the inverse of ``compress_filterbank``)."""
    dense = np.zeros((len(first), bins), np.float32)
    for c, (lo, n, o) in enumerate(zip(first, count, off)):
        dense[c, lo:lo + n] = weights[o:o + n]
    return dense


def twiddle_table():
    """(1024, 2) float32: cos and -sin of 2 pi k / 1024, computed in fp64."""
    ang = 2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT
    return np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)


def frame_count(length, hop):
    """Frames of a centred STFT over ``length`` samples: ``1 + length // hop``."""
    return 1 + int(length) // int(hop)


class MelFrontEnd:
    """The front end with the parameters of ``preprocess.yaml`` (the speaker encoder's
    ``config.yaml`` has the same values).  Tables are built on the host at construction and go to
    ``device`` at the first call."""

    def __init__(self, preprocess_config=None, device="cuda"):
        from scipy.signal import get_window
        pp = preprocess_config if preprocess_config is not None else load_configs()[0]
        stft, mel = pp["stft"], pp.get("mel", {})
        n_fft, win = int(stft["filter_length"]), int(stft.get("win_length", stft["filter_length"]))
        if n_fft != N_FFT or win != N_FFT:
            raise ValueError(f"filter_length {n_fft}, win_length {win}: the kernel is built for "
                             f"n_fft = win_length = {N_FFT}")
        self.hop = int(stft["hop_length"])
        if not 1 <= self.hop <= N_FFT:
            raise ValueError(f"hop_length {self.hop} (1..{N_FFT})")
        self.sr = int(pp["audio"]["sampling_rate"])
        self.n_mels = int(mel.get("n_mel_channels", 80))
        self.fmin, self.fmax = float(mel.get("mel_fmin", 0.0)), float(mel.get("mel_fmax", 8000.0))
        self.device = torch.device(device)
        self.window = get_window("hann", N_FFT, fftbins=True).astype(np.float32)
        self.mel_basis = mel_filterbank(self.sr, N_FFT, self.n_mels, self.fmin, self.fmax)
        self._tables = None

    def _dev_tables(self):
        if self._tables is None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
            self._tables = (up(self.window), up(twiddle_table()),
                            tuple(up(a) for a in compress_filterbank(self.mel_basis)))
        return self._tables

    def check_lens(self, lens, samples):
        """The reflect-pad condition torch enforces, for host lengths: ``512 < len <= S``."""
        for n in lens:
            if not N_FFT // 2 < int(n) <= int(samples):
                raise ValueError(f"length {int(n)}: reflect padding of {N_FFT // 2} needs "
                                 f"{N_FFT // 2} < len <= {int(samples)} samples")

    def n_frames(self, length):
        return frame_count(length, self.hop)

    def __call__(self, wav, lens=None, clip=False, mag=False, log_mag=False):
        """wav (B, S) or (S,) on the device -> ``(logmel (B, n_mels, F), energy (B, F),
        n_frames (B) int64[, mag (B, 513, F)])``, F = 1 + S // hop, zeros past ``n_frames``
        (without the batch axis for a 1-D wav).  ``lens``: None (S for every row), a list
        (checked on the host) or a device int64 tensor (not read back)."""
        single = wav.dim() == 1
        w = (wav[None] if single else wav).contiguous()
        if w.dtype != torch.float32:
            w = w.float()
        B, S = w.shape
        if lens is None:
            self.check_lens([S], S)
        elif not torch.is_tensor(lens):
            lens = [int(n) for n in lens]
            if len(lens) != B:
                raise ValueError(f"{len(lens)} lengths for {B} rows")
            self.check_lens(lens, S)
            lens = torch.from_numpy(np.asarray(lens, np.int64)).pin_memory().to(w.device,
                                                                                 non_blocking=True)
        window, twiddle, fb = self._dev_tables()
        mel_o, en_o, mag_o, nf = K.melspec(w, lens, self.hop, window, twiddle, fb, self.n_mels,
                                           clip=clip, energy=True, mag=mag or log_mag,
                                           log_mag=log_mag)
        out = (mel_o, en_o, nf) + ((mag_o,) if mag or log_mag else ())
        return tuple(o[0] for o in out) if single else out

    def calc_spectrogram(self, audio):
        """``Preprocessor.calc_spectrogram`` (preprocessor.py:330-336): a numpy waveform ->
        numpy ``(n_mels, F)`` float32 log-mel and ``(F,)`` float32 energy, samples clipped to
        [-1, 1]."""
        wav = torch.from_numpy(np.ascontiguousarray(audio, np.float32)).to(self.device)
        mel, energy, _ = self(wav, clip=True)
        return mel.cpu().numpy(), energy.cpu().numpy()

    def mel_spectrogram(self, y):
        """``TacotronSTFT.mel_spectrogram`` (layers.py:101-118): y (B, T) in [-1, 1] ->
        (B, n_mels, F).  The reference's range asserts (two host reads) are not made."""
        return self(y)[0]

    def linear_spectrogram(self, y):
        """``TacotronSTFT.linear_spectrogram`` (layers.py:120-123): (B, T) -> (B, 513, F),
        ``log(clamp(|STFT|, 1e-5))``."""
        return self(y, log_mag=True)[3]


def inverse_mel_basis(fb_dense):
    """The (bins, n_mels) pseudo-inverse of a float32 filterbank (n_mels, bins), computed in
    float64 and rounded once to float32.  ``TacotronSTFT._mel_to_linear`` (layers.py:125-131)
    calls ``torch.pinverse`` in fp32 on every call; this is built once per ``GriffinLim``.  The
    rows of the bins no filter reaches (above ``fmax``) are zero."""
    fb = np.asarray(fb_dense, np.float32)
    return np.ascontiguousarray(np.linalg.pinv(fb.astype(np.float64)).astype(np.float32))


class GriffinLim:
    """Audio without a vocoder checkpoint: ``TacotronSTFT.inv_mel_spectrogram`` /
    ``inv_linear_spectrogram`` (layers.py:125-141) over ``griffin_lim``
    (audio_processing.py:86-102) and ``STFT.inverse`` (stft.py:107-137), on the kernels
    ``fs2_mel_to_linear``, ``fs2_istft`` and ``fs2_griffin_lim_step``.  The window, twiddle and
    filterbank tables are those of a ``MelFrontEnd`` (``front_end``, or one built from
    ``preprocess_config``).  ``128 <= hop_length <= 512``.

    Ragged batches: ``n_frames`` is None (every frame), a host list or a device int64 tensor
    (not read back).  A row of ``F`` frames gives ``hop (F - 1)`` samples -- the signal whose
    centred STFT has ``F`` frames -- and zeros after them.

    The initial phase is drawn on the device from ``generator`` (``self.generator`` when none is
    passed; None = torch's default stream).  The reference draws it from numpy's global stream;
    no parity with that stream is claimed.  ``forward_rows`` makes an instance a drop-in for the
    vocoder argument of ``synthesize.synth_batch`` / ``synthesize`` / ``synth_dvectors``."""

    def __init__(self, preprocess_config=None, device="cuda", n_iters=60, front_end=None):
        self.front = front_end if front_end is not None else MelFrontEnd(preprocess_config, device)
        self.hop, self.n_mels, self.device = self.front.hop, self.front.n_mels, self.front.device
        if not 128 <= self.hop <= 512:
            raise ValueError(f"hop_length {self.hop}: the inverse is built for 128..512")
        self.n_iters = int(n_iters)
        self.inv_mel_basis = inverse_mel_basis(self.front.mel_basis)
        self.generator = None
        self._inv = None

    def _tables(self):
        window, twiddle, _ = self.front._dev_tables()
        if self._inv is None:
            self._inv = torch.from_numpy(self.inv_mel_basis).to(self.device)
        return window, twiddle, self._inv

    def _spec(self, x, name):
        if x.dim() != 3:
            raise ValueError(f"{name} is (B, channels, frames)")
        x = x.contiguous()
        return x if x.dtype == torch.float32 else x.float()

    def _counts(self, n_frames, B, F):
        if n_frames is None:
            return None
        if torch.is_tensor(n_frames):
            if n_frames.numel() != B:
                raise ValueError(f"{n_frames.numel()} frame counts for {B} rows")
            return n_frames.to(device=self.device, dtype=torch.int64).reshape(B).contiguous()
        n = [int(v) for v in n_frames]
        if len(n) != B or min(n) < 0 or max(n) > F:
            raise ValueError(f"n_frames must be {B} frame counts in [0, {F}]")
        return torch.from_numpy(np.asarray(n, np.int64)).pin_memory().to(self.device,
                                                                          non_blocking=True)

    def inverse(self, magnitude, phase=None, n_frames=None):
        """``STFT.inverse``: magnitude, phase (None = zero) (B, 513, F) -> wav (B, hop (F - 1))."""
        mag = self._spec(magnitude, "magnitude")
        window, twiddle, _ = self._tables()
        return K.istft(mag, None if phase is None else self._spec(phase, "phase"),
                       self._counts(n_frames, mag.shape[0], mag.shape[2]), self.hop, window, twiddle)

    def mel_to_linear(self, mel, n_frames=None):
        """``_mel_to_linear`` of LOG-mels (B, n_mels, F): ``max(pinv(mel_basis) @ exp(mel),
        1e-10)`` (B, 513, F)."""
        mel = self._spec(mel, "mel")
        return K.mel_to_linear(mel, self._counts(n_frames, mel.shape[0], mel.shape[2]),
                               self._tables()[2])

    def griffin_lim(self, magnitudes, n_iters=None, angles=None, n_frames=None, generator=None):
        """``griffin_lim``: the inverse of ``magnitudes`` (B, 513, F) under ``angles`` (drawn
        uniform in (-pi, pi] when None; given angles make the result deterministic), then
        ``n_iters`` passes of transform / keep the phase / invert, two waveform buffers taking
        turns and one frame workspace: ``2 (n_iters + 1)`` launches, nothing allocated between."""
        mag = self._spec(magnitudes, "magnitudes")
        B, _, F = mag.shape
        n_iters = self.n_iters if n_iters is None else int(n_iters)
        nf = self._counts(n_frames, B, F)
        window, twiddle, _ = self._tables()
        if angles is None:
            gen = generator if generator is not None else self.generator
            u = torch.rand(mag.shape, dtype=torch.float32, device=mag.device, generator=gen)
            angles = float(np.pi) - (2.0 * float(np.pi)) * u
        scratch = K.griffin_lim_ws(B, F, mag.device)
        cur = K.istft(mag, self._spec(angles, "angles"), nf, self.hop, window, twiddle,
                      ws_buf=scratch)
        nxt = torch.empty_like(cur) if n_iters > 0 else None
        for _ in range(n_iters):
            K.griffin_lim_step(cur, mag, nf, self.hop, window, twiddle, out=nxt, ws_buf=scratch)
            cur, nxt = nxt, cur
        return cur

    def inv_mel_spectrogram(self, mel, iter_=60, n_frames=None, generator=None, angles=None):
        """``TacotronSTFT.inv_mel_spectrogram``: log-mel (B, n_mels, F) -> wav."""
        return self.griffin_lim(self.mel_to_linear(mel, n_frames), iter_, angles, n_frames, generator)

    def inv_linear_spectrogram(self, spec, iter_=60, n_frames=None, generator=None, angles=None):
        """``TacotronSTFT.inv_linear_spectrogram``: log-magnitude (B, 513, F) -> wav."""
        return self.griffin_lim(torch.exp(self._spec(spec, "spec")), iter_, angles, n_frames,
                                generator)

    @torch.no_grad()
    def forward_rows(self, mel_rows, B, T, pcm=True, max_wav_value=32768.0, lengths=None):
        """The contract of ``hifigan.Generator.forward_rows``: mel_rows (B*T, n_mels) (the
        FastSpeech2 row layout) -> ``(wav (B*T*hop,) fp32, pcm int16 or None)``, ``lengths`` = mel
        frames per utterance (a list or a device tensor such as the model's mel_len), ``n_iters``
        passes.  Griffin-Lim yields ``hop (len - 1)`` samples: the last hop of each utterance
        and everything after it is zeros.  int16 as ``fs2_vocoder_post`` converts: the product
        with ``max_wav_value`` truncated toward zero, the low 16 bits kept."""
        B, T = int(B), int(T)
        mel = mel_rows.reshape(B, T, -1).transpose(1, 2)
        live = self.inv_mel_spectrogram(mel, self.n_iters, n_frames=lengths)
        wav = torch.zeros((B, T * self.hop), dtype=torch.float32, device=live.device)
        wav[:, :live.shape[1]] = live
        wav = wav.view(-1)
        return wav, (wav * float(max_wav_value)).to(torch.int32).to(torch.int16) if pcm else None


PYIN_THRESHOLDS, PYIN_BINS_PER_SEMITONE, PYIN_MAX_BINS = 100, 5, 1024


def pyin_tables(hop, sr, f0_floor=71.0, f0_ceil=800.0):
    """The host tables of ``fs2_f0_pyin`` as numpy arrays ``(prior f64 (100), tri f64 (R + 1),
    centres f32 (n_bins))``, Python floats throughout so that any host computes the same bits:

      prior[i - 1] = I(theta_i) - I(theta_(i-1)), theta_i = float32(i / 100), theta_0 = 0, I the
                     Beta(2, 18) CDF 1 - (1 - x)^19 - 19 x (1 - x)^18
      tri[d]       = (R + 1 - d) / (R + 1)^2, R = round(35.92 * 60 * hop / sr): the widest jump
                     between two frames, 35.92 octaves per second
      centres[b]   = float32(f0_floor 2^(b / 60)), n_bins = floor(60 log2(f0_ceil / f0_floor)) + 1
    """
    step = 12 * PYIN_BINS_PER_SEMITONE

    def cdf(x):
        return 1.0 - (1.0 - x) ** 19 - 19.0 * x * (1.0 - x) ** 18

    th = [0.0] + [float(np.float32(i / 100.0)) for i in range(1, PYIN_THRESHOLDS + 1)]
    prior = np.array([cdf(th[i]) - cdf(th[i - 1]) for i in range(1, PYIN_THRESHOLDS + 1)])
    R = int(round(35.92 * step * hop / sr))
    tri = np.array([(R + 1 - d) / float((R + 1) ** 2) for d in range(R + 1)])
    n_bins = int(math.floor(step * math.log2(f0_ceil / f0_floor))) + 1
    centres = np.array([f0_floor * 2.0 ** (b / float(step)) for b in range(n_bins)]).astype(np.float32)
    return prior, tri, centres


class PitchExtractor:
    """The F0 contour on the frames of ``MelFrontEnd`` (centres ``k * hop``, ``1 + len // hop`` of
    them: the count ``pw.dio`` returns for ``frame_period = hop / sr``), by YIN
    (``fs2_f0_yin``).  The reference (preprocessor.py:196-201) calls pyworld's DIO + StoneMask;
    this is another estimator and its values are not DIO's.  ``dip`` is the normalised
    difference function at the chosen lag (its minimum over the lag range for an unvoiced
    frame): small means strongly periodic.

    ``method="pyin"`` is pYIN (``fs2_f0_pyin``; Mauch & Dixon 2014): every threshold of a
    Beta(2, 18) prior votes for YIN's pick at it and a Viterbi pass over (pitch bin, voiced /
    unvoiced) states picks the track, which keeps the voicing decision steady in noise.
    ``threshold`` is ignored by it, and the second result is ``unvoiced``, 1 - the voiced prior
    mass of the frame, in ``dip``'s place and sense."""

    METHODS = ("yin", "pyin")

    def __init__(self, preprocess_config=None, device="cuda", f0_floor=71.0, f0_ceil=800.0,
                 threshold=0.15, method="yin"):
        if method not in self.METHODS:
            raise ValueError(f"method {method!r}: one of {list(self.METHODS)}")
        self.method = method
        pp = preprocess_config if preprocess_config is not None else load_configs()[0]
        self.hop = int(pp["stft"]["hop_length"])
        self.sr = int(pp["audio"]["sampling_rate"])
        self.f0_floor, self.f0_ceil, self.threshold = float(f0_floor), float(f0_ceil), float(threshold)
        if not 1 <= self.hop <= N_FFT:
            raise ValueError(f"hop_length {self.hop} (1..{N_FFT})")
        if not 0.0 < self.f0_floor <= self.f0_ceil <= self.sr or not self.threshold > 0.0:
            raise ValueError(f"f0 range {f0_floor}..{f0_ceil} at {self.sr} Hz, threshold {threshold}")
        if self.sr // self.f0_floor > 512:
            raise ValueError(f"f0_floor {f0_floor} at {self.sr} Hz needs {int(self.sr // self.f0_floor)} "
                             "lags: the kernel is built for at most 512")
        self.device = torch.device(device)
        self.tables = None
        if method == "pyin":
            prior, tri, centres = pyin_tables(self.hop, self.sr, self.f0_floor, self.f0_ceil)
            if len(centres) > PYIN_MAX_BINS:
                raise ValueError(f"f0 range {f0_floor}..{f0_ceil}: {len(centres)} pitch bins, the "
                                 f"kernel is built for at most {PYIN_MAX_BINS}")
            if len(tri) > 1024:
                raise ValueError(f"hop_length {self.hop} at {self.sr} Hz: a reach of {len(tri) - 1} "
                                 "bins per frame, the kernel is built for at most 1023")
            self.tables = tuple(torch.from_numpy(t).to(self.device) for t in (prior, tri, centres))

    def n_frames(self, length):
        return frame_count(length, self.hop)

    def __call__(self, wav, lens=None):
        """wav (B, S) or (S,) on the device -> ``(f0 (B, F), dip (B, F), n_frames (B) int64)``,
        F = 1 + S // hop, zeros past ``n_frames`` (without the batch axis for a 1-D wav); with
        ``method="pyin"`` the second is ``unvoiced``.  ``lens`` as in ``MelFrontEnd.__call__``:
        None, a host list (checked) or a device int64 tensor (not read back)."""
        single = wav.dim() == 1
        w = (wav[None] if single else wav).contiguous()
        if w.dtype != torch.float32:
            w = w.float()
        B, S = w.shape
        if lens is not None and not torch.is_tensor(lens):
            lens = [int(n) for n in lens]
            if len(lens) != B:
                raise ValueError(f"{len(lens)} lengths for {B} rows")
            for n in lens:
                if not 0 <= n <= S:
                    raise ValueError(f"length {n}: 0..{S} samples")
            lens = torch.from_numpy(np.asarray(lens, np.int64)).pin_memory().to(w.device,
                                                                                 non_blocking=True)
        if self.method == "pyin":
            out = K.f0_pyin(w, lens, self.hop, self.sr, self.f0_floor, self.f0_ceil, *self.tables)
        else:
            out = K.f0_yin(w, lens, self.hop, self.sr, self.f0_floor, self.f0_ceil, self.threshold)
        return tuple(o[0] for o in out) if single else out


# ------------------------------------------------------------------ silence split
class SilenceSplitter:
    """``librosa.effects.split(y, top_db, frame_length=2048, hop_length=512)`` on the device
    (``fs2_nonsilent_split``): the intervals of samples whose frames lie within ``top_db`` dB of
    the row's loudest frame (mean-square power per centred frame, floor 1e-10).  The rule is
    librosa 0.7.2's, read from its source; librosa is not a dependency and nothing was compared
    with it.  ``pad_mode="reflect"`` is that version's framing, ``"zero"`` librosa >= 0.10's.

    At ``top_db = 100`` -- the value data_preprocess.py:46 passes -- a waveform in (-1, 1) has
    ``p_max < 1``, every frame lies above ``p_max 1e-10 < 1e-10 <= max(1e-10, p_f)`` and the
    result is the single interval ``[0, len]``."""

    PAD_MODES = {"reflect": 0, "zero": 1}

    def __init__(self, top_db=60.0, frame_length=2048, hop_length=512, pad_mode="reflect",
                 device="cuda"):
        self.top_db, self.frame_length, self.hop = float(top_db), int(frame_length), int(hop_length)
        if pad_mode not in self.PAD_MODES:
            raise ValueError(f"pad_mode {pad_mode!r}: one of {sorted(self.PAD_MODES)}")
        if self.frame_length < 2 or self.frame_length > 4096 or self.frame_length % 2:
            raise ValueError(f"frame_length {frame_length} (even, 2..4096)")
        if not 1 <= self.hop <= self.frame_length:
            raise ValueError(f"hop_length {hop_length} (1..{self.frame_length})")
        if self.top_db != self.top_db:
            raise ValueError("top_db is NaN")
        self.pad_mode = pad_mode
        self.device = torch.device(device)

    def n_frames(self, length):
        return frame_count(length, self.hop) if int(length) > 0 else 0

    def __call__(self, wav, lens=None, max_intervals=None):
        """wav (B, S) or (S,) on the device -> ``(intervals (B, max_intervals, 2) int64,
        n_intervals (B) int32)`` on the device (without the batch axis for a 1-D wav).
        ``n_intervals`` is the true count, so ``n_intervals > max_intervals`` shows an overflow;
        rows of ``intervals`` past the count are zero.  ``max_intervals`` defaults to the bound
        ``(1 + S // hop) // 2 + 1``.  ``lens``: None (S for every row), a host list (checked) or
        a device int64 tensor (not read back).  An empty row has no interval."""
        single = wav.dim() == 1
        w = (wav[None] if single else wav).contiguous()
        if w.dtype != torch.float32:
            w = w.float()
        B, S = w.shape
        if lens is not None and not torch.is_tensor(lens):
            lens = [int(n) for n in lens]
            if len(lens) != B:
                raise ValueError(f"{len(lens)} lengths for {B} rows")
            for n in lens:
                if not 0 <= n <= S:
                    raise ValueError(f"length {n}: 0..{S} samples")
            lens = torch.from_numpy(np.asarray(lens, np.int64)).pin_memory().to(w.device,
                                                                                 non_blocking=True)
        iv, n_iv, _ = K.nonsilent_split(w, lens, self.top_db, self.frame_length, self.hop,
                                        self.PAD_MODES[self.pad_mode], max_intervals)
        return (iv[0], n_iv[0]) if single else (iv, n_iv)

    def split(self, y):
        """A numpy waveform -> numpy ``(n, 2)`` int64 intervals, the shape of the librosa call."""
        y = np.ascontiguousarray(y, np.float32)
        if y.ndim != 1:
            raise ValueError("split takes one mono waveform")
        if y.size == 0:
            return np.zeros((0, 2), np.int64)
        iv, n = self(torch.from_numpy(y).to(self.device))
        return iv[:int(n)].cpu().numpy()


# ------------------------------------------------------------------ resampling
KAISER_ROLLOFF, KAISER_BETA = 0.9475937167399596, 14.769656459379492  # resampy's kaiser_best


def resample_filter(sr_in, sr_out, zeros=64):
    """The low-pass filter of a rational resampler ``sr_in -> sr_out`` as ``fs2_resample`` reads
    it: ``(table float32 (2 half + 1), L, M, half)`` with ``L / M = sr_out / sr_in`` in lowest
    terms, ``half = ceil(zeros max(L, M) / rolloff)`` and ``table[i] = L h[i]``,

      h[i] = (rolloff / big) sinc(rolloff t / big) I0(beta sqrt(1 - (t / half)^2)) / I0(beta),
      t = i - half, big = max(L, M),

    a Kaiser-windowed sinc with the design numbers of resampy's ``kaiser_best``; computed in
    fp64 and rounded once."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1 or zeros < 1:
        raise ValueError(f"rates {sr_in} -> {sr_out}, zeros {zeros}")
    g = int(np.gcd(sr_in, sr_out))
    L, M = sr_out // g, sr_in // g
    big = max(L, M)
    half = int(np.ceil(zeros * big / KAISER_ROLLOFF))
    t = np.arange(-half, half + 1, dtype=np.float64)
    window = np.i0(KAISER_BETA * np.sqrt(np.maximum(1.0 - (t / half) ** 2, 0.0))) / np.i0(KAISER_BETA)
    h = (KAISER_ROLLOFF / big) * np.sinc(KAISER_ROLLOFF * t / big) * window
    return (L * h).astype(np.float32), L, M, half


class Resampler:
    """Waveforms of any rate at ``sr_out`` (``fs2_resample``), where the reference calls
    ``librosa.load(wav_path, sr=22050)`` (preprocessor.py:186).  librosa 0.7.2 resamples with
    resampy's ``kaiser_best``, which interpolates a 512-point table of a Kaiser-windowed sinc;
    this is a polyphase FIR that evaluates the same window design exactly at the offsets the
    ratio needs.  It is another implementation and its sample values are not resampy's (nor
    soxr's); no parity is claimed.  The device tables are kept per ``sr_in``."""

    def __init__(self, sr_out=22050, device="cuda", zeros=64):
        self.sr_out, self.zeros = int(sr_out), int(zeros)
        self.device = torch.device(device)
        self._tables = {}

    def table(self, sr_in):
        sr_in = int(sr_in)
        if sr_in not in self._tables:
            tab, L, M, half = resample_filter(sr_in, self.sr_out, self.zeros)
            self._tables[sr_in] = (torch.from_numpy(tab).to(self.device), L, M, half)
        return self._tables[sr_in]

    def out_len(self, length, sr_in):
        """``ceil(length L / M)``: the samples a row of ``length`` gives."""
        _, L, M, _ = self.table(sr_in) if int(sr_in) != self.sr_out else (None, 1, 1, 0)
        return -(-int(length) * L // M)

    def _i64(self, values, B, name):
        if values is None or torch.is_tensor(values):
            return values
        values = [int(v) for v in values]
        if len(values) != B:
            raise ValueError(f"{len(values)} {name} values for {B} rows")
        return torch.from_numpy(np.asarray(values, np.int64)).pin_memory().to(self.device,
                                                                              non_blocking=True)

    def __call__(self, wav, lens, sr_in, first=None, count=None):
        """wav (B, S) f32 on the device -> ``(out (B, S_out), out_lens (B) int64)``, zeros past
        ``out_lens``.  ``lens``: None (S each), a host list (checked) or a device int64 tensor
        (not read back).  ``first`` / ``count`` (per row, host lists or device int64) cut the
        window ``y[first:first + count]`` out of each row's result, the reference's trim
        (lines 187-189) at no cost; S_out is the largest ``count`` of a host list, otherwise
        ``ceil(S L / M)``.  Equal rates launch nothing: the input comes back (and ``lens`` as a
        tensor), and a window is then not supported."""
        if wav.dim() != 2:
            raise ValueError("wav is (B, S)")
        w = wav.contiguous()
        if w.dtype != torch.float32:
            w = w.float()
        B, S = w.shape
        if lens is not None and not torch.is_tensor(lens):
            lens = [int(n) for n in lens]
            for n in lens:
                if not 0 <= n <= S:
                    raise ValueError(f"length {n}: 0..{S} samples")
        if int(sr_in) == self.sr_out:
            if first is not None or count is not None:
                raise ValueError("equal rates: nothing is launched, slice the rows instead")
            if lens is None:
                lens = torch.full((B,), S, dtype=torch.int64, device=w.device)
            return wav, self._i64(lens, B, "lens")
        tab, L, M, half = self.table(sr_in)
        cols = -(-S * L // M)
        if count is not None and not torch.is_tensor(count):
            cols = max(min(max(int(c) for c in count), cols), 1)
        return K.resample(w, self._i64(lens, B, "lens"), tab, L, M, half,
                          first=self._i64(first, B, "first"), count=self._i64(count, B, "count"),
                          out_samples=cols)
