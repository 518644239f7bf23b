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

Beside it: ``PitchExtractor`` (YIN F0 on the same frames), ``SilenceSplitter``
(``librosa.effects.split``, the speaker encoder's data_preprocess.py:46) and ``Resampler``
(``librosa.load``'s rate conversion).
"""
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


class PitchExtractor:
    """The F0 contour on the frames of ``MelFrontEnd`` (centres ``k * hop``, ``1 + len // hop`` of
    them: the count ``pw.dio`` returns for ``frame_period = hop / sr``), by YIN
    (``fs2_f0_yin``).  The reference (preprocessor.py:196-201) calls pyworld's DIO + StoneMask;
    this is another estimator and its values are not DIO's.  ``dip`` is the normalised
    difference function at the chosen lag (its minimum over the lag range for an unvoiced
    frame): small means strongly periodic."""

    def __init__(self, preprocess_config=None, device="cuda", f0_floor=71.0, f0_ceil=800.0,
                 threshold=0.15):
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

    def n_frames(self, length):
        return frame_count(length, self.hop)

    def __call__(self, wav, lens=None):
        """wav (B, S) or (S,) on the device -> ``(f0 (B, F), dip (B, F), n_frames (B) int64)``,
        F = 1 + S // hop, zeros past ``n_frames`` (without the batch axis for a 1-D wav).
        ``lens`` as in ``MelFrontEnd.__call__``: None, a host list (checked) or a device int64
        tensor (not read back)."""
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
