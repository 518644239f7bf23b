"""``Preprocessor.process_utterance`` and ``build_from_path`` (preprocessor/preprocessor.py:169-328)
on the device: a waveform and its alignment give the mel, pitch, energy and duration targets that
``dataset.py`` loads, and a corpus of them gives ``stats.json``.

  get_alignment       267-305   ``durations_from_intervals`` (host; TextGrid parsing stays with
                                the caller, who hands over ``(start, end, text)`` tuples)
  process_utterance   169-265   ``FeatureExtractor`` (batched, device tensors) and its
                                ``process_utterance`` (one numpy waveform, numpy results)
  remove_outlier, StandardScaler.partial_fit, normalize, stats.json
                      307-315, 94-97, 317-328, 126-141   ``CorpusStats``

The F0 contour is the one thing that is not the reference's: pyworld (DIO + StoneMask) is
replaced by the YIN of ``audio.PitchExtractor``.  Everything after the contour follows the
reference line for line, and every entry point takes ``f0=`` for contours made elsewhere.

Quirk kept: the phoneme-level average writes ``pitch[i]`` while later phonemes still read the
same array (lines 224-231); after zero durations ``pos`` falls behind ``i`` and a later phoneme
averages means already written.  ``fs2_segment_mean`` reproduces it.
"""
import numpy as np
import torch

from . import kernels as K
from .audio import MelFrontEnd, N_FFT, PitchExtractor, frame_count
from .config import load_configs

SIL_PHONES = ("sil", "sp", "spn", "silB", "silE", "")


def durations_from_intervals(intervals, sr, hop):
    """``get_alignment`` (267-305) over ``(start, end, text)`` tuples ->
    ``(phones, durations, start, end)``: leading and trailing silences trimmed, inner ones kept as
    ``sp``, a duration the difference of the rounded frame positions of its two ends."""
    phones, durations = [], []
    start_time, end_time, end_idx = 0, 0, 0
    for s, e, p in intervals:
        if phones == []:
            if p in SIL_PHONES:
                continue
            start_time = s
        if p not in SIL_PHONES:
            phones.append(p)
            end_time = e
            end_idx = len(phones)
        else:
            phones.append("sp")
        durations.append(int(np.round(e * sr / hop) - np.round(s * sr / hop)))
    return phones[:end_idx], durations[:end_idx], start_time, end_time


def check_utterance(length, durations, hop, phoneme_level):
    """The conditions the host can see, raised before anything is launched."""
    length, total = int(length), int(sum(durations))
    if length <= N_FFT // 2:
        raise ValueError(f"length {length}: the mel's reflect padding needs more than "
                         f"{N_FFT // 2} samples")
    if any(int(d) < 0 for d in durations):
        raise ValueError("negative duration")
    if total > frame_count(length, hop):
        raise ValueError(f"durations sum to {total} frames, the waveform has "
                         f"{frame_count(length, hop)}")
    if phoneme_level and len(durations) > total:
        raise ValueError(f"{len(durations)} phonemes over {total} frames (the reference's "
                         "in-place average raises IndexError)")
    return total


class FeatureExtractor:
    """Lines 195-242 for a batch.  ``__call__(wavs, lens, durations, f0=None)``: wavs (B, S) on the
    device, lens a host list (None: S each), durations a list of B int lists -> a dict of device
    tensors, every one zero past its row's length:

      mel       (B, T, n_mels)   T = max sum(durations); log-mel of the samples clipped to [-1, 1]
      pitch     (B, P) phoneme means of the interpolated contour, or (B, T) the raw contour
      energy    (B, P) phoneme means, or (B, T)
      n_frames  (B) int64        sum(durations)
      n_phones  (B) int64        len(durations)
      ok        (B) int32        0 where the reference returns None (at most one voiced frame,
                                 line 204); such a row's pitch is not interpolated

    ``f0`` (B, >= T) replaces the estimator (which reads the unclipped samples, line 196)."""

    def __init__(self, preprocess_config=None, device="cuda", f0_floor=71.0, f0_ceil=800.0,
                 threshold=0.15):
        pp = preprocess_config if preprocess_config is not None else load_configs()[0]
        self.pp = pp
        self.device = torch.device(device)
        self.front = MelFrontEnd(pp, device)
        self.pitcher = PitchExtractor(pp, device, f0_floor, f0_ceil, threshold)
        self.hop, self.sr = self.front.hop, self.front.sr
        for name in ("pitch", "energy"):
            level = pp[name]["feature"]
            if level not in ("phoneme_level", "frame_level"):
                raise ValueError(f"{name}.feature {level!r}")
        self.pitch_phoneme = pp["pitch"]["feature"] == "phoneme_level"
        self.energy_phoneme = pp["energy"]["feature"] == "phoneme_level"

    def _i64(self, values):
        return torch.from_numpy(np.ascontiguousarray(values, np.int64)).to(self.device)

    def __call__(self, wavs, lens, durations, f0=None):
        if wavs.dim() != 2:
            raise ValueError("wavs is (B, S)")
        B, S = wavs.shape
        lens = [S] * B if lens is None else [int(n) for n in lens]
        if len(lens) != B or len(durations) != B:
            raise ValueError(f"{len(lens)} lengths and {len(durations)} duration lists for {B} rows")
        durations = [[int(d) for d in row] for row in durations]
        for n in lens:
            if n > S:
                raise ValueError(f"length {n} of {S} samples")
        totals = [check_utterance(n, d, self.hop, self.pitch_phoneme or self.energy_phoneme)
                  for n, d in zip(lens, durations)]
        T, P = max(max(totals), 1), max(max(len(d) for d in durations), 1)
        if f0 is not None:
            f0 = torch.as_tensor(f0, dtype=torch.float32)
            if f0.dim() != 2 or f0.shape[0] != B or f0.shape[1] < T:
                raise ValueError(f"f0 is (B, >= {T})")
        dur = np.zeros((B, P), np.int64)
        for b, d in enumerate(durations):
            dur[b, :len(d)] = d
        dur, tot = self._i64(dur), self._i64(totals)
        n_phones = self._i64([len(d) for d in durations])

        mel, energy, _ = self.front(wavs, lens, clip=True)
        if f0 is None:
            f0 = self.pitcher(wavs, lens)[0]
        live = torch.arange(T, device=self.device)[None, :] < tot[:, None]
        cut = lambda x: x[:, :T].to(self.device).masked_fill(~live, 0.0).contiguous()  # noqa: E731
        mel = mel.transpose(1, 2)[:, :T].masked_fill(~live[:, :, None], 0.0).contiguous()
        pitch, energy = cut(f0), cut(energy)
        filled = pitch.clone()
        ok = K.pitch_fill_(filled, tot)
        if self.pitch_phoneme:
            pitch = K.segment_mean_(filled, dur, tot)
        if self.energy_phoneme:
            energy = K.segment_mean_(energy, dur, tot)
        return {"mel": mel, "pitch": pitch, "energy": energy, "n_frames": tot, "n_phones": n_phones,
                "ok": ok}

    def process_utterance(self, wav, intervals, f0=None):
        """Lines 169-265 for one numpy waveform at the configured rate and its ``(start, end,
        text)`` intervals: ``None`` where the reference returns it, else ``(mel (T, n_mels), pitch,
        energy, durations)`` as numpy float32 arrays and a list.  ``f0`` is a contour of the
        trimmed waveform."""
        _, durations, start, end = durations_from_intervals(intervals, self.sr, self.hop)
        if start >= end:
            return None
        wav = np.asarray(wav)[int(self.sr * start):int(self.sr * end)].astype(np.float32)
        check_utterance(len(wav), durations, self.hop, self.pitch_phoneme or self.energy_phoneme)
        out = self(torch.from_numpy(wav)[None].to(self.device), None, [durations],
                   None if f0 is None else np.asarray(f0, np.float32)[None])
        if int(out["ok"][0]) == 0:
            return None
        total, n = sum(durations), len(durations)
        pitch = out["pitch"][0, :n if self.pitch_phoneme else total]
        energy = out["energy"][0, :n if self.energy_phoneme else total]
        return (out["mel"][0, :total].cpu().numpy(), pitch.cpu().numpy(), energy.cpu().numpy(),
                durations)


_EXTRACTORS = {}


def process_utterance(wav, intervals, f0=None, preprocess_config=None, device="cuda"):
    """``FeatureExtractor(preprocess_config, device).process_utterance(wav, intervals, f0)`` with
    the extractor (its tables) kept between calls of the same config object and device."""
    key = (id(preprocess_config), str(device))
    if key not in _EXTRACTORS:
        _EXTRACTORS[key] = (preprocess_config, FeatureExtractor(preprocess_config, device))
    return _EXTRACTORS[key][1].process_utterance(wav, intervals, f0)


class CorpusStats:
    """One feature's running statistics (lines 94-141), kept on the device: ``partial_fit`` takes in
    what survives ``remove_outlier`` of each row, ``finalize`` reads the moments back (the only
    host read before ``stats``), ``normalize_`` rewrites values in place and tracks their
    extrema, ``stats`` is the feature's ``stats.json`` entry ``[min, max, mean, std]``.
    ``normalization=False`` is lines 107-116: mean 0 and std 1 whatever was fitted."""

    def __init__(self, device="cuda", normalization=True):
        self.device = torch.device(device)
        self.normalization = bool(normalization)
        self.state = torch.zeros(3, dtype=torch.float64, device=self.device)
        big = np.finfo(np.float64).max
        self.minmax = torch.tensor([big, -big], dtype=torch.float64, device=self.device)
        self.mean = self.std = None

    def _lens(self, values, lens):
        if lens is None or torch.is_tensor(lens):
            return lens
        return torch.from_numpy(np.ascontiguousarray(lens, np.int64)).to(self.device)

    def partial_fit(self, values, lens=None):
        """values (B, cols) f32 on the device, ``lens`` (B) live counts (None: all of a row)."""
        lens = self._lens(values, lens)
        v = values
        if lens is not None:
            dead = torch.arange(v.shape[1], device=v.device)[None, :] >= lens[:, None]
            v = v.masked_fill(dead, float("inf"))
        K.outlier_moments_(self.state, torch.sort(v, dim=1).values.contiguous(), lens)
        self.mean = self.std = None
        return self

    def finalize(self):
        n, mean, m2 = self.state.cpu().tolist()
        if not self.normalization:
            self.mean, self.std = 0.0, 1.0
        else:
            if n == 0:
                raise ValueError("no value was fitted")
            std = float(np.sqrt(m2 / n))
            self.mean, self.std = float(mean), std if std > 0.0 else 1.0  # sklearn's scale_
        return self.mean, self.std

    def normalize_(self, values, lens=None):
        if self.mean is None:
            self.finalize()
        return K.normalize_minmax_(values, self.mean, self.std, self.minmax, self._lens(values, lens))

    def stats(self):
        if self.mean is None:
            self.finalize()
        lo, hi = self.minmax.cpu().tolist()
        return [float(lo), float(hi), float(self.mean), float(self.std)]
