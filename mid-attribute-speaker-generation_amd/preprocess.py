"""``Preprocessor.process_utterance`` and ``build_from_path`` (preprocessor/preprocessor.py:169-328)
on the device: a waveform and its alignment give the mel, pitch, energy and duration targets that
``dataset.py`` loads, and a corpus of them gives ``stats.json``.

  build_from_path     61-167    ``Preprocessor`` (the walk over ``raw_path``, ``.wav`` and
                                TextGrid reading by ``corpus_io``, resampling by
                                ``audio.Resampler``, the ``.npy`` files, ``stats.json``, the split)
  get_alignment       267-305   ``durations_from_intervals`` (host, over ``(start, end, text)``
                                tuples such as ``corpus_io.read_textgrid`` returns)
  process_utterance   169-265   ``FeatureExtractor`` (batched, device tensors) and its
                                ``process_utterance`` (one numpy waveform, numpy results)
  remove_outlier, StandardScaler.partial_fit, normalize, stats.json
                      307-315, 94-97, 317-328, 126-141   ``CorpusStats``

The F0 contour is the one thing that is not the reference's: pyworld (DIO + StoneMask) is
replaced by the YIN of ``audio.PitchExtractor``, or with ``pitch_method="pyin"`` by its pYIN
(threshold-distribution YIN with a Viterbi track: steadier voicing in noise).  Everything after
the contour follows the reference line for line whichever method made it, and every entry point
takes ``f0=`` for contours made elsewhere.

Quirk kept: the phoneme-level average writes ``pitch[i]`` while later phonemes still read the
same array (lines 224-231); after zero durations ``pos`` falls behind ``i`` and a later phoneme
averages means already written.  ``fs2_segment_mean`` reproduces it.
"""
import json
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import kernels as K
from .audio import MelFrontEnd, N_FFT, PitchExtractor, Resampler, frame_count
from .config import load_configs
from .corpus_io import read_textgrid, read_wav

SIL_PHONES = ("sil", "sp", "spn", "silB", "silE", "")
DECODE_THREADS = 4  # file reading and PCM decoding of a group; not sized by the machine


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

    ``f0`` (B, >= T) replaces the estimator (which reads the unclipped samples, line 196).
    ``pitch_method`` is ``PitchExtractor``'s ``method``: ``"yin"`` or ``"pyin"`` (which ignores
    ``threshold``)."""

    def __init__(self, preprocess_config=None, device="cuda", f0_floor=71.0, f0_ceil=800.0,
                 threshold=0.15, pitch_method="yin"):
        pp = preprocess_config if preprocess_config is not None else load_configs()[0]
        self.pp = pp
        self.device = torch.device(device)
        self.front = MelFrontEnd(pp, device)
        self.pitcher = PitchExtractor(pp, device, f0_floor, f0_ceil, threshold,
                                      method=pitch_method)
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


class Preprocessor:
    """The reference's class (preprocessor/preprocessor.py:16-167), same constructor argument
    and ``build_from_path()``: ``raw_path/<speaker>/<basename>.wav`` + ``.lab`` and
    ``preprocessed_path/TextGrid/<speaker>/<basename>.TextGrid`` become ``mel/ pitch/ energy/
    duration/`` ``.npy`` files, ``stats.json`` and ``train.txt`` / ``val.txt`` / ``test.txt``.

    ``config`` is the reference's merged dict (``path.raw_path``, ``path.preprocessed_path``,
    ``preprocessing.{val_size, test_size, audio, stft, mel, pitch, energy}``).  Utterances are
    taken ``batch`` at a time: decoded on the host (``corpus_io.read_wav``, a small thread pool),
    packed into one pinned buffer and copied once, resampled on the device with one launch per
    distinct file rate (``audio.Resampler``, the trim of lines 187-189 as its output window), and
    put through ``FeatureExtractor`` in one call.  Pitch and energy stay on the device between the
    two passes while they fit ``keep_bytes`` (then every file is written once, normalised);
    past the budget a group's raw values go to their files and the second pass re-reads them.
    Only the files this run wrote are normalised.

    Differences from the reference, all deliberate: speakers and files are walked in sorted
    order (``os.listdir`` order there) and the split is drawn from ``random.Random(seed)``; the
    F0 contour is ``audio.PitchExtractor``'s (``pitch_method`` = ``"yin"`` or ``"pyin"``) unless
    ``f0_dir`` holds
    ``<speaker>-f0-<basename>.npy`` contours of the trimmed waveforms; pitch and energy are
    stored as float32."""

    def __init__(self, config, device="cuda", batch=16, seed=None, f0_dir=None,
                 keep_bytes=1 << 30, pitch_method="yin"):
        self.config = config
        self.in_dir = config["path"]["raw_path"]
        self.out_dir = config["path"]["preprocessed_path"]
        pp = config["preprocessing"]
        self.val_size, self.test_size = pp["val_size"], pp["test_size"]
        self.sampling_rate = pp["audio"]["sampling_rate"]
        self.hop_length = pp["stft"]["hop_length"]
        self.pitch_normalization = pp["pitch"]["normalization"]
        self.energy_normalization = pp["energy"]["normalization"]
        self.device = torch.device(device)
        self.batch, self.seed, self.f0_dir = int(batch), seed, f0_dir
        self.keep_bytes = int(keep_bytes)
        if self.batch < 1:
            raise ValueError(f"batch {batch}")
        # checks pitch.feature / energy.feature and the pitch method
        self.extractor = FeatureExtractor(pp, device, pitch_method=pitch_method)
        self.pitch_phoneme_averaging = self.extractor.pitch_phoneme
        self.energy_phoneme_averaging = self.extractor.energy_phoneme
        self.resampler = Resampler(self.sampling_rate, device)
        self._pinned = None

    # -------------------------------------------------------------- the walk (lines 74-92)
    def _walk(self):
        """``[(speaker index, speaker, basename, phones, durations, start, end)]`` of the
        utterances to process and the sorted speakers; a missing TextGrid raises (line 92)."""
        speakers = sorted(s for s in os.listdir(self.in_dir)
                          if os.path.isdir(os.path.join(self.in_dir, s)))
        items = []
        for si, speaker in enumerate(speakers):
            for wav_name in sorted(os.listdir(os.path.join(self.in_dir, speaker))):
                if ".wav" not in wav_name:
                    continue
                basename = wav_name.split(".")[0]
                tg_path = os.path.join(self.out_dir, "TextGrid", speaker, f"{basename}.TextGrid")
                if not os.path.exists(tg_path):
                    raise ValueError(tg_path)
                tiers = read_textgrid(tg_path)
                if "phones" not in tiers:
                    raise ValueError(f"{tg_path}: no interval tier named 'phones'")
                phones, durations, start, end = durations_from_intervals(
                    tiers["phones"], self.sampling_rate, self.hop_length)
                if start >= end:
                    continue
                items.append((si, speaker, basename, phones, durations, start, end))
        return speakers, items

    def _stage(self, group, pool):
        """One group's waveforms at the configured rate, trimmed: ``(wavs (B, S) on the device,
        lens)``.  The decoded files go through one pinned buffer and one copy; each distinct file
        rate is one ``(rows, samples)`` block of it and one resample launch."""
        sr_out = self.sampling_rate
        paths = [os.path.join(self.in_dir, it[1], f"{it[2]}.wav") for it in group]
        decoded = list(pool.map(read_wav, paths))
        window = [(int(sr_out * it[5]), int(sr_out * it[6])) for it in group]
        by_rate = {}
        for b, (x, sr) in enumerate(decoded):
            by_rate.setdefault(sr, []).append(b)
        rows = {}
        for sr, members in by_rate.items():
            if sr == sr_out:  # nothing to resample: only the trimmed span is copied
                for b in members:
                    rows[b] = decoded[b][0][window[b][0]:window[b][1]]
            else:
                for b in members:
                    rows[b] = decoded[b][0]
        blocks, total = {}, 0
        for sr, members in by_rate.items():
            S = max(max(len(rows[b]) for b in members), 1)
            blocks[sr] = (total, S)
            total += len(members) * S
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1 << 20), dtype=torch.float32).pin_memory()
        host = self._pinned.numpy()
        for sr, members in by_rate.items():
            off, S = blocks[sr]
            for k, b in enumerate(members):
                n = len(rows[b])
                host[off + k * S:off + k * S + n] = rows[b]
                host[off + k * S + n:off + (k + 1) * S] = 0.0
        dev = self._pinned[:total].to(self.device, non_blocking=True)
        parts, lens = {}, [0] * len(group)
        for sr, members in by_rate.items():
            off, S = blocks[sr]
            block = dev[off:off + len(members) * S].view(len(members), S)
            n_in = [len(rows[b]) for b in members]
            if sr == sr_out:
                out, n_out = block, n_in
            else:
                first = [window[b][0] for b in members]
                count = [max(window[b][1] - window[b][0], 0) for b in members]
                out, _ = self.resampler(block, n_in, sr, first=first, count=count)
                n_out = [max(min(c, self.resampler.out_len(n, sr) - f), 0)
                         for n, f, c in zip(n_in, first, count)]
            parts[sr] = out
            for k, b in enumerate(members):
                lens[b] = n_out[k]
        if len(parts) == 1:
            (wavs,) = parts.values()
            return wavs[:, :max(max(lens), 1)].contiguous(), lens
        wavs = torch.zeros((len(group), max(max(lens), 1)), dtype=torch.float32, device=self.device)
        for sr, members in by_rate.items():
            out = parts[sr]
            wavs[torch.as_tensor(members, device=self.device), :out.shape[1]] = out[:, :wavs.shape[1]]
        return wavs, lens

    def _given_f0(self, group, totals):
        T = max(max(totals), 1)
        f0 = np.zeros((len(group), T), np.float32)
        for b, it in enumerate(group):
            c = np.load(os.path.join(self.f0_dir, f"{it[1]}-f0-{it[2]}.npy")).astype(np.float32)
            f0[b, :min(len(c), T)] = c[:T]
        return f0

    def _path(self, kind, speaker, basename):
        return os.path.join(self.out_dir, kind, f"{speaker}-{kind}-{basename}.npy")

    def build_from_path(self):
        for kind in ("mel", "pitch", "energy", "duration"):
            os.makedirs(os.path.join(self.out_dir, kind), exist_ok=True)
        print("Processing Data ...")
        speakers, items = self._walk()
        out = [[] for _ in speakers]
        stats = {"pitch": CorpusStats(self.device, self.pitch_normalization),
                 "energy": CorpusStats(self.device, self.energy_normalization)}
        phoneme = {"pitch": self.pitch_phoneme_averaging, "energy": self.energy_phoneme_averaging}
        kept, kept_bytes, n_frames = [], 0, 0
        fx = self.extractor
        with ThreadPoolExecutor(max_workers=DECODE_THREADS) as pool:
            for g0 in range(0, len(items), self.batch):
                group = items[g0:g0 + self.batch]
                wavs, lens = self._stage(group, pool)
                durations = [it[4] for it in group]
                totals = []
                for it, n in zip(group, lens):
                    try:
                        totals.append(check_utterance(n, it[4], self.hop_length,
                                                      fx.pitch_phoneme or fx.energy_phoneme))
                    except ValueError as err:
                        raise ValueError(f"{it[2]}: {err}") from None
                f0 = self._given_f0(group, totals) if self.f0_dir is not None else None
                res = fx(wavs, lens, durations, f0=f0)
                ok = res["ok"].cpu().numpy() != 0  # line 204: the one host read of a group
                rows = np.flatnonzero(ok)
                if rows.size == 0:
                    continue
                pick = torch.from_numpy(rows).to(self.device)
                mel = res["mel"].index_select(0, pick).cpu().numpy()
                members = [group[b] for b in rows]
                for k, (si, speaker, basename, phones, dur, _, _) in enumerate(members):
                    np.save(self._path("duration", speaker, basename), np.asarray(dur, np.int64))
                    np.save(self._path("mel", speaker, basename), mel[k, :sum(dur)])
                    with open(os.path.join(self.in_dir, speaker, f"{basename}.lab"), "r") as f:
                        raw_text = f.readline().strip("\n")
                    out[si].append("|".join([basename, speaker, "{" + " ".join(phones) + "}",
                                             raw_text]))
                    n_frames += sum(dur)
                entry = {"members": members}
                for name in ("pitch", "energy"):
                    values = res[name].index_select(0, pick).contiguous()
                    n = res["n_phones" if phoneme[name] else "n_frames"].index_select(0, pick)
                    stats[name].partial_fit(values, n)
                    entry[name] = (values, n)
                    kept_bytes += values.numel() * 4
                if kept_bytes > self.keep_bytes:  # past the budget: raw values to the files
                    for name in ("pitch", "energy"):
                        self._write(name, members, *entry[name])
                        entry[name] = None
                kept.append(entry)

        print("Computing statistic quantities ...")
        for entry in kept:
            for name in ("pitch", "energy"):
                if entry[name] is None:
                    entry[name] = self._reread(name, entry["members"])
                values, n = entry[name]
                stats[name].normalize_(values, n)
                self._write(name, entry["members"], values, n)
        with open(os.path.join(self.out_dir, "stats.json"), "w") as f:
            f.write(json.dumps({"pitch": stats["pitch"].stats() if kept else [0.0, 0.0, 0.0, 1.0],
                                "energy": stats["energy"].stats() if kept else [0.0, 0.0, 0.0, 1.0]}))
        print("Total time: {} hours".format(n_frames * self.hop_length / self.sampling_rate / 3600))
        write_split(out, self.out_dir, self.val_size, self.test_size, self.seed)
        return out

    def _write(self, name, members, values, n):
        values, n = values.cpu().numpy(), n.cpu().tolist()
        for k, (_, speaker, basename, *_) in enumerate(members):
            np.save(self._path(name, speaker, basename), values[k, :n[k]])

    def _reread(self, name, members):
        rows = [np.load(self._path(name, it[1], it[2])) for it in members]
        values = np.zeros((len(rows), max(max(len(r) for r in rows), 1)), np.float32)
        for k, r in enumerate(rows):
            values[k, :len(r)] = r
        n = torch.from_numpy(np.asarray([len(r) for r in rows], np.int64)).to(self.device)
        return torch.from_numpy(values).to(self.device), n


def write_split(out, out_dir, val_size, test_size, seed=None):
    """Lines 149-165 with a generator of its own: ``out`` (one list of metadata lines per
    speaker) is shuffled in place, speakers first and then each speaker's lines, and every
    speaker's lines are cut at ``int(len * (1 - val - test))`` and ``int(len * (1 - test))`` into
    ``train.txt``, ``val.txt`` and ``test.txt``."""
    rng = random.Random(seed)
    rng.shuffle(out)
    for r in out:
        rng.shuffle(r)
    cuts = {"train.txt": lambda n: (0, int(n * (1 - val_size - test_size))),
            "val.txt": lambda n: (int(n * (1 - val_size - test_size)), int(n * (1 - test_size))),
            "test.txt": lambda n: (int(n * (1 - test_size)), n)}
    for name, cut in cuts.items():
        with open(os.path.join(out_dir, name), "w", encoding="utf-8") as f:
            for spk in out:
                lo, hi = cut(len(spk))
                for m in spk[lo:hi]:
                    f.write(m + "\n")
    return out


def main(argv=None):
    """The reference's ``preprocess.py``: ``--config DIR [--corpus NAME] [--pitch_method
    {yin,pyin}]`` reads
    ``DIR/preprocess.yaml`` (with its two ``normalization = False`` overrides) and
    ``DIR/preprocess_<corpus>.yaml``, every ``preprocess_*.yaml`` without ``--corpus``."""
    import argparse
    from pathlib import Path

    import yaml

    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, required=True, help="path to config")
    parser.add_argument("--corpus", type=str, default=None, help="corpus name")
    parser.add_argument("--pitch_method", choices=PitchExtractor.METHODS, default="yin",
                        help="the F0 estimator: plain YIN, or pYIN (threshold distribution + "
                             "Viterbi track)")
    args = parser.parse_args(argv)
    with open(os.path.join(args.config, "preprocess.yaml")) as f:
        preprocess_config = yaml.safe_load(f)
    preprocess_config["pitch"]["normalization"] = False
    preprocess_config["energy"]["normalization"] = False
    if args.corpus is not None:
        files = [Path(args.config) / f"preprocess_{args.corpus}.yaml"]
    else:
        files = sorted(Path(args.config).glob("preprocess_*.yaml"))
    for path in files:
        with open(path) as f:
            config = yaml.safe_load(f)
        config["preprocessing"] = preprocess_config
        config["preprocessing"]["text"] = config["text"]
        print("preprocessing...:", config["dataset"])
        Preprocessor(config, pitch_method=args.pitch_method).build_from_path()


if __name__ == "__main__":
    main()
