"""The speaker encoder's training corpus from waveforms: ``data_preprocess.py`` and
``dataset/{jvs,vctk}.py`` of ``Multilingual-Speaker-Encoder-with-Domain-Adaptation``.

Per utterance the reference (data_preprocess.py:39-88) reads the wav, resamples it to 22 050 Hz,
splits it with ``librosa.effects.split(utter, top_db=100)``, drops intervals shorter than
``tisv_frame * hop + window`` samples, takes the ``TacotronSTFT`` log-mel of each interval, cuts
it into ``tisv_frame``-frame windows at half-window steps and stacks a speaker's windows into
``<dataset>_<spkr>_<gender>_<language>.npy`` -- the files ``embedder_data.SpeakerStore`` loads.
Here the files are decoded on the host (``corpus_io.read_wav``) and everything after runs on the
device: ``audio.Resampler``, ``fs2_nonsilent_split``, ``fs2_wave_segments``,
``audio.MelFrontEnd`` and ``fs2_tisv_windows``.

At the reference's ``top_db = 100`` the split keeps every frame of a waveform in (-1, 1)
(``audio.SilenceSplitter``), so its corpus is "whole utterance -> mel -> windows"; the split
changes the result only at other values, which ``top_db=`` and ``--top_db`` select.

  python -m mid-attribute-speaker-generation_amd.embedder_preprocess --config config.yaml
"""
import glob
import os
from collections import OrderedDict

import numpy as np
import torch

from . import kernels as K
from .audio import MelFrontEnd, N_FFT, Resampler, SilenceSplitter, frame_count
from .config import load_configs
from .corpus_io import read_wav

data_template = "{dataset}_{spkr}_{gender}_{language}.npy"  # data_preprocess.py:22


class SpeakerCorpus:
    """What ``process_spkr_wavlist`` needs of a dataset class (dataset/jvs.py, dataset/vctk.py):
    ``_name``, ``_language``, ``spkrs``, ``test_speakers``, ``spkr_number``, ``get_gender`` and
    ``spkr_wavlist()``.  ``speakers`` is an ordered ``{spkr: {"gender": g, "wavs": [paths]}}``.

    ``jvs`` and ``vctk`` are written from the corpora's layouts; the reference walks them with
    nnmnkwii's data sources, which are not installed where this was built, so nnmnkwii's own file
    order could not be checked.  The order only matters for reproducing the utterance indices of
    a reference run; the set of windows per speaker is the same."""

    def __init__(self, name, language, speakers, test_speakers=()):
        self._name, self._language = str(name), str(language)
        self.spkrs = OrderedDict((s, dict(v, wavs=list(v["wavs"]))) for s, v in speakers.items())
        self.test_speakers = list(test_speakers)

    @property
    def spkr_number(self):
        return len(self.spkrs)

    def get_gender(self, spkr):
        return self.spkrs[spkr]["gender"].lower()

    def spkr_wavlist(self):
        """``(spkr, wav paths)`` of every speaker that has wavs, in order."""
        for spkr, v in self.spkrs.items():
            if v["wavs"]:
                yield spkr, v["wavs"]

    def filename(self, spkr):
        return data_template.format(dataset=self._name, spkr=spkr, gender=self.get_gender(spkr),
                                    language=self._language)

    @classmethod
    def jvs(cls, root, test_speakers=()):
        """JVS (dataset/jvs.py, jvs_source.py): ``root/gender_f0range.txt`` lists ``speaker
        Male_or_Female minf0[Hz] maxf0[Hz]`` under a header line; a speaker's wavs are
        ``root/<spkr>/parallel100/wav24kHz16bit/*.wav`` sorted by base name (``collect_files()``
        defaults to ``parallel100`` alone)."""
        root = os.path.expanduser(root)
        speakers = OrderedDict()
        with open(os.path.join(root, "gender_f0range.txt"), encoding="utf8") as f:
            for line in f:
                fields = line.strip().split()
                if not fields or fields[0] == "speaker":
                    continue
                if len(fields) != 4:
                    raise ValueError(f"gender_f0range.txt: {line.strip()!r} has {len(fields)} fields")
                wavs = glob.glob(os.path.join(root, fields[0], "parallel100", "wav24kHz16bit", "*.wav"))
                speakers[fields[0]] = {"gender": fields[1],
                                       "wavs": sorted(wavs, key=os.path.basename)}
        return cls("jvs", "jp", speakers, test_speakers)

    @classmethod
    def vctk(cls, root, test_speakers=()):
        """VCTK (dataset/vctk.py): ``root/speaker-info.txt`` has the columns ``ID AGE GENDER
        ...`` under a header line; speaker ``p<ID>``'s wavs are ``root/wav48/p<ID>/*.wav``
        sorted; a speaker without wavs is dropped (vctk.py:18-20)."""
        root = os.path.expanduser(root)
        speakers = OrderedDict()
        with open(os.path.join(root, "speaker-info.txt"), encoding="utf8") as f:
            for line in f:
                fields = line.strip().split()
                if len(fields) < 3 or fields[0] == "ID":
                    continue
                spkr = "p" + fields[0]
                wavs = sorted(glob.glob(os.path.join(root, "wav48", spkr, "*.wav")))
                if wavs:
                    speakers[spkr] = {"gender": fields[2], "wavs": wavs}
        return cls("vctk", "en", speakers, test_speakers)


class EncoderPreprocessor:
    """``save_spectrogram_tisv`` (data_preprocess.py:90-116) over ``corpora`` (``SpeakerCorpus``
    objects): one ``(windows, n_mels, tisv_frame)`` fp32 file per speaker, under ``test_path``
    for a corpus's ``test_speakers`` and ``train_path`` for the rest.

    A speaker's files are taken ``batch`` at a time: decoded on the host, uploaded padded,
    resampled with one launch per distinct file rate, split, and the one host read of the group
    (the interval counts and intervals) sizes the rest -- the kept intervals gathered into rows,
    their log-mel in one ``fs2_melspec`` launch, the windows cut.  Windows are ordered by file,
    then interval, then window, as in the reference.

    Deviations, deliberate: a speaker with no window writes no file and is reported with count
    0 (the reference saves an empty array, which ``SpeakerStore`` rejects); multi-channel files
    are averaged by ``read_wav`` (``soundfile.read`` would hand the reference a 2-D array); the
    resampler is ``audio.Resampler``, not ``librosa.resample``."""

    def __init__(self, corpora, train_path, test_path, device="cuda", sr=22050, hop=256,
                 window=1024, tisv_frame=150, top_db=100.0, batch=16, overwrite=False):
        self.corpora = list(corpora)
        self.train_path, self.test_path = train_path, test_path
        self.device = torch.device(device)
        self.sr, self.hop, self.window = int(sr), int(hop), int(window)
        self.tisv_frame, self.batch, self.overwrite = int(tisv_frame), int(batch), bool(overwrite)
        if self.batch < 1 or not 1 <= self.tisv_frame <= 256:
            raise ValueError(f"batch {batch}, tisv_frame {tisv_frame} (1..256)")
        pp = load_configs()[0]
        pp = dict(pp, audio=dict(pp["audio"], sampling_rate=self.sr),
                  stft=dict(pp["stft"], filter_length=self.window, win_length=self.window,
                            hop_length=self.hop))
        self.frontend = MelFrontEnd(pp, device)  # raises unless window == 1024
        self.resampler = Resampler(self.sr, device)
        self.splitter = SilenceSplitter(top_db=top_db, device=device)
        self.utter_min_len = self.tisv_frame * self.hop + self.window  # line 99

    # ------------------------------------------------------------------ one group of files
    def _i64(self, values):
        return torch.from_numpy(np.asarray(values, np.int64)).to(self.device)

    def _stage(self, decoded):
        """Decoded ``(samples, rate)`` pairs -> ``(wavs (B, S) at self.sr on the device, host
        lengths)``; one upload and one resample launch per distinct file rate."""
        by_rate = OrderedDict()
        for b, (_, sr) in enumerate(decoded):
            by_rate.setdefault(sr, []).append(b)
        parts, lens = [], [0] * len(decoded)
        for sr, members in by_rate.items():
            n_in = [len(decoded[b][0]) for b in members]
            host = np.zeros((len(members), max(max(n_in), 1)), np.float32)
            for k, b in enumerate(members):
                host[k, :n_in[k]] = decoded[b][0]
            out, _ = self.resampler(torch.from_numpy(host).to(self.device), n_in, sr)
            for k, b in enumerate(members):
                lens[b] = self.resampler.out_len(n_in[k], sr)
            parts.append((members, out))
        if len(parts) == 1:
            return parts[0][1].contiguous(), lens
        wavs = torch.zeros((len(decoded), max(max(lens), 1)), dtype=torch.float32, device=self.device)
        for members, out in parts:
            cols = min(out.shape[1], wavs.shape[1])
            wavs[torch.as_tensor(members, device=self.device), :cols] = out[:, :cols]
        return wavs, lens

    def _group(self, paths):
        """``(windows (W, n_mels, tisv) or None, per-file window counts)`` of up to ``batch``
        files."""
        wavs, lens = self._stage([read_wav(p) for p in paths])
        B = len(paths)
        iv, n_iv = self.splitter(wavs, lens)
        # the one host read of the group: counts and intervals together
        host = torch.cat([n_iv.to(torch.int64)[:, None], iv.reshape(B, -1)], dim=1).cpu().numpy()
        seg_row, seg_first, seg_len, owner = [], [], [], []
        for b in range(B):
            for a, e in host[b, 1:1 + 2 * int(host[b, 0])].reshape(-1, 2):
                if e - a < self.utter_min_len:  # lines 53-55
                    continue
                seg_row.append(b), seg_first.append(int(a)), seg_len.append(int(e - a))
        counts = [0] * B
        if not seg_row:
            return None, counts
        per_seg = [K.tisv_window_count(frame_count(n, self.hop), self.tisv_frame) for n in seg_len]
        for b, n in zip(seg_row, per_seg):
            counts[b] += n
        win_off = np.concatenate([[0], np.cumsum(per_seg)]).astype(np.int64)
        # one upload for the four descriptor arrays
        n_seg = len(seg_row)
        desc = self._i64(np.concatenate([seg_first, seg_len, win_off, seg_row]))
        first_d, len_d, off_d = desc[:n_seg], desc[n_seg:2 * n_seg], desc[2 * n_seg:3 * n_seg + 1]
        row_d = desc[3 * n_seg + 1:].to(torch.int32)
        segs = K.wave_segments(wavs, row_d, first_d, len_d, max(seg_len))
        mel, _, n_frames = self.frontend(segs, lens=len_d)
        windows = K.tisv_windows(mel, n_frames, off_d, int(win_off[-1]), self.tisv_frame)
        return windows, counts

    def process_wavs(self, paths):
        """``process_wav`` (lines 39-67) over a speaker's files: ``(windows (W, n_mels,
        tisv_frame) on the device, per-file window counts)``."""
        paths = list(paths)
        chunks, counts = [], []
        for lo in range(0, len(paths), self.batch):
            w, c = self._group(paths[lo:lo + self.batch])
            counts.extend(c)
            if w is not None and w.shape[0]:
                chunks.append(w)
        if not chunks:
            empty = torch.zeros((0, self.frontend.n_mels, self.tisv_frame), dtype=torch.float32,
                                device=self.device)
            return empty, counts
        return (chunks[0] if len(chunks) == 1 else torch.cat(chunks)), counts

    # ------------------------------------------------------------------ the corpus
    def save_spectrogram_tisv(self):
        """Write every speaker's file; ``{file name: window count}``.  An existing file is kept
        unless ``overwrite`` (line 79) and reported with the count it holds."""
        os.makedirs(self.train_path, exist_ok=True)
        os.makedirs(self.test_path, exist_ok=True)
        report = OrderedDict()
        for ds in self.corpora:
            for spkr, wavlist in ds.spkr_wavlist():
                name = ds.filename(spkr)
                folder = self.test_path if spkr in ds.test_speakers else self.train_path
                path = os.path.join(folder, name)
                if os.path.exists(path) and not self.overwrite:
                    report[name] = int(np.load(path, mmap_mode="r").shape[0])
                    continue
                windows, counts = self.process_wavs(wavlist)
                report[name] = int(windows.shape[0])
                for wav, n in zip(wavlist, counts):
                    if n == 0:
                        print(f"Warning: spkr {spkr}'s wav: {wav} has no specs, try to improve top_db")
                if windows.shape[0] == 0:
                    if os.path.exists(path):
                        os.remove(path)
                    continue
                tmp = path + ".tmp"
                with open(tmp, "wb") as f:
                    np.save(f, windows.cpu().numpy())
                os.replace(tmp, path)
        return report


def load_hparam(path):
    """The reference's multi-document ``config.yaml`` merged into one dict (hparam.py:8-15)."""
    import yaml
    merged = {}
    with open(path) as f:
        for doc in yaml.safe_load_all(f):
            merged.update(doc or {})
    return merged


def collect_datasets(hp):
    """``collect_datasets`` (lines 24-35): the ``datasets`` entries named in ``train_datasets``,
    in the order of ``datasets``."""
    corpora = []
    for name, kwarg in hp["datasets"].items():
        if name not in hp["train_datasets"]:
            continue
        make = {"jvs": SpeakerCorpus.jvs, "vctk": SpeakerCorpus.vctk}.get(name.lower())
        if make is None:
            raise ValueError(f"dataset {name!r}: JVS and VCTK are built")
        corpora.append(make(kwarg["root"], kwarg.get("test_speakers", ())))
    return corpora


def main(argv=None):
    import argparse

    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, required=True, help="the encoder's config.yaml")
    parser.add_argument("--top_db", type=float, default=100.0, help="silence threshold (dB)")
    parser.add_argument("--batch", type=int, default=16, help="files per group")
    parser.add_argument("--overwrite", action="store_true")
    args = parser.parse_args(argv)
    hp = load_hparam(args.config)
    data = hp["data"]
    if int(data.get("nfft", N_FFT)) != N_FFT:
        raise ValueError(f"data.nfft {data['nfft']}: the mel front end is built for {N_FFT}")
    report = EncoderPreprocessor(
        collect_datasets(hp), data["train_path"], data["test_path"], device=hp.get("device", "cuda"),
        sr=data["sr"], hop=data["hop"], window=data["window"], tisv_frame=data["tisv_frame"],
        top_db=args.top_db, batch=args.batch, overwrite=args.overwrite).save_spectrogram_tisv()
    for name, n in report.items():
        print(f"{name}: {n} windows")
    return report


if __name__ == "__main__":
    main()
