"""TextGrids from ``.wav`` + phoneme transcriptions, where the reference needs the Montreal
Forced Aligner (or HTS / Julius labels) to have run first:

    python -m mid-attribute-speaker-generation_amd.align --config DIR [--corpus NAME]
        [--steps N] [--batch B] [--checkpoint P] [--seed S] [--optional_sil SYMBOL]
        [--no_edge_sil]

walks ``raw_path/<speaker>/*.wav`` as ``Preprocessor._walk`` does, reads each utterance's phoneme
string from ``<basename>.phn`` (one line of space-separated symbols of ``configs/symbols.json``,
braces optional; the ``.lab`` file stays the raw text), computes the log-mels with ``Resampler``
and ``MelFrontEnd`` and keeps them on the device (flat, with an offset table), trains an
``aligner.Aligner`` on them for ``--steps`` updates (or loads ``--checkpoint``), aligns every
utterance and writes ``preprocessed_path/TextGrid/<speaker>/<basename>.TextGrid`` with one
interval tier ``phones``.  ``preprocess.Preprocessor`` then reads those files as it reads MFA's.

An existing TextGrid is never overwritten (hand-made alignments win) and its utterance is left
out.  The first ``L // hop`` frames of a file of ``L`` samples (at the configured rate) are
aligned, so that the waveform trimmed to the last boundary still has every frame.

Silences.  Without ``--optional_sil`` a silence is aligned only where the ``.phn`` line has ``sp``.
With ``--optional_sil sp`` the token ``|`` in a ``.phn`` line marks a place where a pause may
stand (a word boundary), and, unless ``--no_edge_sil``, one may stand at the start and at the end
of the utterance.  Each such place becomes an optional ``sp`` position that the forward-sum loss
and the alignment search may give no frame at all (``K.forward_sum`` / ``K.mas`` with a mask);
positions left without a frame are not written, the others are ordinary ``sp`` intervals, which
``preprocess.durations_from_intervals`` trims at the edges and keeps inside.  An aligner trained
with the flag runs without the beta-binomial prior (``omega = 0`` instead of 1).
"""
import os

import numpy as np
import torch

from . import kernels as K
from .aligner import Aligner, AlignerTrainer
from .audio import N_FFT, MelFrontEnd, Resampler
from .corpus_io import read_wav, write_textgrid
from .dataset import symbol_table
from .preprocess import SIL_PHONES


def parse_phn(path, table=None, optional_sil=None, edges=True):
    """The symbols and ids of a ``.phn`` file; a missing file, an empty line or a symbol that is
    not in ``configs/symbols.json`` (or is its padding symbol, id 0) raises naming the file.

    With ``optional_sil`` (a symbol of the table, normally ``sp``) the token ``|`` marks a place
    where a pause may stand: each run of ``|`` becomes one optional ``optional_sil`` position,
    except next to an explicit silence phone (``preprocess.SIL_PHONES``), which stays mandatory;
    with ``edges`` an optional position is added at the start and at the end unless the line
    starts or ends with a silence phone.  Returns ``(phones, ids, optional)`` then, ``optional``
    a list of 0 / 1 per position."""
    table = table if table is not None else {s: i for i, s in enumerate(symbol_table())}
    if not os.path.exists(path):
        raise ValueError(f"{path}: no phoneme transcription for this utterance")
    with open(path, encoding="utf-8") as f:
        line = f.readline().strip()
    if line.startswith("{") and line.endswith("}"):
        line = line[1:-1]
    phones = line.split()
    if optional_sil is not None:
        return _with_optional_sil(path, phones, table, optional_sil, edges)
    if not phones:
        raise ValueError(f"{path}: no phonemes")
    for p in phones:
        if table.get(p, 0) == 0:
            raise ValueError(f"{path}: unknown symbol {p!r}")
    return phones, [table[p] for p in phones]


def _with_optional_sil(path, tokens, table, optional_sil, edges):
    if table.get(optional_sil, 0) == 0:
        raise ValueError(f"optional_sil {optional_sil!r} is not a symbol of configs/symbols.json")
    phones, optional, pending = [], [], False
    for p in tokens:
        if p == "|":
            pending = bool(phones)  # a boundary mark before the first phone is the edge's
            continue
        if table.get(p, 0) == 0:
            raise ValueError(f"{path}: unknown symbol {p!r}")
        if pending and p not in SIL_PHONES and phones[-1] not in SIL_PHONES:
            phones.append(optional_sil), optional.append(1)
        pending = False
        phones.append(p), optional.append(0)
    if not phones:
        raise ValueError(f"{path}: no phonemes")
    lead, trail = tokens[0] == "|", tokens[-1] == "|"
    if (edges or lead) and phones[0] not in SIL_PHONES:
        phones.insert(0, optional_sil), optional.insert(0, 1)
    if (edges or trail) and phones[-1] not in SIL_PHONES:
        phones.append(optional_sil), optional.append(1)
    return phones, [table[p] for p in phones], optional


class MelStore:
    """The corpus's log-mels on the device: ``flat`` (total frames, n_mels) f32 and per utterance
    ``offset`` / ``frames`` (host lists), as ``corpus_store.CorpusStore`` keeps its features."""

    def __init__(self, preprocess_config, device="cuda", batch=16):
        self.device = torch.device(device)
        self.front = MelFrontEnd(preprocess_config, device)
        self.resampler = Resampler(self.front.sr, device)
        self.hop, self.sr, self.batch = self.front.hop, self.front.sr, int(batch)
        self.flat, self.offset, self.frames = None, [], []

    def build(self, wav_paths):
        parts, total = [], 0
        for g0 in range(0, len(wav_paths), self.batch):
            group = wav_paths[g0:g0 + self.batch]
            decoded = [read_wav(p) for p in group]
            for rate in sorted({sr for _, sr in decoded}):
                rows = [b for b, (_, sr) in enumerate(decoded) if sr == rate]
                n_in = [len(decoded[b][0]) for b in rows]
                host = np.zeros((len(rows), max(max(n_in), 1)), np.float32)
                for r, b in enumerate(rows):
                    host[r, :n_in[r]] = decoded[b][0]
                wavs, _ = self.resampler(torch.from_numpy(host).to(self.device), n_in, rate)
                lens = [self.resampler.out_len(n, rate) for n in n_in]
                for b, n in zip(rows, lens):
                    if n <= N_FFT // 2 or n // self.hop < 1:
                        raise ValueError(f"{group[b]}: {n} samples at {self.sr} Hz are too few")
                    if n // self.hop > K.ALIGN_MAX_MEL:
                        raise ValueError(f"{group[b]}: {n // self.hop} frames, the aligner takes "
                                         f"{K.ALIGN_MAX_MEL}")
                mel = self.front(wavs[:, :max(lens)].contiguous(), lens, clip=True)[0]
                for r, b in enumerate(rows):
                    f = lens[r] // self.hop
                    parts.append((g0 + b, mel[r, :, :f].t().contiguous()))
        parts.sort(key=lambda p: p[0])
        for _, m in parts:
            self.offset.append(total)
            self.frames.append(m.shape[0])
            total += m.shape[0]
        self.flat = torch.cat([m for _, m in parts]) if parts else \
            torch.zeros((0, self.front.n_mels), device=self.device)
        return self

    def gather(self, idx):
        """Padded ``(mels (B, T_m, n_mels), mel_lens (B) int64)`` of the utterances ``idx``."""
        T = max(self.frames[i] for i in idx)
        mels = K.zeros((len(idx), T, self.flat.shape[1]), self.device)
        for r, i in enumerate(idx):
            mels[r, :self.frames[i]] = self.flat[self.offset[i]:self.offset[i] + self.frames[i]]
        lens = torch.tensor([self.frames[i] for i in idx], dtype=torch.int64, device=self.device)
        return mels, lens


def _texts(ids, idx, device):
    T = max(len(ids[i]) for i in idx)
    texts = np.zeros((len(idx), T), np.int64)
    for r, i in enumerate(idx):
        texts[r, :len(ids[i])] = ids[i]
    lens = np.asarray([len(ids[i]) for i in idx], np.int64)
    return torch.from_numpy(texts).to(device), torch.from_numpy(lens).to(device)


def _masks(optional, idx, device):
    """The padded (B, T_s) uint8 mask of the utterances ``idx`` on the device."""
    T = max(len(optional[i]) for i in idx)
    mask = np.zeros((len(idx), T), np.uint8)
    for r, i in enumerate(idx):
        mask[r, :len(optional[i])] = optional[i]
    return torch.from_numpy(mask).to(device)


def align_corpus(config, steps=2000, batch=16, checkpoint=None, seed=0, device="cuda",
                 channels=64, attn_dim=40, save=None, optional_sil=None, edge_sil=True):
    """``config``: the merged dict ``Preprocessor`` takes.  Returns ``(written, left)``: the
    TextGrid paths written and those that existed and were left alone.  ``optional_sil``: the
    symbol of the optional pauses that ``|`` and (``edge_sil``) the utterance edges stand for, see
    ``parse_phn``; positions the alignment gives no frame are not written.  With ``optional_sil``
    a freshly trained aligner has its beta-binomial prior off (``omega = 0``, otherwise 1): with the
    prior the blank takes the silent frames and the pauses are omitted.  A loaded
    ``checkpoint`` keeps the omega it was saved with."""
    raw, pre = config["path"]["raw_path"], config["path"]["preprocessed_path"]
    table = {s: i for i, s in enumerate(symbol_table())}
    items, left = [], []
    for speaker in sorted(s for s in os.listdir(raw) if os.path.isdir(os.path.join(raw, s))):
        for wav_name in sorted(os.listdir(os.path.join(raw, speaker))):
            if ".wav" not in wav_name:
                continue
            basename = wav_name.split(".")[0]
            tg = os.path.join(pre, "TextGrid", speaker, f"{basename}.TextGrid")
            if os.path.exists(tg):
                left.append(tg)
                continue
            phn = os.path.join(raw, speaker, f"{basename}.phn")
            if optional_sil is None:
                (phones, ids), marks = parse_phn(phn, table), None
            else:
                phones, ids, marks = parse_phn(phn, table, optional_sil, edge_sil)
            if len(ids) > K.ALIGN_MAX_SRC:
                raise ValueError(f"{basename}.phn: {len(ids)} phonemes, the aligner takes "
                                 f"{K.ALIGN_MAX_SRC}")
            items.append((speaker, basename, phones, ids, tg, marks))
    if not items:
        print(f"align: wrote 0 TextGrids, left {len(left)}" +
              ("; pauses kept 0 of 0" if optional_sil is not None else ""))
        return [], left
    store = MelStore(config["preprocessing"], device, batch).build(
        [os.path.join(raw, it[0], f"{it[1]}.wav") for it in items])
    ids = [it[3] for it in items]
    marks = [it[5] for it in items] if optional_sil is not None else None
    for i, it in enumerate(items):
        need = len(ids[i]) - (sum(marks[i]) if marks is not None else 0)
        if store.frames[i] < need:
            raise ValueError(f"{it[1]}: {store.frames[i]} frames for {need} phonemes")
    torch.manual_seed(int(seed))
    model = Aligner(len(table), store.front.n_mels, channels, attn_dim, device)
    # with optional pauses the prior is off: it handicaps every label against the blank, which
    # then explains the silent frames, and the trained model omits the pauses
    trainer = AlignerTrainer(model) if marks is None else AlignerTrainer(model, omega=0.0)
    if checkpoint is not None:
        trainer.load(checkpoint)
    rng = np.random.default_rng(int(seed))

    def host_lens(idx):
        lens = [len(ids[i]) for i in idx], [store.frames[i] for i in idx]
        return lens if marks is None else lens + ([marks[i] for i in idx],)

    def mask(idx):
        return None if marks is None else _masks(marks, idx, store.device)

    for _ in range(0 if checkpoint is not None else int(steps)):
        idx = sorted(rng.choice(len(items), size=min(int(batch), len(items)), replace=False).tolist())
        texts, src_lens = _texts(ids, idx, store.device)
        mels, mel_lens = store.gather(idx)
        trainer.train_step(texts, src_lens, mels, mel_lens, host_lens(idx), mask(idx))
    if save is not None:
        trainer.save(save)
    written, kept, places = [], 0, 0
    for g0 in range(0, len(items), int(batch)):
        idx = list(range(g0, min(g0 + int(batch), len(items))))
        texts, src_lens = _texts(ids, idx, store.device)
        mels, mel_lens = store.gather(idx)
        dur = trainer.align(texts, src_lens, mels, mel_lens, host_lens(idx),
                            mask(idx)).cpu().numpy()
        for r, i in enumerate(idx):
            speaker, _, phones, _, tg, _ = items[i]
            d = dur[r, :len(phones)]
            if marks is not None:  # positions without a frame are no intervals
                live = d > 0
                kept += int(live[np.asarray(marks[i]) != 0].sum())
                places += int(sum(marks[i]))
                phones, d = [p for p, on in zip(phones, live) if on], d[live]
            os.makedirs(os.path.dirname(tg), exist_ok=True)
            write_textgrid(tg, phones, d, store.hop, store.sr)
            written.append(tg)
    line = f"align: wrote {len(written)} TextGrids, left {len(left)}"
    print(line if marks is None else f"{line}; pauses kept {kept} of {places}")
    return written, left


def main(argv=None):
    """``--config DIR [--corpus NAME]`` as ``preprocess.main`` reads them."""
    import argparse
    from pathlib import Path

    import yaml

    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, required=True, help="path to config")
    parser.add_argument("--corpus", type=str, default=None, help="corpus name")
    parser.add_argument("--steps", type=int, default=2000, help="aligner updates")
    parser.add_argument("--batch", type=int, default=16)
    parser.add_argument("--checkpoint", type=str, default=None,
                        help="a trained aligner (AlignerTrainer.save): align without training")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--optional_sil", type=str, default=None, metavar="SYMBOL",
                        help="'|' in a .phn line and the utterance edges are optional pauses of "
                             "this symbol (normally sp); training then runs without the "
                             "beta-binomial prior (omega 0 instead of 1), see DESIGN.md")
    parser.add_argument("--no_edge_sil", action="store_true",
                        help="with --optional_sil: no optional pause at the utterance edges")
    args = parser.parse_args(argv)
    with open(os.path.join(args.config, "preprocess.yaml")) as f:
        preprocess_config = yaml.safe_load(f)
    if args.corpus is not None:
        files = [Path(args.config) / f"preprocess_{args.corpus}.yaml"]
    else:
        files = sorted(Path(args.config).glob("preprocess_*.yaml"))
    out = []
    for path in files:
        with open(path) as f:
            config = yaml.safe_load(f)
        config["preprocessing"] = preprocess_config
        print("aligning...:", config["dataset"])
        out.append(align_corpus(config, args.steps, args.batch, args.checkpoint, args.seed,
                                optional_sil=args.optional_sil, edge_sil=not args.no_edge_sil))
    return out


if __name__ == "__main__":
    main()
