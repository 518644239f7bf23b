"""The data path of the speaker encoder: ``data_load.py``'s ``SpeakerDataset`` + ``Collate`` of
``Multilingual-Speaker-Encoder-with-Domain-Adaptation`` with the corpus resident on the device.

``SpeakerStore`` loads the reference's preprocessed files (``<dataset>_<spkr>_<gender>_
<language>.npy``, each ``(utterances, 80, frames)`` fp32; data_preprocess.py:22,86-88) once into
one flat device buffer.  ``SpeakerBatcher`` draws a batch the way ``DataLoader(SpeakerDataset(),
batch_size=N, shuffle=False, num_workers=0, drop_last=True, collate_fn=Collate(True))`` does --
the same calls of Python's ``random`` module on the same populations in the same order -- but
only as row descriptors (file, utterance, crop start); ``fs2_mel_crop_gather`` then cuts, transposes and
stacks the rows on the device.  The reference slices, transposes, stacks and copies ~15 MB per
batch on the host; here 20 bytes per row cross the bus.
"""
import glob
import os
import random as _random

import numpy as np
import torch

from . import kernels as K

NMELS = 80
STAGE_BYTES = 64 << 20  # pinned staging chunk of the corpus load
RING = 4                # descriptor buffers in flight


def decode_filename(name):
    """data_load.py:84-88."""
    d, s, g, l = os.path.basename(name)[:-4].split("_")
    return {"dataset": d, "spkr": s, "gender": g, "language": l}


class SpeakerStore:
    """Every utterance of every speaker file in one flat fp32 buffer on ``device``.

    ``file_list=None`` takes the files of each dataset (``<dataset.lower()>*.npy``) in sorted
    order.  The reference takes them in ``glob`` order, which depends on the file system; pass
    the list a reference run saw (base names) to reproduce its draws exactly.  Languages are
    sorted (data_load.py:59-61).  A file with fewer than ``tisv_frame`` frames raises
    ``ValueError`` here (the reference fails at whichever later batch first crops it).

    Per file ``k``: ``utt_count[k]``, ``frames[k]`` and ``offset[k]`` (elements); utterance ``u``
    is the ``(n_mels, frames[k])`` block at ``offset[k] + u * n_mels * frames[k]``.
    """

    def __init__(self, path, datasets=("JVS", "VCTK"), device="cuda", file_list=None,
                 tisv_frame=150, da_on="language"):
        self.path, self.tisv_frame, self.da_on = path, int(tisv_frame), da_on
        self.device = torch.device(device)
        if file_list is None:
            file_list = []
            for d in datasets:
                pat = os.path.join(path, "{}*.npy".format(d.lower()))
                file_list.extend(sorted(os.path.basename(f) for f in glob.glob(pat)))
        self.files = list(file_list)
        if not self.files:
            raise ValueError(f"no speaker files of {tuple(datasets)} under {path}")
        self.lang2files = {}
        for k, f in enumerate(self.files):
            self.lang2files.setdefault(decode_filename(f)[da_on], []).append(k)
        self.langs = sorted(self.lang2files)
        self.file_lang = [self.langs.index(decode_filename(f)[da_on]) for f in self.files]
        self.utt_count, self.frames, self.offset = [], [], []
        total, self.n_mels = 0, None
        for f in self.files:
            a = np.load(os.path.join(path, f), mmap_mode="r")
            if a.ndim != 3 or a.dtype != np.float32:
                raise ValueError(f"{f}: expected fp32 (utterances, n_mels, frames), got "
                                 f"{a.dtype} {a.shape}")
            u, c, t = a.shape
            if self.n_mels is None:
                self.n_mels = c
            if c != self.n_mels or u < 1:
                raise ValueError(f"{f}: {c} mel channels / {u} utterances (others: {self.n_mels})")
            if t < self.tisv_frame:
                raise ValueError(f"{f}: {t} frames, fewer than tisv_frame = {self.tisv_frame}")
            self.utt_count.append(u)
            self.frames.append(t)
            self.offset.append(total)
            total += u * c * t
            del a
        self.numel = total
        self.data = torch.empty(total, dtype=torch.float32, device=self.device)
        self._load()

    def _load(self):
        cuda = self.device.type == "cuda"
        chunk = STAGE_BYTES // 4
        stage = torch.empty(min(chunk, max(n * self.n_mels * t for n, t in
                                           zip(self.utt_count, self.frames))),
                            dtype=torch.float32, pin_memory=cuda)
        done, busy = (torch.cuda.Event() if cuda else None), False
        for k, f in enumerate(self.files):
            flat = np.load(os.path.join(self.path, f), mmap_mode="r").reshape(-1)
            for lo in range(0, flat.shape[0], stage.numel()):
                hi = min(lo + stage.numel(), flat.shape[0])
                if busy:
                    done.synchronize()  # the staging buffer is read by the previous copy
                busy = cuda
                stage.numpy()[:hi - lo] = flat[lo:hi]
                dst = self.data[self.offset[k] + lo:self.offset[k] + hi]
                dst.copy_(stage[:hi - lo], non_blocking=True)
                if cuda:
                    done.record()
        if cuda:
            done.synchronize()

    def __len__(self):
        return len(self.files)


class SpeakerBatcher:
    """``next_batch()`` -> ``(mels (n_spk * n_utt, L, n_mels), langs (n_spk * n_utt))`` on the
    device, speaker-major, as ``EmbedderTrainer.train_step`` takes them.

    ``rng`` (default: the ``random`` module itself, as in the reference) supplies ``sample``,
    ``choices``, ``randint`` and ``shuffle``.  Per batch, for item ``idx`` of the epoch:
    ``sample(files_of_lang[idx % n_langs], 1)``, then ``choices(range(U), k=M)`` if ``M > U``
    else ``sample(range(U), M)``; after the items ``randint(lower, tisv_frame)`` for the length
    and one ``randint(0, min(frames, tisv_frame) - L)`` per speaker; with ``consume_shuffle`` one
    ``shuffle`` of an ``n_spk * n_utt`` list follows (train_speech_embedder.py:160-161: the
    embedder treats rows independently, so the permutation is drawn, to stay in step with the
    reference's generator, and not applied).  An epoch has ``len(store) // n_spk`` batches.

    ``draw()`` is the host half alone (no device work).  The descriptors of a batch go to the
    device in one asynchronous copy from a small ring of pinned buffers, each guarded by an
    event, so a buffer is rewritten only after the copy out of it has finished and no batch
    waits for the device.
    """

    def __init__(self, store, n_spk, n_utt, variable_length=True, sr=22050, hop=256,
                 consume_shuffle=True, rng=None):
        self.store, self.n_spk, self.n_utt = store, int(n_spk), int(n_utt)
        self.variable_length, self.consume_shuffle = bool(variable_length), bool(consume_shuffle)
        self.rng = rng if rng is not None else _random
        self.tisv_frame = store.tisv_frame
        self.lower = int(self.tisv_frame - 0.4 / hop * sr)  # data_load.py:118
        self.batches_per_epoch = len(store) // self.n_spk
        if self.batches_per_epoch < 1:
            raise ValueError(f"{len(store)} files give no batch of {self.n_spk} speakers")
        self._item = 0
        self._ring = [None] * RING
        self._slot = 0

    # ------------------------------------------------------------------ host draws
    def _utterances(self, k, m):
        u = range(self.store.utt_count[k])
        return self.rng.choices(u, k=m) if m > len(u) else self.rng.sample(u, m)

    def _collate(self, files):
        frames = [min(self.store.frames[k], self.tisv_frame) for k in files]
        if not self.variable_length:
            if len(set(frames)) != 1:
                raise ValueError("variable_length=False needs equal frame counts")
            return frames[0], [0] * len(files)
        length = self.rng.randint(self.lower, self.tisv_frame)
        return length, [self.rng.randint(0, t - length) for t in frames]

    def draw(self):
        """The next batch as host descriptors: ``{"files", "utts" (n_spk, n_utt), "length",
        "starts" (n_spk), "langs" (n_spk)}``."""
        st, files, utts, langs = self.store, [], [], []
        for _ in range(self.n_spk):
            lang = self._item % len(st.langs)
            k = self.rng.sample(st.lang2files[st.langs[lang]], 1)[0]
            files.append(k)
            langs.append(lang)
            utts.append(self._utterances(k, self.n_utt))
            self._item += 1
        if self._item >= self.batches_per_epoch * self.n_spk:
            self._item = 0  # drop_last, then the sampler starts over
        length, starts = self._collate(files)
        if self.consume_shuffle:
            self.rng.shuffle(list(range(self.n_spk * self.n_utt)))
        return {"files": files, "utts": utts, "length": length, "starts": starts, "langs": langs}

    def draw_speaker(self, file_index, utter_num=400):
        """get_spkr2embedding's batch (train_speech_embedder.py:289-295): file ``file_index``,
        ``shuffle=False``, ``utter_num`` utterances, the same collate, no batch shuffle."""
        utts = self._utterances(file_index, int(utter_num))
        length, starts = self._collate([file_index])
        return {"files": [file_index], "utts": [utts], "length": length, "starts": starts,
                "langs": [self.store.file_lang[file_index]]}

    # ------------------------------------------------------------------ device half
    def rows(self, d):
        """Host descriptor arrays of a draw: (row_off i64, row_stride i32, row_start i32,
        langs f32), one entry per row, speaker-major."""
        st = self.store
        off, stride, start, langs = [], [], [], []
        for k, us, p, lang in zip(d["files"], d["utts"], d["starts"], d["langs"]):
            t = st.frames[k]
            if p < 0 or p + d["length"] > t:
                raise ValueError(f"crop {p}+{d['length']} outside {t} frames of {st.files[k]}")
            for u in us:
                if not 0 <= u < st.utt_count[k]:
                    raise ValueError(f"utterance {u} outside {st.files[k]}")
                off.append(st.offset[k] + u * st.n_mels * t)
                stride.append(t)
                start.append(p)
                langs.append(lang)
        return (np.asarray(off, np.int64), np.asarray(stride, np.int32),
                np.asarray(start, np.int32), np.asarray(langs, np.float32))

    def _upload(self, off, stride, start, langs):
        """One async H2D copy of the four arrays; returns their device views."""
        n = off.shape[0]
        nbytes = 20 * n
        dev = self.store.device
        slot = self._ring[self._slot]
        if slot is None or slot[0].numel() < nbytes:
            if slot is not None:
                slot[1].synchronize()
            slot = (torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
            self._ring[self._slot] = slot
        else:
            slot[1].synchronize()  # the copy issued RING batches ago; long finished
        self._slot = (self._slot + 1) % RING
        host = slot[0].numpy()
        host[:8 * n].view(np.int64)[:] = off
        host[8 * n:12 * n].view(np.int32)[:] = stride
        host[12 * n:16 * n].view(np.int32)[:] = start
        host[16 * n:20 * n].view(np.float32)[:] = langs
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        buf.copy_(slot[0][:nbytes], non_blocking=True)
        slot[1].record()
        return (buf[:8 * n].view(torch.int64), buf[8 * n:12 * n].view(torch.int32),
                buf[12 * n:16 * n].view(torch.int32), buf[16 * n:20 * n].view(torch.float32))

    def gather(self, d):
        off, stride, start, langs = self._upload(*self.rows(d))
        mels = K.mel_crop_gather(self.store.data, off, stride, start, self.store.n_mels,
                                 d["length"])
        return mels, langs

    def next_batch(self):
        return self.gather(self.draw())

    def speaker_batch(self, file_index, utter_num=400):
        """``(mels (utter_num, L, n_mels), langs (utter_num))`` of one file."""
        return self.gather(self.draw_speaker(file_index, utter_num))
