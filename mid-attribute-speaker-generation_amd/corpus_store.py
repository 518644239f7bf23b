"""The FastSpeech2 corpus resident on the device: ``dataset.Dataset`` / ``ConcatDataset`` read
once, every later batch cut from HBM by one kernel.

The host path (``dataset.py``) loads five ``.npy`` files per utterance for every batch, pads
with numpy and copies the padded batch to the device.  ``CorpusStore`` reads each utterance once
through the dataset's own ``__getitem__`` (so the z-normalisation and speaker re-mapping of
``ConcatDataset`` are the host code's), converts every field as ``to_device`` would and packs
each field into one flat device buffer.  ``CorpusBatcher`` reproduces the batch order of the
reference's loader (``train.py:56-63``, ``dataset.py:175-194``) as host arithmetic on the length
tables; per batch B int32 indices cross the bus and ``fs2_batch_gather`` writes the padded tuple.

Store layout (``n`` utterances in dataset order, utterance ``u``):

* ``text``, ``dur``, ``accent``: int64, ``src_len[u]`` entries at element ``src_off[u]``;
* ``mel``: fp32, ``mel_len[u] * n_mels`` entries at element ``mel_off[u]`` (a multiple of
  ``n_mels``, so every utterance starts on a 16-byte boundary);
* ``pitch`` fp32 and ``energy`` (fp32 or fp64, as the corpus holds it): one value per phoneme
  at ``src_off[u]``, or per frame at ``mel_off[u] // n_mels`` (``levels``);
* ``meta``: fp32 ``(n, meta_dim)``, the concatenated one-hot row of ``Dataset.reprocess``;
* the tables ``src_len``, ``mel_len`` (int32), ``src_off``, ``mel_off``, ``speaker`` (int64) on
  the host (numpy) and on the device (``d_*``); ``ids`` and ``raw_text`` stay host lists.
"""
import numpy as np
import torch

from . import kernels as K

STAGE_BYTES = 64 << 20  # pinned staging chunk of the corpus load
RING = 4                # descriptor buffers in flight
LEVEL_NAMES = ("phoneme_level", "frame_level")


def _collator(dataset):
    """The ``Dataset`` whose ``collate_fn`` pads the batches (the first one of a
    ``ConcatDataset``: its ``use_accent`` and metadata layout hold for every corpus)."""
    owner = getattr(dataset.collate_fn, "__self__", None)
    if owner is None or not hasattr(owner, "speaker_meta"):
        raise ValueError("CorpusStore needs a dataset.Dataset or dataset.ConcatDataset")
    return owner


def meta_row(layout, speaker_meta):
    """``dataset.py:123-126``: one one-hot per attribute, concatenated in the item's order."""
    return np.concatenate([np.eye(len(layout[m]))[layout[m][v]] for m, v in speaker_meta.items()])


def _level(name, n, src, mel, u):
    """The levels an ``n``-entry feature of utterance ``u`` can have: bit 0 phoneme, bit 1 frame."""
    ok = (1 if n == src else 0) | (2 if n == mel else 0)
    if not ok:
        raise ValueError(f"utterance {u}: {name} has {n} entries, neither its {src} phonemes "
                         f"nor its {mel} frames")
    return ok


def build_tables(samples, layout, levels=None):
    """The host half of the store: ``samples`` (an iterable of ``Dataset.__getitem__`` dicts, read
    once) -> ``(tables, fields)``.

    ``tables``: ``src_len``, ``mel_len`` (int32), ``src_off``, ``mel_off``, ``speaker`` (int64),
    ``levels`` = (pitch is frame-level, energy is frame-level), ``n_mels``, ``energy_dtype``,
    ``ids``, ``raw_text``.  ``fields``: per field the list of converted arrays (``text``,
    ``dur``, ``accent`` int64; ``mel``, ``pitch`` fp32; ``energy`` as it arrives; ``meta`` fp32).

    A feature's level is read off the arrays: its length is the utterance's phoneme count or its
    frame count, the same choice for the whole corpus.  ``levels`` (``loss.feature_levels``)
    must agree with them and decides where every utterance has as many frames as phonemes.
    ``ValueError``: no single level fits, it contradicts ``levels``, or the energy's dtype is not
    fp32 or fp64 throughout."""
    names = ("text", "dur", "accent", "mel", "pitch", "energy", "meta")
    fields = {k: [] for k in names}
    src_len, mel_len, speaker, ids, raw = [], [], [], [], []
    can = [3, 3]  # levels still possible for (pitch, energy)
    n_mels = e_dtype = None
    for u, d in enumerate(samples):
        text = np.asarray(d["text"]).astype(np.int64, copy=False)
        mel = np.asarray(d["mel"])
        if mel.ndim != 2 or (n_mels is not None and mel.shape[1] != n_mels):
            raise ValueError(f"utterance {u} ({d['id']}): mel of shape {mel.shape}")
        n_mels = mel.shape[1]
        L, M = int(text.shape[0]), int(mel.shape[0])
        dur, acc = np.asarray(d["duration"]), np.asarray(d["accent"])
        if dur.shape != (L,) or acc.shape != (L,):
            raise ValueError(f"utterance {u} ({d['id']}): {L} phonemes, {dur.shape[0]} durations, "
                             f"{acc.shape[0]} accents")
        pitch, energy = np.asarray(d["pitch"]), np.asarray(d["energy"])
        if e_dtype is None:
            e_dtype = energy.dtype
        if energy.dtype != e_dtype or e_dtype not in (np.float32, np.float64):
            raise ValueError(f"utterance {u} ({d['id']}): energy is {energy.dtype}, the corpus "
                             f"so far {e_dtype}; it must be float32 or float64 throughout")
        for k, (name, a) in enumerate((("pitch", pitch), ("energy", energy))):
            can[k] &= _level(name, a.shape[0] if a.ndim == 1 else -1, L, M, u)
            if not can[k]:
                raise ValueError(f"utterance {u} ({d['id']}): {name} has {a.shape[0]} entries; "
                                 "earlier utterances fix the other feature level (one level per "
                                 "feature for the whole corpus)")
        fields["text"].append(text)
        fields["dur"].append(dur.astype(np.int64, copy=False))
        fields["accent"].append(acc.astype(np.int64, copy=False))
        fields["mel"].append(mel.astype(np.float32, copy=False))
        fields["pitch"].append(pitch.astype(np.float32))  # after normalisation, as .float()
        fields["energy"].append(energy)
        fields["meta"].append(meta_row(layout, d["speaker_meta"]).astype(np.float32))
        src_len.append(L)
        mel_len.append(M)
        speaker.append(int(d["speaker"]))
        ids.append(d["id"])
        raw.append(d["raw_text"])
    if not ids:
        raise ValueError("CorpusStore: the dataset is empty")
    found = []
    for k, name in enumerate(("pitch", "energy")):
        if levels is not None and not can[k] & (2 if levels[k] else 1):
            raise ValueError(f"{name} is stored {LEVEL_NAMES[can[k] == 2]} but the preprocess "
                             f"config asks for {LEVEL_NAMES[bool(levels[k])]}")
        found.append(bool(levels[k]) if levels is not None else can[k] == 2)
    src_len, mel_len = np.asarray(src_len, np.int32), np.asarray(mel_len, np.int32)
    off = lambda n: np.concatenate([[0], np.cumsum(n.astype(np.int64))[:-1]]).astype(np.int64)
    tables = dict(src_len=src_len, mel_len=mel_len, src_off=off(src_len),
                  mel_off=off(mel_len) * n_mels, speaker=np.asarray(speaker, np.int64),
                  levels=tuple(found), n_mels=int(n_mels), energy_dtype=np.dtype(e_dtype),
                  ids=ids, raw_text=raw)
    return tables, fields


class DeviceBatch(tuple):
    """A gathered batch tuple that remembers where it came from: ``regather(max_src_len,
    max_mel_len)`` cuts the same utterances again padded to other lengths (what
    ``Trainer._agree_lengths`` asks for under data parallelism)."""
    store = indices = desc = None

    def regather(self, max_src_len, max_mel_len):
        return self.store.gather(self.indices, max_src_len, max_mel_len, desc=self.desc)


class CorpusStore:
    """``CorpusStore(dataset, device="cuda")``: see the module docstring.  ``levels``: the
    ``loss.feature_levels`` of the preprocess config, checked against the arrays.  A corpus
    larger than the free device memory raises ``MemoryError`` with both byte counts."""

    def __init__(self, dataset, device="cuda", levels=None):
        owner = _collator(dataset)
        self.device = torch.device(device)
        self.use_accent = bool(owner.use_accent)
        self.n_tuple = 14 if self.use_accent else 13
        t, fields = build_tables((dataset[i] for i in range(len(dataset))), owner.speaker_meta,
                                 levels)
        self.src_len, self.mel_len = t["src_len"], t["mel_len"]
        self.src_off, self.mel_off, self.speaker = t["src_off"], t["mel_off"], t["speaker"]
        self.levels, self.n_mels = t["levels"], t["n_mels"]
        self.ids, self.raw_text = t["ids"], t["raw_text"]
        self.meta_dim = int(fields["meta"][0].shape[0])
        self.nbytes = sum(a.nbytes for v in fields.values() for a in v) + 32 * len(self.ids)
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            if self.nbytes > free:
                raise MemoryError(f"CorpusStore: the corpus takes {self.nbytes} bytes, the device "
                                  f"has {free} bytes free; there is no host fallback")
        for name in ("text", "dur", "accent", "mel", "pitch", "energy", "meta"):
            setattr(self, name, self._upload(fields.pop(name)))
        self.meta = self.meta.view(len(self.ids), self.meta_dim)
        for name in ("src_len", "mel_len", "src_off", "mel_off", "speaker"):
            setattr(self, "d_" + name, self._upload([getattr(self, name)]))
        self._ring = [None] * RING
        self._slot = 0

    def __len__(self):
        return len(self.ids)

    def _upload(self, arrays):
        """The arrays end to end in one flat buffer on the device, through a pinned staging
        chunk guarded by an event (the corpus never exists twice in pinned memory)."""
        dtype = arrays[0].dtype
        total = sum(a.size for a in arrays)
        tdt = torch.from_numpy(np.empty(0, dtype)).dtype
        if self.device.type != "cuda":
            return torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays]))
        dst = torch.empty(total, dtype=tdt, device=self.device)
        cap = max(1, min(total, STAGE_BYTES // dtype.itemsize))
        stage = torch.empty(cap, dtype=tdt, pin_memory=True)
        host, done, busy = stage.numpy(), torch.cuda.Event(), False
        pos = fill = 0  # elements already sent, elements waiting in the stage

        def flush():
            nonlocal pos, fill, busy
            dst[pos:pos + fill].copy_(stage[:fill], non_blocking=True)
            done.record()
            pos, fill, busy = pos + fill, 0, True

        for a in arrays:
            flat = a.reshape(-1)
            lo = 0
            while lo < flat.shape[0]:
                if busy:
                    done.synchronize()  # the previous copy still reads the stage
                    busy = False
                n = min(cap - fill, flat.shape[0] - lo)
                host[fill:fill + n] = flat[lo:lo + n]
                fill, lo = fill + n, lo + n
                if fill == cap:
                    flush()
        if fill:
            flush()
        done.synchronize()
        return dst

    # ------------------------------------------------------------------ batches
    def maxima(self, indices):
        idx = np.asarray(indices, np.int64)
        return int(self.src_len[idx].max()), int(self.mel_len[idx].max())

    def _descriptor(self, idx):
        """One asynchronous copy of the B int32 indices from a ring of pinned buffers, each
        guarded by an event (rewritten only after the copy out of it has finished)."""
        n = idx.shape[0]
        slot = self._ring[self._slot]
        if slot is None or slot[0].numel() < n:
            if slot is not None:
                slot[1].synchronize()
            slot = (torch.empty(max(n, 64), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
            self._ring[self._slot] = slot
        else:
            slot[1].synchronize()  # the copy issued RING batches ago
        self._slot = (self._slot + 1) % RING
        slot[0].numpy()[:n] = idx
        dev = torch.empty(n, dtype=torch.int32, device=self.device)
        dev.copy_(slot[0][:n], non_blocking=True)
        slot[1].record()
        return dev

    def gather(self, indices, max_src_len=None, max_mel_len=None, out=None, desc=None):
        """The batch tuple ``to_device(dataset.collate_fn([dataset[i] for i in indices])[0])``
        would give (rows in the order of ``indices``), cut on the device.

        ``max_src_len`` / ``max_mel_len``: pad to these instead of the group's own maxima (not
        below them).  ``out``: a tuple this method returned; its tensors are written in place
        and returned, so the batch is padded to THEIR lengths (a captured step's static inputs
        are filled without a copy; stale contents do not survive: every element is written)."""
        idx = np.ascontiguousarray(np.asarray(indices, np.int64).astype(np.int32))
        if idx.ndim != 1 or idx.size < 1:
            raise ValueError("gather: a batch needs at least one utterance index")
        if idx.min() < 0 or idx.max() >= len(self):
            raise IndexError(f"gather: index outside 0..{len(self) - 1}")
        if self.device.type != "cuda":
            raise RuntimeError("CorpusStore.gather needs the store on the GPU (no CPU path exists)")
        ts, tm = self.maxima(idx)
        outs = None
        if out is not None:
            if len(out) != self.n_tuple:
                raise ValueError(f"gather: out is a {len(out)}-tuple, the store yields {self.n_tuple}")
            max_src_len, max_mel_len = out[3].shape[1], out[6].shape[1]
            outs = (out[2], out[3], out[4], out[6], out[7], out[9], out[10], out[11], out[12],
                    out[13] if self.use_accent else None)
        ts = ts if max_src_len is None else int(max_src_len)
        tm = tm if max_mel_len is None else int(max_mel_len)
        if desc is None:
            desc = self._descriptor(idx)
        spk, texts, sl, mels, ml, pit, ene, dur, meta, acc = K.batch_gather(
            self, desc, idx, ts, tm, accents=self.use_accent, out=outs)
        batch = ([self.ids[i] for i in idx], [self.raw_text[i] for i in idx], spk, texts, sl, ts,
                 mels, ml, tm, pit, ene, dur, meta) + ((acc,) if self.use_accent else ())
        batch = DeviceBatch(batch)
        batch.store, batch.indices, batch.desc = self, idx, desc
        return batch


class CorpusBatcher:
    """The index groups of ``DataLoader(dataset, batch_size=batch_size * group_size,
    shuffle=True, collate_fn=dataset.collate_fn, generator=g)`` with ``Dataset(sort,
    drop_last)`` (``train.py:56-63``, ``dataset.py:175-194``), computed on the host tables:

    * per epoch the loader's iterator draws its base seed from the generator, then the
      ``RandomSampler`` its permutation (``generator=None``: the sampler seeds a generator of
      its own from torch's global one, as the loader does); at the end of an epoch the
      sampler's closing (empty) ``randperm`` is drawn too, so a second epoch stays in step;
    * chunks of ``batch_size * group_size``, the last one short;
    * inside a chunk ``np.argsort(-text_lens)`` (the same call on the same values);
    * groups of ``batch_size``; the chunk's tail dropped or kept per ``drop_last``.

    ``shuffle=False, sort=False, drop_last=False, group_size=1`` is ``evaluate.py``'s loader.
    ``world > 1``: a group is ``world * batch_size`` utterances and rank ``rank`` takes its
    contiguous rows of it, ``nn.DataParallel``'s split (``torch.chunk``: ceil(rows / world) per
    rank; a rank whose share of a short tail is empty skips it).

    ``groups()`` yields one epoch's index lists (host only); iterating the batcher yields the
    gathered device tuples.  ``len(batcher)`` is the number of groups of an epoch."""

    def __init__(self, store, batch_size, group_size=4, shuffle=True, sort=True, drop_last=True,
                 generator=None, rank=0, world=1):
        if batch_size < 1 or group_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("CorpusBatcher: batch_size, group_size >= 1, 0 <= rank < world")
        self.store, self.batch_size, self.group_size = store, int(batch_size), int(group_size)
        self.shuffle, self.sort, self.drop_last = bool(shuffle), bool(sort), bool(drop_last)
        self.generator, self.rank, self.world = generator, int(rank), int(world)

    def _split(self, order):
        """One epoch's groups (global, before the rank split) of a sample order."""
        n, gb = len(order), self.batch_size * self.world
        step = gb * self.group_size
        for lo in range(0, n, step):
            chunk = np.asarray(order[lo:lo + step], np.int64)
            if self.sort:
                chunk = chunk[np.argsort(-self.store.src_len[chunk].astype(np.int64))]
            cut = len(chunk) - len(chunk) % gb
            for g in chunk[:cut].reshape(-1, gb).tolist():
                yield g
            if not self.drop_last and cut < len(chunk):
                yield chunk[cut:].tolist()

    def _mine(self, group):
        size = -(-len(group) // self.world)
        return group[self.rank * size:(self.rank + 1) * size]

    def __len__(self):
        return sum(1 for g in self._split(list(range(len(self.store)))) if self._mine(g))

    def groups(self):
        n = len(self.store)
        # the loader iterator's base seed (drawn for every epoch, shuffled or not)
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)
        gen = None
        if self.shuffle:
            gen = self.generator
            if gen is None:
                gen = torch.Generator()
                gen.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            order = torch.randperm(n, generator=gen).tolist()
        else:
            order = list(range(n))
        for g in self._split(order):
            g = self._mine(g) if self.world > 1 else g
            if g:
                yield g
        if gen is not None:
            torch.randperm(n, generator=gen)  # RandomSampler's closing draw (num_samples % n)

    def __iter__(self):
        for g in self.groups():
            yield self.store.gather(g)
