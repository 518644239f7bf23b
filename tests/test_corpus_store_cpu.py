"""The device-resident FastSpeech2 corpus, the parts that need no GPU: the batcher's order
against ``torch.utils.data.DataLoader`` itself, the store's host tables, and the C-ABI of the
two new entry points."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from corpus_store_helpers import corpora_at, datasets, set_level  # noqa: E402

PKG = "mid-attribute-speaker-generation_amd"
C = importlib.import_module(PKG + ".corpus_store")
D = importlib.import_module(PKG + ".dataset")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return corpora_at(str(tmp_path_factory.mktemp("corpus_store_cpu")))


@pytest.fixture(scope="module")
def store(corpus):
    return C.CorpusStore(datasets(corpus), device="cpu")


# ------------------------------------------------------------------ batcher order
def _loader_ids(concat, batch_size, group_size, drop_last, seed, shuffle=True, epochs=2):
    """The id lists of the reference's loader (train.py:56-63) over ``epochs`` epochs."""
    for d in concat.datasets:
        d.batch_size, d.drop_last = batch_size, drop_last
    g = torch.Generator()
    g.manual_seed(seed)
    loader = torch.utils.data.DataLoader(concat, batch_size=batch_size * group_size,
                                         shuffle=shuffle, collate_fn=concat.collate_fn, generator=g)
    return [[list(b[0]) for batchs in loader for b in batchs] for _ in range(epochs)]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("batch_size,group_size", [(2, 4), (3, 2), (24, 1)])
@pytest.mark.parametrize("drop_last", [True, False])
def test_batcher_order_is_the_loaders(corpus, store, seed, batch_size, group_size, drop_last):
    concat = datasets(corpus, sort=True, drop_last=drop_last)
    want = _loader_ids(concat, batch_size, group_size, drop_last, seed)
    g = torch.Generator()
    g.manual_seed(seed)
    b = C.CorpusBatcher(store, batch_size, group_size, drop_last=drop_last, generator=g)
    got = [[[store.ids[i] for i in grp] for grp in b.groups()] for _ in range(2)]
    assert got == want  # the second epoch too: the generator stays in step with the loader's
    assert len(b) == len(want[0]) > 0


def test_batcher_without_a_generator_follows_the_global_one(corpus, store):
    concat = datasets(corpus, sort=True, drop_last=True)
    for d in concat.datasets:
        d.batch_size = 3
    torch.manual_seed(5)
    loader = torch.utils.data.DataLoader(concat, batch_size=6, shuffle=True,
                                         collate_fn=concat.collate_fn)
    want = [list(b[0]) for batchs in loader for b in batchs]
    torch.manual_seed(5)
    got = [[store.ids[i] for i in g] for g in C.CorpusBatcher(store, 3, 2).groups()]
    assert got == want


def test_evaluate_setting_is_file_order(corpus, store):
    concat = datasets(corpus, sort=False, drop_last=False)
    want = _loader_ids(concat, 4, 1, False, 0, shuffle=False, epochs=1)[0]
    b = C.CorpusBatcher(store, 4, group_size=1, shuffle=False, sort=False, drop_last=False)
    groups = list(b.groups())
    assert [[store.ids[i] for i in g] for g in groups] == want
    assert [i for g in groups for i in g] == list(range(len(store)))
    assert [len(g) for g in groups] == [4] * 6  # 24 utterances


@pytest.mark.parametrize("drop_last", [True, False])
def test_world_2_hands_each_rank_its_contiguous_half(store, drop_last):
    def run(**kw):
        g = torch.Generator()
        g.manual_seed(3)
        return list(C.CorpusBatcher(store, 2, 2, drop_last=drop_last, generator=g, **kw).groups())
    # the global groups: one process with the global batch of world * batch_size
    g = torch.Generator()
    g.manual_seed(3)
    glob = list(C.CorpusBatcher(store, 4, 2, drop_last=drop_last, generator=g).groups())
    r0, r1 = run(rank=0, world=2), run(rank=1, world=2)
    assert len(r0) == len(r1) == len(glob)
    for whole, a, b in zip(glob, r0, r1):
        half = -(-len(whole) // 2)  # torch.chunk, nn.DataParallel's scatter
        assert a == whole[:half] and b == whole[half:]
        assert [x.tolist() for x in torch.tensor(whole).chunk(2)] == [a, b]


# ------------------------------------------------------------------ host tables
def test_store_tables_and_fields(corpus, store):
    concat = datasets(corpus)
    n = len(concat)
    assert len(store) == n == 24 and store.n_tuple == 14 and store.use_accent
    assert store.levels == (False, False) and store.n_mels == 80 and store.meta_dim == 4
    items = [concat[i] for i in range(n)]
    assert store.src_len.dtype == store.mel_len.dtype == np.int32
    assert store.src_len.tolist() == [len(d["text"]) for d in items]
    assert store.mel_len.tolist() == [d["mel"].shape[0] for d in items]
    assert store.src_off.tolist() == np.concatenate([[0], np.cumsum(store.src_len)[:-1]]).tolist()
    assert store.mel_off.tolist() == (80 * np.concatenate([[0], np.cumsum(store.mel_len)[:-1]])).tolist()
    assert store.speaker.tolist() == [d["speaker"] for d in items]
    assert store.ids == [d["id"] for d in items] and store.raw_text == [d["raw_text"] for d in items]
    assert (store.text.dtype, store.dur.dtype, store.accent.dtype, store.mel.dtype, store.pitch.dtype,
            store.energy.dtype, store.meta.dtype) == (torch.int64,) * 3 + (torch.float32,) * 4
    for name in ("src_len", "mel_len", "src_off", "mel_off", "speaker"):
        assert np.array_equal(getattr(store, "d_" + name).numpy(), getattr(store, name))
    for u in (0, 12, 13, n - 1):  # first, the corpus boundary, last
        d, so, mo = items[u], int(store.src_off[u]), int(store.mel_off[u])
        L, M = len(d["text"]), d["mel"].shape[0]
        assert np.array_equal(store.text[so:so + L].numpy(), d["text"])
        assert np.array_equal(store.dur[so:so + L].numpy(), d["duration"])
        assert np.array_equal(store.accent[so:so + L].numpy(), d["accent"])
        assert np.array_equal(store.mel[mo:mo + M * 80].numpy().reshape(M, 80), d["mel"])
        assert np.array_equal(store.pitch[so:so + L].numpy(), d["pitch"].astype(np.float32))
        assert np.array_equal(store.energy[so:so + L].numpy(), d["energy"])
        row = concat.collate_fn.__self__.reprocess([d], [0])[12][0]
        assert np.array_equal(store.meta[u].numpy(), row.astype(np.float32))
    assert store.text.numel() == store.src_len.sum() and store.mel.numel() == 80 * store.mel_len.sum()


def test_tuple_length_follows_the_first_dataset(corpus):
    en_first = C.CorpusStore(datasets(corpus, order=(1, 0)), device="cpu")
    assert en_first.n_tuple == 13 and not en_first.use_accent
    assert en_first.ids[0].startswith("en") and en_first.meta_dim == 4


def test_frame_level_is_read_off_the_arrays(tmp_path):
    corpus = corpora_at(str(tmp_path))
    set_level(corpus, "pitch", "frame_level")
    st = C.CorpusStore(datasets(corpus), device="cpu")
    assert st.levels == (True, False)
    assert st.pitch.numel() == st.mel_len.sum() and st.energy.numel() == st.src_len.sum()
    assert C.CorpusStore(datasets(corpus), device="cpu", levels=(True, False)).levels == (True, False)
    with pytest.raises(ValueError, match="pitch is stored frame_level"):
        C.CorpusStore(datasets(corpus), device="cpu", levels=(False, False))


def test_mixed_levels_and_mixed_energy_dtypes_raise(tmp_path):
    corpus = corpora_at(str(tmp_path))
    set_level(corpus, "energy", "frame_level", only=(1,))  # the EN corpus alone
    with pytest.raises(ValueError, match="one level per feature"):
        C.CorpusStore(datasets(corpus), device="cpu")
    corpus = corpora_at(str(tmp_path / "b"))
    set_level(corpus, "energy", "phoneme_level", only=(1,), dtype=np.float64)
    with pytest.raises(ValueError, match="float32 or float64 throughout"):
        C.CorpusStore(datasets(corpus), device="cpu")
    corpus = corpora_at(str(tmp_path / "c"))
    set_level(corpus, "energy", "phoneme_level", dtype=np.float64)
    st = C.CorpusStore(datasets(corpus), device="cpu")
    assert st.energy.dtype == torch.float64  # ConcatDataset's normalisation keeps fp64


def test_gather_needs_the_gpu_and_valid_indices(store):
    with pytest.raises(RuntimeError, match="no CPU path"):
        store.gather([0, 1])
    with pytest.raises(IndexError):
        store.gather([0, len(store)])
    with pytest.raises(ValueError):
        store.gather([])


# ------------------------------------------------------------------ C-ABI
NEW = {
    "fs2_batch_gather": (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int64] * 2 +
                         [ctypes.c_void_p] * 14 + [ctypes.c_int64] * 7 + [ctypes.c_void_p] * 11),
    "fs2_eval_accum": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_void_p]),
}


def test_header_declares_and_binding_matches():
    L = importlib.import_module(PKG + "._lib")
    src = re.sub(r"/\*.*?\*/", " ", open(f"{REPO}/include/fs2hip.h").read(), flags=re.S)
    sigs = L.parse_header()
    L.lib.load()
    for name, (res, args) in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert sigs[name] == (res, args), name
        fn = getattr(L.lib._dll, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the wrappers pass one argument per declared parameter
    ksrc = open(f"{REPO}/{PKG}/kernels.py").read()
    for name, (_, args) in NEW.items():
        call = re.search(r"lib\." + name + r"\((.*?)\)\n", ksrc, flags=re.S).group(1)
        depth, count = 0, 1
        for ch in call:
            depth += ch in "(["
            depth -= ch in ")]"
            count += ch == "," and depth == 0
        assert count == len(args), (name, count, len(args))


def _gather_args(**kw):
    """Placeholder arguments of fs2_batch_gather (p: non-null, never dereferenced by the checks
    that are expected to fail; the host tables are real)."""
    p = 64
    idx = np.array([0, 2], np.int32)
    src, mel = np.array([3, 9, 5], np.int32), np.array([10, 40, 20], np.int32)
    a = dict(idx=p, idx_host=idx.ctypes.data, batch=2, n_utt=3, src_len_host=src.ctypes.data,
             mel_len_host=mel.ctypes.data, src_len=p, mel_len=p, src_off=p, mel_off=p, speaker=p,
             text=p, dur=p, accent=p, mel=p, pitch=p, energy=p, meta=p, n_mels=80, meta_dim=4,
             energy_bytes=4, pitch_frame=0, energy_frame=0, max_src_len=5, max_mel_len=20,
             o_text=p, o_dur=p, o_accent=p, o_mel=p, o_pitch=p, o_energy=p, o_src_len=p,
             o_mel_len=p, o_speaker=p, o_meta=p, stream=0)
    a.update(kw)
    return list(a.values()), (idx, src, mel)


@pytest.mark.parametrize("bad", [
    dict(batch=0), dict(max_src_len=4), dict(max_mel_len=19), dict(idx=None), dict(o_mel=None),
    dict(mel=None), dict(energy_bytes=2), dict(n_mels=81), dict(accent=None), dict(o_mel=72),
    dict(n_utt=2), dict(idx_host=None), dict(o_speaker=None)])
def test_batch_gather_validates_before_any_launch(bad):
    L = importlib.import_module(PKG + "._lib")
    args, keep = _gather_args(**bad)
    with pytest.raises(L.KernelError, match="fs2_batch_gather"):
        L.lib.fs2_batch_gather(*args)
    del keep


def test_batch_gather_rejects_a_negative_index():
    L = importlib.import_module(PKG + "._lib")
    args, keep = _gather_args()
    keep[0][1] = -1
    with pytest.raises(L.KernelError, match="index -1"):
        L.lib.fs2_batch_gather(*args)
    with pytest.raises(L.KernelError):
        L.lib.fs2_eval_accum(None, 64, 64, 64, 4, 0)
    with pytest.raises(L.KernelError):
        L.lib.fs2_eval_accum(64, 64, 64, None, 0, 0)
