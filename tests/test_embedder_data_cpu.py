"""The speaker encoder's data path and EER test, the parts that need no GPU: argument checks of
the new entries, the batcher's host draws against the reference's own (fixture g15), the numpy
EER oracle against the fixture, and the epoch loops' control flow with stub steps."""
import importlib
import random

import numpy as np
import pytest

from conftest import load_golden
import embedder_data_oracle as O

PKG = "mid-attribute-speaker-generation_amd"
NEW = ("fs2_mel_crop_gather", "fs2_rows_mean_unit", "fs2_ge2e_eer", "fs2_ge2e_eer_ws_bytes",
       "fs2_epoch_stats_add")


def test_new_symbols_resolve():
    L = importlib.import_module(PKG + "._lib")
    assert set(NEW) <= set(L.lib.symbols())
    L.lib.load()
    for name in NEW:
        assert callable(getattr(L.lib, name))


def test_entries_validate_arguments_before_any_launch():
    L = importlib.import_module(PKG + "._lib")
    lib, p, big = L.lib, 16, 1 << 30  # p: a non-null placeholder, never dereferenced
    for n_mels, length in ((80, 0), (80, 257), (129, 150), (0, 150)):
        with pytest.raises(L.KernelError):
            lib.fs2_mel_crop_gather(p, p, p, p, 4, n_mels, length, p, 0)
    with pytest.raises(L.KernelError):
        lib.fs2_mel_crop_gather(p, p, p, p, -1, 80, 150, p, 0)
    assert lib.fs2_mel_crop_gather(None, None, None, None, 0, 80, 150, None, 0) == 0  # no-op
    with pytest.raises(L.KernelError):
        lib.fs2_rows_mean_unit(p, p, 1, 1025, p, 0)
    assert lib.fs2_ge2e_eer_ws_bytes(5, 64) == (2 * 5 * 64 + 5) * 4
    for n_spk, m_ver, dim, ws in ((1, 4, 64, big), (5, 1, 64, big), (5, 4, 257, big),
                                  (5, 4, 64, (2 * 5 * 64 + 5) * 4 - 4)):
        with pytest.raises(L.KernelError):
            lib.fs2_ge2e_eer(p, p, n_spk, 2, m_ver, dim, p, p, p, p, ws, 0)
    with pytest.raises(L.KernelError):
        lib.fs2_epoch_stats_add(None, p, p, p, p, 4, None, 0)
    with pytest.raises(L.KernelError):
        lib.fs2_epoch_stats_add(p, p, p, p, None, 4, None, 0)  # logits without labels


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    path = tmp_path_factory.mktemp("g15_corpus")
    O.write_corpus(str(path))
    return str(path)


def _batcher(corpus, g, seed, **kw):
    D = importlib.import_module(PKG + ".embedder_data")
    store = D.SpeakerStore(corpus, device="cpu", file_list=[str(f) for f in g["files"]])
    return D.SpeakerBatcher(store, 4, 3, rng=random.Random(seed), **kw)


def _check_draw(b, d, g, tag):
    """The draw decodes to the fixture's files, utterances, crop starts, L and langs."""
    length = int(g[f"{tag}.L"])
    assert d["length"] == length
    k, u, c, f = O.decode(g[f"{tag}.first"])
    k2, u2, c2, f2 = O.decode(g[f"{tag}.last"])
    assert (c == 0).all() and (c2 == O.NMELS - 1).all() and (k == k2).all() and (u == u2).all()
    assert (f2 - f == length - 1).all()
    files = [O.NAMES.index(b.store.files[i]) for i in d["files"] for _ in d["utts"][0]]
    assert files == k.tolist()
    assert [x for us in d["utts"] for x in us] == u.tolist()
    assert [p for p, us in zip(d["starts"], d["utts"]) for _ in us] == f.tolist()
    off, stride, start, langs = b.rows(d)
    assert langs.tolist() == g[f"{tag}.langs"].tolist()
    assert start.tolist() == f.tolist()
    assert stride.tolist() == [O.FILES[i][2] for i in k]
    # the row descriptors address exactly those elements of the flat store
    data = b.store.data.numpy()
    assert np.array_equal(data[off + start], g[f"{tag}.first"])
    assert np.array_equal(data[off + (O.NMELS - 1) * stride + start + length - 1], g[f"{tag}.last"])


def test_batcher_draws_what_the_reference_drew(corpus):
    g = load_golden("g15_embedder_data.npz")
    b = _batcher(corpus, g, int(g["seed"]))
    assert b.lower == 115 and b.batches_per_epoch == 1
    for i in range(2):
        _check_draw(b, b.draw(), g, f"batch{i}")
        state = b.rng.getstate()
        assert b.rng.random() == float(g[f"batch{i}.next"])  # consume_shuffle keeps in step
        b.rng.setstate(state)


def test_without_consume_shuffle_the_generator_falls_behind(corpus):
    g = load_golden("g15_embedder_data.npz")
    b = _batcher(corpus, g, int(g["seed"]), consume_shuffle=False)
    _check_draw(b, b.draw(), g, "batch0")
    assert b.rng.random() != float(g["batch0.next"])


def test_speaker_batch_draw(corpus):
    g = load_golden("g15_embedder_data.npz")
    b = _batcher(corpus, g, int(g["spk.seed"]))
    d = b.draw_speaker(int(g["spk.index"]), 400)
    assert len(d["utts"][0]) == 400 == g["spk.first"].shape[0]
    _check_draw(b, d, g, "spk")
    assert b.rng.random() == float(g["spk.next"])


def test_store_layout_and_short_file(corpus, tmp_path):
    D = importlib.import_module(PKG + ".embedder_data")
    store = D.SpeakerStore(corpus, device="cpu")
    assert store.files == list(O.NAMES) and store.langs == ["english", "japanese"]
    assert store.lang2files == {"japanese": [0, 1, 2], "english": [3, 4, 5]}
    assert store.utt_count == [f[1] for f in O.FILES] and store.frames == [f[2] for f in O.FILES]
    for k in range(len(O.FILES)):
        n = O.file_array(k).size
        assert np.array_equal(store.data[store.offset[k]:store.offset[k] + n].numpy(),
                              O.file_array(k).reshape(-1))
    np.save(tmp_path / "jvs_009_M_japanese.npy", np.zeros((2, 80, 149), np.float32))
    with pytest.raises(ValueError, match="149 frames"):
        D.SpeakerStore(str(tmp_path), device="cpu")


@pytest.mark.parametrize("k", range(4))
def test_eer_oracle_reproduces_fixture(k):
    g = load_golden("g15_embedder_data.npz")
    sim, want = g[f"eer{k}.sim"], g[f"eer{k}.result"]
    assert O.threshold_gap(sim) >= 1e-4  # fp32 rounding of sim cannot flip a comparison
    table, got = O.eer_sweep(sim)
    assert got[1] == want[1]
    assert np.abs(got - want).max() <= 1e-6
    # the float64 restatement of get_cossim agrees with the reference's fp32 sim
    assert np.abs(O.cossim(g[f"eer{k}.enroll"], g[f"eer{k}.verify"]) - sim).max() <= 1e-6
    if k == 3:
        assert sim.max() < 0.5 and not want.any() and (table[:, 1] == 1).all()


def test_fixture_has_interior_thresholds():
    g = load_golden("g15_embedder_data.npz")
    shapes = [g[f"eer{k}.enroll"].shape[:2] + g[f"eer{k}.verify"].shape[1:2] for k in range(3)]
    assert shapes == [(5, 2, 4), (4, 3, 3), (2, 1, 2)]
    r = [g[f"eer{k}.result"] for k in range(3)]
    assert sum(0.5 < x[1] < 0.99 and x[0] > 0 for x in r) >= 2


class _StubBatcher:
    batches_per_epoch = 3

    def __init__(self):
        self.n = 0

    def next_batch(self):
        self.n += 1
        return None, None


def _stub_trainer(da_losses, da_startpoint=0.0):
    """An EmbedderTrainer whose steps and statistics are host stubs."""
    T = importlib.import_module(PKG + ".embedder_train")
    tr = T.EmbedderTrainer(device="meta", n_utt=3, da_startpoint=da_startpoint)
    tr.calls, it = [], iter(da_losses)
    tr.train_step = lambda m, l, progress, ge2e: (tr.calls.append(("train", progress, ge2e)) or
                                                  (2.0, 4.0, 0, 0, 0))
    tr.da_classifier_step = lambda m, l: (tr.calls.append(("da",)) or (0, next(it), 0, 0, 0))
    tr._stats_new = lambda: [0.0, 0.0, 0.0, 0.0]

    def add(t, loss, da_loss, langs):
        t[0] += loss or 0.0
        t[1] += da_loss
        t[2] += 50.0
        t[3] += 1
    tr._stats_add, tr._stats_read = add, list
    return tr


def test_da_subroutine_stops_below_the_floor():
    tr = _stub_trainer([30.0] * 3 + [25.0] * 3 + [10.0] * 3 + [5.0] * 30)
    b = _StubBatcher()
    assert tr.da_subroutine(b) == [30.0, 25.0, 10.0] and b.n == 9


def test_da_subroutine_stops_when_the_loss_rises():
    tr = _stub_trainer([30.0] * 3 + [40.0] * 3 + [35.0] * 30)
    b = _StubBatcher()
    assert tr.da_subroutine(b) == [30.0, 40.0] and b.n == 6
    tr = _stub_trainer([30.0] * 60)  # neither rule: max_passes
    assert tr.da_subroutine(_StubBatcher(), max_passes=4) == [30.0] * 4


def test_train_epoch_batches_anneal_and_subroutine():
    tr = _stub_trainer([1.0] * 30, da_startpoint=0.25)
    b = _StubBatcher()
    stats = tr.train_epoch(b, 0, 2)
    assert stats == {"loss": 2.0, "da_loss": 4.0, "da_acc": 50.0}
    assert tr.calls == [("train", 0.0, False)] * 3 and b.n == 3 and tr.last_da_passes is None
    tr.calls.clear()
    tr.train_epoch(b, 1, 2, ge2e_backward=True)  # progress 0.5 > da_startpoint
    assert tr.calls == [("train", 0.5, True)] * 3 + [("da",)] * 3 and tr.last_da_passes == [1.0]
    lr = tr.optimizers["main"].lr
    tr.train_epoch(b, 800, 2400)
    assert tr.optimizers["main"].lr == lr / 2
