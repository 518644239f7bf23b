"""The FastSpeech2 corpus on the device against the host path it replaces: ``fs2_batch_gather``
against ``Dataset.collate_fn`` + ``to_device``, ``evaluate`` against the reference's ``.item()``
loop, ``fit`` against a manual loop of ``Trainer.step`` over host-collated batches, and a captured
step fed through ``out=``.  Every comparison is exact: both sides move or add the same values."""
import copy
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from corpus_store_helpers import corpora_at, datasets, set_level, write_val  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("mid-attribute-speaker-generation_amd")
C = importlib.import_module("mid-attribute-speaker-generation_amd.corpus_store")
D = importlib.import_module("mid-attribute-speaker-generation_amd.dataset")
M = importlib.import_module("mid-attribute-speaker-generation_amd.model")
T = importlib.import_module("mid-attribute-speaker-generation_amd.train")
DEV = "cuda"
LEVELS = {False: "phoneme_level", True: "frame_level"}


# ------------------------------------------------------------------ corpora and stores
VARIANTS = {
    "ja_first": dict(order=(0, 1)),
    "en_first": dict(order=(1, 0)),                                   # a 13-tuple: no accents
    "energy_f64": dict(order=(0, 1), energy=("phoneme_level", np.float64)),
    "pitch_frame": dict(order=(0, 1), pitch=("frame_level", None)),
    "energy_frame": dict(order=(0, 1), energy=("frame_level", None)),
}


@pytest.fixture(scope="module")
def variant(tmp_path_factory):
    """name -> (corpus, host dataset in gather order (no sort, tail kept), device store)."""
    made = {}

    def get(name):
        if name not in made:
            v = VARIANTS[name]
            corpus = corpora_at(str(tmp_path_factory.mktemp(name)))
            for key in ("pitch", "energy"):
                if key in v:
                    set_level(corpus, key, v[key][0], dtype=v[key][1])
            host = datasets(corpus, order=v["order"], sort=False, drop_last=False)
            made[name] = (corpus, host, C.CorpusStore(host, device=DEV))
        return made[name]
    return get


def _host_batch(host, group):
    return D.to_device(host.collate_fn([host[i] for i in group])[0], DEV)


def _same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if torch.is_tensor(b):
            assert torch.is_tensor(a) and a.dtype == b.dtype and a.shape == b.shape, \
                (k, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
            assert a.device.type == "cuda" and torch.equal(a, b), k
        else:
            assert a == b, (k, a, b)


def _groups(store):
    """Index groups with the cases a gather can get wrong (at most batch_size = 4 each)."""
    src, mel, n = store.src_len, store.mel_len, len(store)
    extremes = [int(np.argmax(mel)), int(np.argmin(mel)), int(np.argmax(src)), int(np.argmin(src))]
    cross = [(i, j) for i in range(n) for j in range(n)
             if src[i] > src[j] and mel[i] < mel[j]]  # text maximum and mel maximum differ
    assert cross and len(set(extremes)) >= 2
    return {"extremes": list(dict.fromkeys(extremes)), "one": [5], "cross": list(cross[0]),
            "first_last": [0, n - 1], "last_first_repeat": [n - 1, 0, n - 1],
            "boundary": [11, 12, 13, 14]}


@pytest.mark.parametrize("name", ["ja_first", "en_first", "energy_f64"])
def test_gather_equals_the_host_path(variant, name):
    _, host, store = variant(name)
    assert store.n_tuple == (13 if name == "en_first" else 14)
    assert store.energy.dtype == (torch.float64 if name == "energy_f64" else torch.float32)
    for tag, group in _groups(store).items():
        got, want = store.gather(group), _host_batch(host, group)
        _same(got, want)
        assert isinstance(got[5], int) and isinstance(got[8], int), tag
        assert got[10].dtype == store.energy.dtype


def test_batcher_yields_the_loaders_batches(variant):
    """Iterating the batcher: the reference loader's batches (train.py:56-63), on the device."""
    corpus, host, store = variant("ja_first")
    g = torch.Generator()
    g.manual_seed(0)
    batches = list(C.CorpusBatcher(store, 4, 2, generator=g))
    g.manual_seed(0)
    groups = list(C.CorpusBatcher(store, 4, 2, generator=g).groups())
    assert len(batches) == len(groups) == 6
    for b, grp in zip(batches, groups):
        _same(b, _host_batch(host, grp))
        assert np.all(np.diff(b[4].cpu().numpy()) <= 0)  # sorted by phoneme count


def test_target_lengths_above_the_maxima_equal_pad_batch(variant):
    _, host, store = variant("ja_first")
    for group in _groups(store).values():
        want = _host_batch(host, group)
        ts, tm = int(want[5]) + 3, int(want[8]) + 5
        _same(store.gather(group, ts, tm), PKG.data.pad_batch(want, ts, tm))
        _same(store.gather(group, int(want[5]), tm), PKG.data.pad_batch(want, int(want[5]), tm))
    L = importlib.import_module("mid-attribute-speaker-generation_amd._lib")
    with pytest.raises(L.KernelError, match="max_mel_len"):
        store.gather([0, 1], max_mel_len=int(store.mel_len[[0, 1]].max()) - 1)
    with pytest.raises(L.KernelError, match="max_src_len"):
        store.gather([0, 1], max_src_len=int(store.src_len[[0, 1]].max()) - 1)


@pytest.mark.parametrize("name,levels", [("pitch_frame", (True, False)),
                                         ("energy_frame", (False, True))])
def test_frame_level_features(variant, name, levels):
    _, host, store = variant(name)
    assert store.levels == levels
    names = tuple(LEVELS[f] for f in levels)
    for group in _groups(store).values():
        got, want = store.gather(group), _host_batch(host, group)
        _same(got, want)
        for k, frame in zip((9, 10), levels):  # the padded width follows the feature's level
            assert got[k].shape[1] == (got[8] if frame else got[5])
        ts, tm = int(want[5]) + 2, int(want[8]) + 7
        _same(store.gather(group, ts, tm), PKG.data.pad_batch(want, ts, tm, names))


def test_out_is_written_in_place_and_padding_is_zeroed(variant):
    _, host, store = variant("ja_first")
    long = [int(i) for i in np.argsort(-store.mel_len.astype(np.int64))[:4]]
    short = [int(i) for i in np.argsort(store.mel_len.astype(np.int64))[:4]]
    ts = int(store.src_len[long + short].max())
    first = store.gather(long, max_src_len=ts)
    tm = first[8]
    assert all(bool((t != 0).any()) for t in (first[6][:, -1], first[3]))  # the padding-to-be
    got = store.gather(short, out=first)
    assert all(a is b for a, b in zip(got[2:], first[2:]) if torch.is_tensor(b))
    want = PKG.data.pad_batch(_host_batch(host, short), ts, tm)
    _same(got, want)
    assert got[0] == [store.ids[i] for i in short] and (got[5], got[8]) == (ts, tm)
    with pytest.raises(RuntimeError, match="out tensor"):
        store.gather(short[:3], out=first)  # another batch size: not "the same shapes"


def test_a_corpus_above_the_free_memory_raises_with_both_counts(variant, monkeypatch):
    _, host, store = variant("ja_first")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (4096, 1 << 30))
    with pytest.raises(MemoryError, match=rf"{store.nbytes} bytes.* 4096 bytes free"):
        C.CorpusStore(host, device=DEV)


def test_agree_lengths_regathers_on_the_device(variant, monkeypatch):
    """``Trainer._agree_lengths`` with a store-cut shard: the agreed lengths come from the
    gather, and equal the host re-padding it replaces."""
    _, host, store = variant("ja_first")
    group = [1, 2, 3]
    want = _host_batch(host, group)
    ts, tm = int(want[5]) + 4, int(want[8]) + 9
    tr = T.Trainer.__new__(T.Trainer)
    tr._agree, tr._host_pg = True, None
    monkeypatch.setattr(T.dist, "all_reduce", lambda t, **kw: t.copy_(torch.tensor([ts, tm])))
    monkeypatch.setattr(PKG.data, "pad_batch", None)  # the host path must not be taken
    got = tr._agree_lengths(store.gather(group))
    monkeypatch.undo()
    _same(got, PKG.data.pad_batch(want, ts, tm))


# ------------------------------------------------------------------ model-level tests
@pytest.fixture(scope="module")
def configs():
    pp, mc, tc, path = PKG.config.load_configs("JVS-VCTK")
    return pp, mc, tc, path


def _model(configs):
    pp, mc, tc, path = configs
    model = M.FastSpeech2(pp, mc, path, device=DEV, compute_dtype=torch.float32)
    PKG.seeded.load_seeded_(model)
    model.dropout = False
    model.train()
    return model


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_evaluate_equals_the_item_loop(variant, configs):
    corpus, _, _ = variant("ja_first")
    write_val(corpus)
    val = datasets(corpus, sort=False, drop_last=False, filename="val.txt")
    store = C.CorpusStore(val, device=DEV)
    pp, mc, tc, _ = configs
    model = _model(configs)
    Loss = T.FastSpeech2Loss(pp, mc)
    eLoss = T.SpeakerMetaEncLoss(pp, mc)
    before = _state(model)
    n, bs = len(val), 4
    assert n == 13  # 4 + 4 + 4 + 1: the last batch is short

    # evaluate.py:53-75, per host batch with .item()
    model.eval()
    loss_sums, eloss_sums = [0 for _ in range(6)], 0
    for lo in range(0, n, bs):
        batch = D.to_device(val.collate_fn([val[i] for i in range(lo, min(lo + bs, n))])[0], DEV)
        with torch.no_grad():
            output = model(*(batch[2:12]), accents=batch[13], speaker_meta=batch[12])
            losses = Loss(batch[:12], output[:-2])
            for i in range(len(losses)):
                loss_sums[i] += losses[i].item() * len(batch[0])
            eloss = eLoss(output[-1], output[-2])
            eloss_sums += eloss * len(batch[0])
    model.train()
    want_means = [s / n for s in loss_sums]
    want_emean = eloss_sums / n
    want_msg = T.VAL_MESSAGE.format(7, *want_means) + ", Speaker Loss: {:.4f}".format(want_emean)

    for source, kw in ((store, dict(batch_size=bs)),
                       (C.CorpusBatcher(store, bs, group_size=1, shuffle=False, sort=False,
                                        drop_last=False), {})):
        means, emean, msg = T.evaluate(model, 7, source, Loss, eLoss, **kw)
        print("validation means", means, emean, "reference loop", want_means, float(want_emean))
        assert means == want_means
        assert emean == float(want_emean)
        assert msg == want_msg
        assert model.training
    after = _state(model)
    assert before.keys() == after.keys()
    for k in before:  # no parameter and no BatchNorm buffer moved
        assert torch.equal(before[k], after[k]), k


def _train_config(tc, root):
    tc = copy.deepcopy(tc)
    tc["optimizer"]["batch_size"] = 4
    tc["step"] = dict(total_step=3, save_step=2, val_step=2, log_step=1, synth_step=1000)
    tc["path"] = {k: os.path.join(root, k) for k in ("ckpt_path", "log_path", "result_path")}
    return tc


def test_fit_equals_a_manual_loop_and_resumes(variant, configs, tmp_path):
    corpus, host, store = variant("ja_first")
    write_val(corpus)
    val = C.CorpusStore(datasets(corpus, sort=False, drop_last=False, filename="val.txt"), device=DEV)
    pp, mc, tc, _ = configs
    tc = _train_config(tc, str(tmp_path))
    g = torch.Generator()
    g.manual_seed(9)
    groups = list(C.CorpusBatcher(store, 4, 4, generator=g).groups())[:3]
    assert len(groups) == 3 and all(len(grp) == 4 for grp in groups)

    model = _model(configs)
    tr = T.Trainer(model, pp, mc, tc)
    g.manual_seed(9)
    messages = []
    last = T.fit(tr, C.CorpusBatcher(store, 4, 4, generator=g),
                 C.CorpusBatcher(val, 4, group_size=1, shuffle=False, sort=False, drop_last=False),
                 tc, log=messages.append)
    torch.cuda.synchronize()
    assert last == 3 and model.training and tr.opt.current_step == 3
    got = model.arena().flat.clone()

    # the same three index groups, collated on the host
    model2 = _model(configs)
    tr2 = T.Trainer(model2, pp, mc, tc)
    lines = []
    for step, grp in enumerate(groups, start=1):
        losses = tr2.step(_host_batch(host, grp))[0]
        lines.append("Step {}/3, ".format(step) + T.LOSS_MESSAGE.format(*[l.item() for l in losses]))
    torch.cuda.synchronize()
    assert torch.equal(got, model2.arena().flat)
    assert torch.equal(tr.opt.m, tr2.opt.m) and torch.equal(tr.opt.v, tr2.opt.v)

    with open(os.path.join(tc["path"]["log_path"], "train", "log.txt")) as f:
        assert f.read().split("\n") == lines + [""]
    with open(os.path.join(tc["path"]["log_path"], "val", "log.txt")) as f:
        val_lines = f.read().split("\n")
    assert len(val_lines) == 2 and val_lines[0].startswith("Validation Step 2, Total Loss: ")
    assert ", Speaker Loss: " in val_lines[0] and val_lines[1] == ""
    assert messages == lines[:2] + [val_lines[0]] + lines[2:]

    # 2.pth.tar: the reference's checkpoint; one more step from it reaches the same weights
    assert os.listdir(tc["path"]["ckpt_path"]) == ["2.pth.tar"]
    ckpt = torch.load(os.path.join(tc["path"]["ckpt_path"], "2.pth.tar"), weights_only=True)
    assert sorted(ckpt) == ["model", "optimizer"]
    model3 = _model(configs)
    with torch.no_grad():
        for p in model3.parameters():
            p.add_(1.0)
    model3.load_state_dict(ckpt["model"])
    tr3 = T.Trainer(model3, pp, mc, tc, current_step=2)
    tr3.opt.load_state_dict(ckpt["optimizer"])
    tr3.step(store.gather(groups[2]))
    torch.cuda.synchronize()
    assert torch.equal(got, model3.arena().flat)


def test_fit_use_clf_draws_the_reference_permutation(variant, configs, tmp_path):
    """``--use_clf``: the discriminator comes from ``path.discriminator_path``, the permutation
    from ``random.sample(range(B), B)`` once per step, ``lambda`` from the train config."""
    import random
    G = importlib.import_module("mid-attribute-speaker-generation_amd.ge2e")
    _, host, store = variant("ja_first")
    pp, mc, tc, _ = configs
    tc = _train_config(tc, str(tmp_path))
    tc["step"].update(total_step=2, save_step=100, val_step=100)
    tc["lambda"] = 0.5
    disc = G.SpeechEmbedder(device=DEV)
    PKG.seeded.load_seeded_(disc)
    tc["path"]["discriminator_path"] = str(tmp_path / "disc.pth.tar")
    torch.save({"embedder_net": disc.state_dict(), "ge2e": G.GE2ELoss(DEV).state_dict()},
               tc["path"]["discriminator_path"])
    clf = T.load_discriminator(tc, DEV)
    for a, b in zip(clf[0].state_dict().values(), disc.state_dict().values()):
        assert torch.equal(a, b)
    clf[0].da_dropout = disc.da_dropout = 0.0  # two discriminators: no shared dropout stream

    g = torch.Generator()
    g.manual_seed(4)
    groups = list(C.CorpusBatcher(store, 4, 4, generator=g).groups())[:2]
    model = _model(configs)
    tr = T.Trainer(model, pp, mc, tc)
    g.manual_seed(4)
    random.seed(3)
    assert T.fit(tr, C.CorpusBatcher(store, 4, 4, generator=g), None, tc, clf=clf) == 2

    model2 = _model(configs)
    tr2 = T.Trainer(model2, pp, mc, tc)
    random.seed(3)
    lines = []
    for step, grp in enumerate(groups, start=1):
        perm = random.sample(range(4), 4)
        out = tr2.step(_host_batch(host, grp), clf=(disc, G.GE2ELoss(DEV)),
                       clf_args=(perm, step, 2, 0.5))
        lines.append("Step {}/2, ".format(step) + T.LOSS_MESSAGE.format(*[l.item() for l in out[0]])
                     + " Clf Loss: {:.4f}".format(out[4][0]))
    torch.cuda.synchronize()
    assert torch.equal(model.arena().flat, model2.arena().flat)
    with open(os.path.join(tc["path"]["log_path"], "train", "log.txt")) as f:
        assert f.read().split("\n") == lines + [""]
    assert os.listdir(tc["path"]["ckpt_path"]) == []


def test_command_line_trains_from_a_config_directory(variant, configs, tmp_path, capsys):
    """``python -m ... .train -c DIR --corpus JA EN`` in process: two steps, then one more from
    ``--restore_step 2``."""
    import shutil
    import yaml
    corpus, _, _ = variant("ja_first")
    write_val(corpus)
    pp, mc, tc, _ = configs
    tc = _train_config(tc, str(tmp_path))
    tc["step"].update(total_step=2, save_step=2, val_step=2)
    cfg = str(tmp_path / "config")
    shutil.copytree(corpus[0], cfg)  # stats.json, speakers.json
    for name, obj in (("preprocess", pp), ("model", mc), ("train", tc),
                      ("preprocess_JA", corpus[1][0]), ("preprocess_EN", corpus[1][1])):
        with open(os.path.join(cfg, name + ".yaml"), "w") as f:
            yaml.safe_dump(obj, f)
    T.main(["-c", cfg, "--corpus", "JA", "EN"])
    out = capsys.readouterr().out
    assert "finished at step 2" in out and "Validation Step 2, Total Loss: " in out
    assert os.listdir(tc["path"]["ckpt_path"]) == ["2.pth.tar"]
    tc["step"]["total_step"] = 3
    with open(os.path.join(cfg, "train.yaml"), "w") as f:
        yaml.safe_dump(tc, f)
    T.main(["-c", cfg, "--corpus", "JA", "EN", "--restore_step", "2"])
    assert "Step 3/3, Total Loss: " in capsys.readouterr().out
    with open(os.path.join(tc["path"]["log_path"], "train", "log.txt")) as f:
        assert [l.split(",")[0] for l in f.read().split("\n")[:-1]] == ["Step 1/2", "Step 2/2",
                                                                       "Step 3/3"]


def test_graph_trainer_fed_through_out(variant, configs):
    """``Trainer(graph=True)`` whose static inputs the gather fills directly: step 1 eager +
    capture, two replays, against three eager steps over the same batches."""
    _, _, store = variant("ja_first")
    pp, mc, tc, _ = configs
    groups = [[0, 1, 2, 3], [20, 21, 22, 23], [8, 9, 14, 15]]
    ts = max(store.maxima(grp)[0] for grp in groups)
    tm = max(store.maxima(grp)[1] for grp in groups)

    eager = _model(configs)
    tr_e = T.Trainer(eager, pp, mc, tc)
    want_losses = [torch.stack(list(tr_e.step(store.gather(grp, ts, tm))[0])).clone()
                   for grp in groups]

    model = _model(configs)
    tr = T.Trainer(model, pp, mc, tc, graph=True)
    assert tr.static_batch() is None
    losses = [torch.stack(list(tr.step(store.gather(groups[0], ts, tm))[0])).clone()]
    static = tr.static_batch()
    assert static is not None
    for grp in groups[1:]:
        batch = store.gather(grp, out=static)
        assert all(a is b for a, b in zip(batch, static) if torch.is_tensor(b))
        graph = tr._graph
        losses.append(torch.stack(list(tr.step(batch)[0])).clone())
        assert tr._graph is graph  # a replay, not a new capture
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(losses), torch.stack(want_losses))
    assert torch.equal(model.arena().flat, eager.arena().flat)
    assert torch.equal(tr.opt.m, tr_e.opt.m) and torch.equal(tr.opt.v, tr_e.opt.v)
    assert tr.opt.adam_steps == tr_e.opt.adam_steps == 3
