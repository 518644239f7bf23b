"""Objective synthesis metrics on the GPU against the numpy oracle (tests/dtw_oracle.py): DTW bit
for bit where the arithmetic is exact, to 1e-12 and with the exact path where it is not, the MFCC
against scipy's DCT, the path records, and the way up to ``evaluate_synthesis`` and ``fit``."""
import copy
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_oracle as O  # noqa: E402
from corpus_store_helpers import corpora_at, datasets, write_val  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("mid-attribute-speaker-generation_amd")
A = importlib.import_module("mid-attribute-speaker-generation_amd.audio")
C = importlib.import_module("mid-attribute-speaker-generation_amd.corpus_store")
K = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
M = importlib.import_module("mid-attribute-speaker-generation_amd.model")
MT = importlib.import_module("mid-attribute-speaker-generation_amd.metrics")
T = importlib.import_module("mid-attribute-speaker-generation_amd.train")
DEV = "cuda"
SEED = 20261020


def _pair(t1, t2, k, integer):
    rng = np.random.default_rng([SEED, t1, t2, 0 if integer else 1])
    if integer:
        draw = lambda t: rng.integers(0, 3, (t, k)).astype(np.float32)  # noqa: E731
    else:
        draw = lambda t: rng.standard_normal((t, k)).astype(np.float32)  # noqa: E731
    return draw(t1), draw(t2)


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else \
        torch.tensor(x, dtype=dtype, device=DEV)


def _run(a, b):
    """One pair at its own shape -> (cost float, path (n, 2) numpy)."""
    cost, path, n = K.dtw(_dev(a)[None], _dev(b)[None], _dev([len(a)], torch.int64),
                          _dev([len(b)], torch.int64))
    n = int(n[0])
    assert path.shape == (1, len(a) + len(b) - 1, 2) and 1 <= n <= path.shape[1]
    return float(cost[0]), path[0, :n].cpu().numpy()


# ------------------------------------------------------------------ DTW
@pytest.mark.parametrize("t1,t2", [(65, 64), (37, 53)])
def test_dtw_integer_features_bit_for_bit(t1, t2):
    """Values 0..2, K = 2: the sums of squares are exact, fp64 sqrt is correctly rounded and a
    cell is one add, so cost and path equal the oracle's bit for bit -- ties included."""
    a, b = _pair(t1, t2, 2, integer=True)
    ties = O.path_ties(a, b)
    print(f"({t1}, {t2}): {ties} exact ties on the optimal path")
    assert ties >= 1  # otherwise the tie rule goes untested
    want_cost, want_path = O.dtw(a, b)
    cost, path = _run(a, b)
    assert cost == want_cost
    assert np.array_equal(path, want_path)


REAL = [(37, 53, 13), (65, 64, 13), (130, 257, 24), (257, 300, 13), (1, 9, 13), (9, 1, 13),
        (1, 1, 13)]


@pytest.mark.parametrize("t1,t2,k", REAL)
def test_dtw_real_features(t1, t2, k):
    """1e-12 relative: at most 600 adds on the path, each cell's local cost within an ulp of the
    oracle's (FMA contraction).  The path is compared exactly, which is legitimate because the
    oracle's smallest on-path gap is far above that rounding -- asserted first."""
    a, b = _pair(t1, t2, k, integer=False)
    gap = O.path_gap(a, b)
    print(f"({t1}, {t2}, K={k}): smallest on-path gap {gap:.3e}")
    assert gap >= 1e-6
    want_cost, want_path = O.dtw(a, b)
    cost, path = _run(a, b)
    print(f"cost {cost!r} oracle {want_cost!r} rel {abs(cost - want_cost) / want_cost:.2e}")
    assert abs(cost - want_cost) <= 1e-12 * want_cost
    assert np.array_equal(path, want_path)


def test_dtw_ragged_batch_equals_single_runs():
    """Five pairs of different lengths inside (70, 90), NaN in every padding row: each pair's
    result is bitwise that of its own run (which, for la > lb, sweeps along the other side)."""
    lens = [(70, 90), (1, 90), (70, 1), (33, 17), (12, 64)]
    T1, T2, k = 70, 90, 13
    rng = np.random.default_rng([SEED, 5])
    a = np.full((len(lens), T1, k), np.nan, np.float32)
    b = np.full((len(lens), T2, k), np.nan, np.float32)
    for p, (la, lb) in enumerate(lens):
        a[p, :la] = rng.standard_normal((la, k))
        b[p, :lb] = rng.standard_normal((lb, k))
    cost, path, n = K.dtw(_dev(a), _dev(b), _dev([l[0] for l in lens], torch.int64),
                          _dev([l[1] for l in lens], torch.int64))
    cost, path, n = cost.cpu().numpy(), path.cpu().numpy(), n.cpu().numpy()
    for p, (la, lb) in enumerate(lens):
        one_cost, one_path = _run(a[p, :la], b[p, :lb])
        assert np.isfinite(cost[p]) and cost[p] == one_cost, p
        assert n[p] == len(one_path) and np.array_equal(path[p, :n[p]], one_path), p
        want_cost, want_path = O.dtw(a[p, :la], b[p, :lb])
        assert O.path_gap(a[p, :la], b[p, :lb]) >= 1e-6
        assert abs(one_cost - want_cost) <= 1e-12 * want_cost and np.array_equal(one_path, want_path)


@pytest.mark.parametrize("t1,t2", [(1000, 1000), (2048, 3), (3, 2048)])
def test_dtw_at_the_limits(t1, t2):
    """The training limit (max_seq_len = 1000) and the kernel's own (2048, along either side).
    1e-12 still holds: a path of at most 2050 cells is 2050 adds of relative error 1.1e-16 each
    plus an ulp per local cost, below 5e-13."""
    a, b = _pair(t1, t2, 13, integer=False)
    want_cost, want_path = O.dtw(a, b)
    cost, path = _run(a, b)
    print(f"({t1}, {t2}): cost {cost!r} oracle {want_cost!r}, path {len(path)}")
    assert abs(cost - want_cost) <= 1e-12 * want_cost
    assert len(path) == len(want_path)
    if t1 != t2:
        assert np.array_equal(path, want_path)
    L = importlib.import_module("mid-attribute-speaker-generation_amd._lib")
    with pytest.raises(L.KernelError, match="2048"):
        K.dtw(torch.zeros(1, 2049, 2, device=DEV), torch.zeros(1, 3, 2, device=DEV),
              _dev([3], torch.int64), _dev([3], torch.int64))


# ------------------------------------------------------------------ MFCC
@pytest.mark.parametrize("F", [1, 7, 65])
def test_mfcc_both_layouts(F):
    """atol 1e-3 is the worst-case fp32 bound gamma_80 * sum |x| |w| ~ 4.8e-6 * 146 (|x| <= 11.6,
    sum_m |w_km| <= sqrt(80) * 1): derived, not measured."""
    B, n_mels = 3, 80
    rng = np.random.default_rng([SEED, F])
    x = rng.uniform(-11.6, 2.0, (B, n_mels, F)).astype(np.float32)
    live = [F, max(F - 3, 0), (F + 1) // 2]
    n = _dev(live, torch.int64)
    for k in (13, 1, 79):
        want = O.mfcc(np.swapaxes(x, 1, 2), k)  # (B, F, k)
        got = MT.mfcc(_dev(x), n, k)
        rows = np.ascontiguousarray(np.swapaxes(x, 1, 2))
        got_rows = MT.mfcc(_dev(rows), n, k, rows=True)
        got_flat = MT.mfcc(_dev(rows.reshape(B * F, n_mels)), n, k, rows=True)
        assert got.shape == got_rows.shape == got_flat.shape == (B, F, k)
        assert torch.equal(got_rows, got_flat)
        for name, g in (("(B, n_mels, F)", got), ("rows", got_rows)):
            g = g.cpu().numpy()
            for p in range(B):
                err = np.abs(g[p, :live[p]] - want[p, :live[p]]).max() if live[p] else 0.0
                print(f"mfcc {name} F={F} K={k} pair {p}: max abs err {err:.2e}")
                assert err <= 1e-3
                assert not g[p, live[p]:].any()  # exactly zero past n_frames
    every = MT.mfcc(_dev(x), None, 13).cpu().numpy()  # no lengths: every frame is live
    assert np.abs(every - O.mfcc(np.swapaxes(x, 1, 2), 13)).max() <= 1e-3


# ------------------------------------------------------------------ path records
def test_path_metrics_with_f0_contours():
    t1, t2 = 65, 64
    a, b = _pair(t1, t2, 2, integer=True)
    want_cost, want_path = O.dtw(a, b)
    # voiced/voiced with an exact octave (1200 cents), a fifth-ish ratio, voiced/unvoiced both
    # ways and unvoiced/unvoiced, cycling along both contours with different periods
    fa = np.array([(220.0, 110.0, 0.0, 0.0, 330.0)[i % 5] for i in range(t1)], np.float32)
    fb = np.array([(110.0, 0.0, 165.0)[j % 3] for j in range(t2)], np.float32)
    x, y = fa[want_path[:, 0]], fb[want_path[:, 1]]
    kinds = {(bool(u > 0), bool(v > 0)) for u, v in zip(x, y)}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    assert np.any((x == 220.0) & (y == 110.0))  # the octave is on the path
    cost, path, n = K.dtw(_dev(a)[None], _dev(b)[None], _dev([t1], torch.int64),
                          _dev([t2], torch.int64))
    la, lb = _dev([t1], torch.int64), _dev([t2], torch.int64)
    for f0 in (True, False):
        rec = K.path_metrics(cost, path, n, la, lb, t1, t2, _dev(fa)[None] if f0 else None,
                             _dev(fb)[None] if f0 else None)
        assert rec.shape == (1, len(MT.FIELDS)) and rec.dtype == torch.float64
        got = rec[0].cpu().numpy()
        want = O.path_metrics(want_cost, want_path, t1, t2, fa if f0 else None, fb if f0 else None)
        print(dict(zip(MT.FIELDS, got.tolist())), want.tolist())
        for f in ("path_len", "frames_a", "frames_b", "n_vv", "n_vuv", "len_err"):
            assert got[MT.FIELDS.index(f)] == want[MT.FIELDS.index(f)], f
        for f in ("mcd_db", "f0_sq_cents"):
            g, w = got[MT.FIELDS.index(f)], want[MT.FIELDS.index(f)]
            assert abs(g - w) <= 1e-12 * abs(w), f
        assert (got[MT.N_VV] > 0) == f0
    # one octave alone is exactly 1200 cents
    one = K.path_metrics(cost, path, n, la, lb, t1, t2, torch.full((1, t1), 220.0, device=DEV),
                         torch.full((1, t2), 110.0, device=DEV))[0]
    assert float(one[MT.F0_SQ_CENTS]) == 1200.0 ** 2 * float(one[MT.N_VV])
    assert float(one[MT.N_VUV]) == 0.0 and float(one[MT.N_VV]) == float(one[MT.PATH_LEN])


# ------------------------------------------------------------------ end to end
def _mels(B, F, seed):
    rng = np.random.default_rng([SEED, seed])
    return rng.uniform(-11.6, 2.0, (B, 80, F)).astype(np.float32)


def test_compare_mels_of_a_mel_with_itself_and_with_a_stretched_copy():
    B, F = 3, 40
    m = _mels(B, F, 1)
    live = [40, 17, 1]
    n = _dev(live, torch.int64)
    rec = MT.compare_mels(_dev(m), n, _dev(m), n).cpu().numpy()
    assert rec.shape == (B, len(MT.FIELDS))
    assert not rec[:, MT.MCD_DB].any() and rec[:, MT.PATH_LEN].tolist() == live  # the diagonal
    assert not rec[:, MT.LEN_ERR].any() and not rec[:, MT.N_VV].any()
    ca = MT.mfcc(_dev(m), n)
    cost, path, pl = MT.dtw(ca, ca, n, n)
    for p, l in enumerate(live):
        assert np.array_equal(path[p, :l].cpu().numpy(), np.stack([np.arange(l)] * 2, 1))
    # every second frame repeated: frame f of the copy is frame idx[f] of the original
    idx = np.repeat(np.arange(F), 1 + (np.arange(F) % 2))  # 0 1 1 2 3 3 ...
    long = np.ascontiguousarray(m[:, :, idx])
    live_long = [int((idx < l).sum()) for l in live]
    rec = MT.compare_mels(_dev(m), n, _dev(long), _dev(live_long, torch.int64)).cpu().numpy()
    assert not rec[:, MT.MCD_DB].any()
    assert rec[:, MT.PATH_LEN].tolist() == live_long  # one path entry per frame of the longer
    assert rec[:, MT.FRAMES_A].tolist() == live and rec[:, MT.FRAMES_B].tolist() == live_long
    # the row layout gives the same records
    rows = MT.compare_mels(_dev(np.ascontiguousarray(np.swapaxes(m, 1, 2))), n,
                           _dev(np.ascontiguousarray(np.swapaxes(long, 1, 2))),
                           _dev(live_long, torch.int64), rows=True).cpu().numpy()
    assert np.array_equal(rows, rec)


def test_compare_wavs_runs_the_front_end_and_yin():
    pp = PKG.config.load_configs("JVS-VCTK")[0]
    fe, pitch = A.MelFrontEnd(pp, device=DEV), A.PitchExtractor(pp, device=DEV)
    sr, S = fe.sr, 8192
    t = np.arange(S) / sr
    wav = np.stack([np.sin(2 * np.pi * 220.0 * t), np.sin(2 * np.pi * 110.0 * t)]).astype(np.float32)
    lens = [S, S - 1000]
    same = MT.summarise(MT.compare_wavs(_dev(wav), lens, _dev(wav), lens, fe, pitch))
    assert same["mcd_db"] == 0.0 and same["length_error"] == 0.0 and same["vuv_error"] == 0.0
    assert same["f0_rmse_cents"] == 0.0 and same["voiced_pairs"] > 0
    other = MT.summarise(MT.compare_wavs(_dev(wav), lens, _dev(wav[::-1].copy()), lens[::-1], fe,
                                         pitch))
    print(other)
    assert other["mcd_db"] > 0.0 and 900.0 < other["f0_rmse_cents"] < 1500.0  # an octave apart
    # with an embedder trainer: the d-vectors' cosine per pair, one more column
    G = importlib.import_module("mid-attribute-speaker-generation_amd.ge2e")
    E = importlib.import_module("mid-attribute-speaker-generation_amd.embedder_train")
    d = G.SpeechEmbedder(device=DEV, weight_grads=True)
    PKG.seeded.load_seeded_(d)
    tr = E.EmbedderTrainer(d, G.GE2ELoss(DEV), n_utt=3)
    rec = MT.compare_wavs(_dev(wav), lens, _dev(wav), lens, fe, trainer=tr)
    assert rec.shape == (2, MT.DVEC_COS + 1)
    assert np.abs(rec[:, MT.DVEC_COS].cpu().numpy() - 1.0).max() <= 1e-6
    assert abs(MT.summarise(rec)["dvector_cos"] - 1.0) <= 1e-6


@pytest.fixture(scope="module")
def configs():
    return PKG.config.load_configs("JVS-VCTK")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    corpus = corpora_at(str(tmp_path_factory.mktemp("metrics")))
    write_val(corpus)
    host = datasets(corpus, sort=False, drop_last=False)
    val = datasets(corpus, sort=False, drop_last=False, filename="val.txt")
    return C.CorpusStore(host, device=DEV), C.CorpusStore(val, device=DEV)


def _model(configs):
    pp, mc, tc, path = configs
    model = M.FastSpeech2(pp, mc, path, device=DEV, compute_dtype=torch.float32)
    PKG.seeded.load_seeded_(model)
    model.dropout = False
    model.train()
    return model


def test_evaluate_synthesis_on_the_synthetic_corpus(corpus, configs, monkeypatch):
    _, val = corpus
    pp = configs[0]
    model = _model(configs)
    fe = A.MelFrontEnd(pp, device=DEV)
    gl = A.GriffinLim(front_end=fe, n_iters=4)
    pitch = A.PitchExtractor(pp, device=DEV)
    reads = []
    for name in ("item", "tolist"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name,
                            lambda self, _o=orig, _n=name: (reads.append(_n), _o(self))[1])
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for kw, f0 in ((dict(), False), (dict(vocoder=gl, pitch=pitch, front_end=fe), True),
                   (dict(pitch=pitch, front_end=fe), True)):
        reads.clear()
        figures, message = T.evaluate_synthesis(model, 7, val, batch_size=4, **kw)
        print(figures, message, reads)
        assert reads == ["tolist"]  # one host read per pass
        assert figures["utterances"] == len(val) == 13
        assert all(np.isfinite(figures[k]) for k in ("mcd_db", "length_error", "vuv_error"))
        assert figures["mcd_db"] > 0.0 and figures["length_error"] > -1.0
        assert message == T.synthesis_message(7, figures, f0=f0)
        assert message.startswith("Synthesis, Step 7, MCD: ") and (", F0 RMSE: " in message) == f0
        assert model.training
    batcher = C.CorpusBatcher(val, 4, group_size=1, shuffle=False, sort=False, drop_last=False)
    again = T.evaluate_synthesis(model, 7, batcher)[0]
    assert again["mcd_db"] == T.evaluate_synthesis(model, 7, val, batch_size=4)[0]["mcd_db"]
    after = model.state_dict()
    for k in before:  # no parameter and no BatchNorm buffer moved
        assert torch.equal(before[k], after[k]), k


def _train_config(tc, root):
    tc = copy.deepcopy(tc)
    tc["optimizer"]["batch_size"] = 4
    tc["step"] = dict(total_step=3, save_step=2, val_step=2, log_step=1, synth_step=2)
    tc["path"] = {k: os.path.join(root, k) for k in ("ckpt_path", "log_path", "result_path")}
    return tc


def test_fit_logs_the_synthesis_line_only_when_asked(corpus, configs, tmp_path):
    """The tiny run of test_gpu_corpus_store.py, three times: ``synth_eval`` absent, None and set.
    Absent and None write the same bytes -- the training and validation lines only, although
    ``synth_step`` divides step 2 --; set, the training log is still the same and the
    validation log gains one line at ``synth_step``."""
    store, val = corpus
    pp, mc, tc, _ = configs
    runs = {}
    for name, kw in (("absent", {}), ("none", dict(synth_eval=None)), ("set", dict(synth_eval={}))):
        cfg = _train_config(tc, str(tmp_path / name))
        model = _model(configs)
        g = torch.Generator()
        g.manual_seed(9)
        messages = []
        last = T.fit(T.Trainer(model, pp, mc, cfg), C.CorpusBatcher(store, 4, 4, generator=g),
                     C.CorpusBatcher(val, 4, group_size=1, shuffle=False, sort=False,
                                     drop_last=False), cfg, log=messages.append, **kw)
        assert last == 3
        logs = {}
        for part in ("train", "val"):
            with open(os.path.join(cfg["path"]["log_path"], part, "log.txt"), "rb") as f:
                logs[part] = f.read()
            assert os.listdir(os.path.join(cfg["path"]["log_path"], part)) == ["log.txt"]
        assert os.listdir(cfg["path"]["ckpt_path"]) == ["2.pth.tar"]
        runs[name] = (logs, messages)
    assert runs["absent"] == runs["none"]
    logs, messages = runs["none"]
    train_lines = logs["train"].decode().split("\n")
    assert [l.split(",")[0] for l in train_lines] == ["Step 1/3", "Step 2/3", "Step 3/3", ""]
    val_lines = logs["val"].decode().split("\n")
    assert len(val_lines) == 2 and val_lines[0].startswith("Validation Step 2, Total Loss: ")
    assert messages == train_lines[:2] + [val_lines[0]] + train_lines[2:3]
    logs_set, messages_set = runs["set"]
    assert logs_set["train"] == logs["train"]
    set_lines = logs_set["val"].decode().split("\n")
    assert set_lines[0] == val_lines[0] and len(set_lines) == 3 and set_lines[2] == ""
    assert set_lines[1].startswith("Synthesis, Step 2, MCD: ") and " dB, Length Error: " in set_lines[1]
    assert messages_set == train_lines[:2] + set_lines[:2] + train_lines[2:3]
    with pytest.raises(ValueError, match="validation batcher"):
        T.fit(T.Trainer(_model(configs), pp, mc, cfg), C.CorpusBatcher(store, 4, 4), None, cfg,
              synth_eval={})
