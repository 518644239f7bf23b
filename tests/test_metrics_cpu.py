"""Objective synthesis metrics, the parts that need no GPU: the numpy oracle against brute force
over every monotone path, the argument checks of the new entries, the DCT table, the arithmetic of
``summarise`` and the log line of ``evaluate_synthesis``."""
import importlib
import math

import numpy as np
import pytest
import torch

import dtw_oracle as O

PKG = "mid-attribute-speaker-generation_amd"
NEW = ("fs2_mfcc", "fs2_dtw_ws_bytes", "fs2_dtw", "fs2_path_metrics")


def test_oracle_equals_brute_force():
    """All-integer one-dimensional features: every local cost |a - b| and every sum of them is
    exact, so ties are exact too.  The oracle's cost must be the minimum over all monotone paths
    and its path the one the tie rule (diagonal, then (i-1, j), then (i, j-1)) picks."""
    rng = np.random.default_rng(5)
    shapes = [(t1, t2) for t1 in range(1, 6) for t2 in range(1, 6)]
    ties = 0
    for t1, t2 in shapes:
        for _ in range(4):
            a = rng.integers(0, 3, (t1, 1)).astype(np.float32)
            b = rng.integers(0, 3, (t2, 1)).astype(np.float32)
            cost, path = O.dtw(a, b)
            want_cost, want_path = O.brute_force(a, b)
            assert cost == want_cost, (t1, t2)
            assert np.array_equal(path, want_path), (t1, t2, path.tolist(), want_path.tolist())
            assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (t1 - 1, t2 - 1)
            assert set(map(tuple, np.diff(path, axis=0))) <= {(1, 1), (1, 0), (0, 1)}
            ties += O.path_ties(a, b)
            assert (O.path_gap(a, b) == 0) == (O.path_ties(a, b) > 0)
    assert ties > 50  # the tie rule was exercised, not avoided


def test_oracle_cost_is_the_accumulated_local_cost():
    rng = np.random.default_rng(6)
    a = rng.standard_normal((7, 3)).astype(np.float32)
    b = rng.standard_normal((9, 3)).astype(np.float32)
    cost, path = O.dtw(a, b)
    c = O.local_cost(a, b)
    total = c[0, 0]
    for i, j in path[1:]:
        total = total + c[i, j]  # the recurrence's order of adds
    assert cost == total
    assert O.dtw(a, a)[0] == 0.0 and np.array_equal(O.dtw(a, a)[1], np.stack([np.arange(7)] * 2, 1))


def test_dct_table_is_scipys_orthonormal_dct():
    M = importlib.import_module(PKG + ".metrics")
    x = np.random.default_rng(7).uniform(-11.6, 2.0, (5, 80))
    for k in (1, 13, 79):
        table = M.dct_table(80, k)
        assert table.dtype == np.float32 and table.shape == (80, k)
        np.testing.assert_allclose(x @ table.astype(np.float64), O.mfcc(x, k), atol=2e-5)
    for bad in (0, 80, 81):
        with pytest.raises(ValueError):
            M.dct_table(80, bad)


def test_entries_validate_arguments_before_any_launch():
    L = importlib.import_module(PKG + "._lib")
    assert set(NEW) <= set(L.lib.symbols())
    lib, p, big = L.lib, 16, 1 << 40  # p: a non-null placeholder, never dereferenced
    ws = lib.fs2_dtw_ws_bytes(2, 70, 90, 13)
    bad = [
        lambda: lib.fs2_mfcc(None, p, 2, 80, 7, 0, p, 13, p, 0),
        lambda: lib.fs2_mfcc(p, p, 2, 80, 7, 0, None, 13, p, 0),
        lambda: lib.fs2_mfcc(p, p, 2, 80, 7, 0, p, 13, None, 0),
        lambda: lib.fs2_mfcc(p, p, 2, 80, 7, 0, p, 0, p, 0),      # K = 0
        lambda: lib.fs2_mfcc(p, p, 2, 80, 7, 0, p, 80, p, 0),     # K = n_mels
        lambda: lib.fs2_mfcc(p, p, 2, 80, 7, 0, p, 81, p, 0),
        lambda: lib.fs2_mfcc(p, p, 2, 129, 7, 0, p, 13, p, 0),    # more mels than the tile holds
        lambda: lib.fs2_mfcc(p, p, 2, 80, 7, 2, p, 13, p, 0),     # no such layout
        lambda: lib.fs2_dtw(None, p, p, p, 2, 70, 90, 13, p, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, None, p, p, 2, 70, 90, 13, p, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, None, p, 2, 70, 90, 13, p, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, None, 2, 70, 90, 13, p, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 70, 90, 13, None, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 70, 90, 13, p, None, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 70, 90, 13, p, p, None, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 70, 90, 13, p, p, p, None, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 70, 90, 0, p, p, p, p, big, 0),      # K = 0
        lambda: lib.fs2_dtw(p, p, p, p, 2, 2049, 90, 13, p, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 70, 2049, 13, p, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 0, 90, 13, p, p, p, p, big, 0),
        lambda: lib.fs2_dtw(p, p, p, p, 2, 70, 90, 13, p, p, p, p, ws - 1, 0),  # one byte short
        lambda: lib.fs2_path_metrics(None, p, p, p, p, 2, 70, 90, None, None, p, 0),
        lambda: lib.fs2_path_metrics(p, None, p, p, p, 2, 70, 90, None, None, p, 0),
        lambda: lib.fs2_path_metrics(p, p, None, p, p, 2, 70, 90, None, None, p, 0),
        lambda: lib.fs2_path_metrics(p, p, p, None, p, 2, 70, 90, None, None, p, 0),
        lambda: lib.fs2_path_metrics(p, p, p, p, None, 2, 70, 90, None, None, p, 0),
        lambda: lib.fs2_path_metrics(p, p, p, p, p, 2, 70, 90, None, None, None, 0),
        lambda: lib.fs2_path_metrics(p, p, p, p, p, 2, 70, 90, p, None, p, 0),     # half a pair
        lambda: lib.fs2_path_metrics(p, p, p, p, p, 2, 2049, 90, None, None, p, 0),
        lambda: lib.fs2_path_metrics(p, p, p, p, p, 2, 70, 2049, None, None, p, 0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(L.KernelError):
            call()
            pytest.fail(f"call {k} was accepted")
    # an empty batch launches nothing and needs no operand
    assert lib.fs2_mfcc(None, None, 0, 80, 7, 0, None, 13, None, 0) == 0
    assert lib.fs2_dtw(None, None, None, None, 0, 70, 90, 13, None, None, None, None, 0, 0) == 0
    assert lib.fs2_path_metrics(None, None, None, None, None, 0, 70, 90, None, None, None, 0) == 0
    # one step byte per cell, diagonal-major over the shorter side, the reversed path and the
    # feature-major copy of both sequences
    assert ws == 2 * ((159 * 70 + 7) // 8 * 8 + 159 * 8 + 160 * 13 * 4)
    assert lib.fs2_dtw_ws_bytes(1, 2048, 2048, 1) == 4095 * 2048 + 4095 * 8 + 4096 * 4
    assert lib.fs2_dtw_ws_bytes(1, 3, 2048, 2) == (2050 * 3 + 7) // 8 * 8 + 2050 * 8 + 2051 * 8
    assert lib.fs2_dtw_ws_bytes(1, 2049, 3, 13) == 0 and lib.fs2_dtw_ws_bytes(0, 3, 3, 13) == 0
    assert lib.fs2_dtw_ws_bytes(1, 3, 3, 0) == 0


def test_wrappers_reject_host_tensors_and_bad_shapes():
    K = importlib.import_module(PKG + ".kernels")
    M = importlib.import_module(PKG + ".metrics")
    a = torch.zeros(1, 4, 3)
    n = torch.ones(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="on the GPU"):
        K.dtw(a, a, n, n)
    with pytest.raises(RuntimeError, match="on the GPU"):
        M.mfcc(torch.zeros(1, 80, 4), n)
    assert M.FIELDS == O.FIELDS and len(M.FIELDS) == K.METRIC_FIELDS == M.DVEC_COS
    assert [M.PATH_LEN, M.MCD_DB, M.FRAMES_A, M.FRAMES_B, M.N_VV, M.F0_SQ_CENTS, M.N_VUV,
            M.LEN_ERR] == list(range(8))


def test_summarise_arithmetic():
    M = importlib.import_module(PKG + ".metrics")
    #                 path_len mcd  fa   fb   n_vv  sq     n_vuv len_err
    rec = torch.tensor([[10.0, 4.0, 8.0, 10.0, 4.0, 400.0, 1.0, -0.2],
                        [30.0, 6.0, 30.0, 20.0, 12.0, 1200.0, 3.0, 0.5]], dtype=torch.float64)
    s = M.summarise(rec)
    assert s["utterances"] == 2 and s["mcd_db"] == 5.0  # the mean over utterances, not frames
    assert s["length_error"] == (-0.2 + 0.5) / 2
    assert s["f0_rmse_cents"] == math.sqrt(1600.0 / 16.0) == 10.0
    assert s["vuv_error"] == 4.0 / 40.0 and "dvector_cos" not in s
    with_cos = torch.cat([rec, torch.tensor([[0.5], [0.7]], dtype=torch.float64)], 1)
    assert M.summarise(with_cos)["dvector_cos"] == (0.5 + 0.7) / 2
    unvoiced = rec.clone()
    unvoiced[:, M.N_VV] = 0
    assert math.isnan(M.summarise(unvoiced)["f0_rmse_cents"])
    with pytest.raises(ValueError):
        M.summarise(rec[:, :7])
    # the oracle's record has the same layout and the same arithmetic
    path = np.array([[0, 0], [1, 1], [2, 1], [3, 2]], np.int32)
    r = O.path_metrics(3.0, path, 4, 3, fa=[100, 200, 0, 0], fb=[100, 100, 0])
    assert r.tolist() == [4.0, 10.0 / np.log(10.0) * np.sqrt(2.0) * 3.0 / 4, 4.0, 3.0, 2.0,
                          1200.0 ** 2, 1.0, (4 - 3) / 3]


def test_synthesis_message_format():
    T = importlib.import_module(PKG + ".train")
    figures = {"mcd_db": 7.12345, "length_error": -0.0412, "f0_rmse_cents": 183.26,
               "vuv_error": 0.1234, "utterances": 13}
    assert T.synthesis_message(500, figures) == \
        "Synthesis, Step 500, MCD: 7.123 dB, Length Error: -4.12%"
    assert T.synthesis_message(500, figures, f0=True) == \
        "Synthesis, Step 500, MCD: 7.123 dB, Length Error: -4.12%, F0 RMSE: 183.3 cents, " \
        "V/UV Error: 12.34%"
    figures["length_error"] = 0.25
    assert ", Length Error: +25.00%" in T.synthesis_message(1, figures)
    import inspect
    sig = inspect.signature(T.fit)
    assert sig.parameters["synth_eval"].default is None
    assert list(inspect.signature(T.evaluate_synthesis).parameters)[:7] == [
        "model", "step", "store_or_batcher", "batch_size", "vocoder", "pitch", "front_end"]
