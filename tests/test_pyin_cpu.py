"""The pYIN oracle (``pyin_oracle.py``) against ground truth -- brute-force path enumeration, a
numeric integral of the Beta density, clean tones, silence, and the noisy-voice contrast with
plain YIN that the method is there for -- and the host side of the pYIN entry points.  No GPU."""
import copy
import importlib

import numpy as np
import pytest
import torch

import pitch_oracle as O
import pyin_oracle as P

NAME = "mid-attribute-speaker-generation_amd"
PKG = importlib.import_module(NAME)
AUDIO = importlib.import_module(NAME + ".audio")
PRE = importlib.import_module(NAME + ".preprocess")
NEW = ("fs2_f0_pyin_candidates", "fs2_f0_pyin_viterbi_ws_bytes", "fs2_f0_pyin_viterbi",
       "fs2_f0_pyin_ws_bytes", "fs2_f0_pyin")


# ------------------------------------------------------------------ the Viterbi pass
def _tiny_obs(F, seed):
    """Sparse masses over 3 bins -> the observation matrix (F, 6)."""
    rng = np.random.default_rng(seed)
    mass = rng.random((F, 3)) * (rng.random((F, 3)) < 0.6) / 3.0
    return P.observations(mass, np.minimum(mass.sum(axis=1), 1.0))


@pytest.mark.parametrize("F", (1, 2, 4))
def test_viterbi_equals_brute_force_enumeration(F):
    trans = P.transition(3, P.tri_table(1))
    assert trans.shape == (6, 6) and trans[0, 2] == 0.0 and trans[0, 3] == 0.5 * 0.01
    for seed in range(12):
        obs = _tiny_obs(F, 100 * F + seed)
        assert np.array_equal(P.viterbi(obs, trans), P.viterbi_brute(obs, trans)), (F, seed)


@pytest.mark.parametrize("F", (1, 2, 4))
def test_viterbi_ties_go_to_the_first_index(F):
    trans = P.transition(3, P.tri_table(1))
    # all-equal observations: every constant path ties; the lowest state wins at every frame
    obs = np.ones((F, 6))
    assert P.viterbi(obs, trans).tolist() == [0] * F
    assert P.viterbi_brute(obs, trans).tolist() == [0] * F
    # dyadic transitions and observations: every product is exact, so equal paths tie exactly
    rng = np.random.default_rng(F)
    ties = 0
    for _ in range(20):
        dy = 0.5 ** rng.integers(1, 3, (6, 6)) * (rng.random((6, 6)) < 0.8)
        obs = 0.5 ** rng.integers(0, 2, (F, 6))
        got, want = P.viterbi(obs, dy), P.viterbi_brute(obs, dy)
        assert np.array_equal(got, want)
        ties += int(got[-1] != 5)
    assert ties > 0


# ------------------------------------------------------------------ the host tables
def test_beta_table_matches_a_numeric_integral_and_sums_to_one():
    w = P.beta_weights()
    # past theta = 0.85 the closed form's terms fall below the rounding of 1: those masses are 0
    assert w.shape == (100,) and (w >= 0).all() and (w[:80] > 0).all()
    assert abs(w.sum() - 1.0) <= 64 * np.finfo(np.float64).eps
    # Simpson's rule over the Beta(2, 18) density 342 x (1 - x)^17 on 2000 intervals per step
    th = P.thresholds()
    for i in (1, 2, 5, 15, 50, 100):
        x = np.linspace(th[i - 1], th[i], 2001)
        y = 342.0 * x * (1.0 - x) ** 17
        h = (th[i] - th[i - 1]) / 2000.0
        integral = h / 3.0 * (y[0] + y[-1] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum())
        assert abs(integral - w[i - 1]) <= 1e-12, i
    assert P.thresholds()[15] == float(np.float32(0.15)) and P.beta_cdf(1.0) == 1.0
    assert P.bin_count() == 210 and P.reach() == 25 and P.reach(200, 22050) == 20
    tri = P.tri_table(25)
    assert tri[0] == 26 / 676 and tri[25] == 1 / 676
    assert abs(tri[0] + 2.0 * tri[1:].sum() - 1.0) <= 1e-15  # a distribution inside the range


def test_package_tables_are_the_oracles_bitwise():
    for hop, sr, lo, hi in ((256, 22050, 71.0, 800.0), (200, 22050, 44.0, 700.0),
                            (256, 16000, 350.0, 700.0)):
        prior, tri, centres = AUDIO.pyin_tables(hop, sr, lo, hi)
        assert prior.dtype == tri.dtype == np.float64 and centres.dtype == np.float32
        assert np.array_equal(prior, P.beta_weights())
        assert np.array_equal(tri, P.tri_table(P.reach(hop, sr)))
        assert np.array_equal(centres, P.bin_centres(P.bin_count(lo, hi), lo))


# ------------------------------------------------------------------ the estimator
@pytest.mark.parametrize("hz", (110.0, 220.0, 440.0))
def test_clean_tone_is_voiced_throughout_with_yins_f0(hz):
    x = O.voice(6000, hz, hz, seed=int(hz), snr_db=30.0)
    yin = O.oracle64(x)[0]
    got = P.oracle64(x)
    assert (got["f0"] > 0).all() and (got["states"] < P.bin_count()).all()
    # the same pick and parabola: the same f0 wherever plain YIN has one, and the track carries
    # the voicing over the edge frames YIN drops
    assert np.array_equal(got["f0"][yin > 0], yin[yin > 0])
    inner = slice(2, -2)  # the frames whose window lies inside the signal
    assert (yin[inner] > 0).all()
    assert np.abs(got["f0"][inner] - hz).max() <= 5e-3 * hz
    assert (got["unvoiced"][inner] < 0.1).all()


def test_silence_and_dc_have_no_voiced_frame():
    for x in (np.zeros(4096, np.float32), np.full(4096, 0.5, np.float32)):
        for fn in (P.oracle64, P.ref32):
            got = fn(x)
            assert not got["f0"].any() and (got["states"] >= P.bin_count()).all()
            assert np.isfinite(got["unvoiced"]).all()


def _score(f0, n, hop=256):
    """(scored frames, voiced scored frames, missed voiced, V/UV errors, gross errors) of a
    contour of ``voice(n, 110, 170, ..., gaps=((6000, 9000),))``; frames outside the gap whose
    centre lies within 400 samples of it are left out."""
    c = np.arange(len(f0)) * hop
    truth = 110.0 + 60.0 * c / (n - 1)
    in_gap = (c >= 6000) & (c < 9000)
    edge = ~in_gap & ((np.abs(c - 6000) < 400) | (np.abs(c - 9000) < 400))
    keep, voiced = ~edge, ~in_gap
    got = f0 > 0
    vuv = keep & (got != voiced)
    both = keep & got & voiced
    cents = np.abs(1200.0 * np.log2(np.where(both, f0, truth) / truth))
    return (int(keep.sum()), int((keep & voiced).sum()), int((keep & voiced & ~got).sum()),
            int(vuv.sum()), int((cents > 100.0).sum()))


@pytest.mark.parametrize("seed", (1, 2))
def test_noisy_voice_contrast_with_plain_yin(seed):
    """What pYIN is for: at 3 dB SNR plain YIN's fixed threshold calls the voice unvoiced, the
    threshold distribution and the track do not."""
    n = 16384
    x = O.voice(n, 110, 170, seed, 3.0, gaps=((6000, 9000),))
    yin = _score(O.oracle64(x)[0], n)
    pyin = _score(P.oracle64(x)["f0"].astype(np.float64), n)
    print(f"seed {seed}: scored {yin[0]} (voiced {yin[1]}); YIN misses {yin[2]}, V/UV {yin[3]}; "
          f"pYIN V/UV {pyin[3]}, gross {pyin[4]}")
    assert yin[0] == 62
    assert 2 * yin[2] >= yin[1]
    assert 10 * (pyin[3] + pyin[4]) <= pyin[0]


def test_ref32_decodes_what_oracle64_decodes():
    """What the GPU comparison with the float64 oracle rests on: on the inputs of
    test_gpu_pyin.py the float32 formulation changes the decoded state on at most 2 % of an
    input's frames."""
    for tag, x, kw in P.cases():
        a, b = P.want(tag, x, **kw)
        diff = int((a["states"] != b["states"]).sum())
        print(f"{tag}: {len(a['states'])} frames, {diff} differ")
        assert diff <= 0.02 * len(a["states"]), tag


# ------------------------------------------------------------------ the host side
def _config():
    return copy.deepcopy(PKG.config.load_configs("JVS-VCTK")[0])


def test_pitch_extractor_method_argument():
    px = AUDIO.PitchExtractor(device="cpu")
    assert px.method == "yin" and px.tables is None  # the default builds no table
    py = AUDIO.PitchExtractor(device="cpu", method="pyin", threshold=0.3)
    prior, tri, centres = py.tables
    assert py.method == "pyin" and prior.dtype == tri.dtype == torch.float64
    assert centres.dtype == torch.float32
    assert (prior.numel(), tri.numel(), centres.numel()) == (100, 26, 210)
    assert py.n_frames(6000) == 24
    with pytest.raises(ValueError, match="nope"):
        AUDIO.PitchExtractor(device="cpu", method="nope")
    with pytest.raises(ValueError, match="512"):
        AUDIO.PitchExtractor(device="cpu", method="pyin", f0_floor=40.0)
    with pytest.raises(ValueError):
        AUDIO.PitchExtractor(device="cpu", method="pyin", f0_floor=900.0)
    slow = _config()
    slow["audio"]["sampling_rate"], slow["stft"]["hop_length"] = 2000, 1024
    AUDIO.PitchExtractor(slow, device="cpu", f0_floor=10.0, f0_ceil=400.0)
    with pytest.raises(ValueError, match="reach"):
        AUDIO.PitchExtractor(slow, device="cpu", f0_floor=10.0, f0_ceil=400.0, method="pyin")


def test_feature_extractor_and_cli_take_the_method():
    fx = PRE.FeatureExtractor(_config(), device="cpu", pitch_method="pyin")
    assert fx.pitcher.method == "pyin" and fx.pitcher.tables is not None
    assert PRE.FeatureExtractor(_config(), device="cpu").pitcher.method == "yin"
    with pytest.raises(ValueError, match="nope"):
        PRE.FeatureExtractor(_config(), device="cpu", pitch_method="nope")
    with pytest.raises(SystemExit):
        PRE.main(["--config", "nowhere", "--pitch_method", "nope"])
    with pytest.raises(SystemExit):
        importlib.import_module(NAME + ".train").main(["-c", "nowhere", "--synth_pitch", "nope"])


def test_entries_validate_arguments_before_any_launch():
    L = importlib.import_module(NAME + "._lib")
    assert set(NEW) <= set(L.lib.symbols())
    lib, p, big = L.lib, 16, 1 << 40  # p: a non-null placeholder, never dereferenced
    cand = lambda **k: lib.fs2_f0_pyin_candidates(  # noqa: E731
        k.get("wav", p), p, 2, k.get("S", 4096), k.get("hop", 256), 22050.0, k.get("lo", 71.0),
        k.get("hi", 800.0), k.get("prior", p), k.get("nb", 210), k.get("mass", p), p, p, None, p, 0)
    vit = lambda **k: lib.fs2_f0_pyin_viterbi(  # noqa: E731
        k.get("mass", p), p, None, 2, k.get("F", 17), k.get("nb", 210), k.get("tri", p),
        k.get("R", 25), k.get("cf0", None), None, k.get("path", p), k.get("f0", None), p,
        k.get("ws", big), 0)
    full = lambda **k: lib.fs2_f0_pyin(  # noqa: E731
        k.get("wav", p), None, 2, 4096, k.get("hop", 256), 22050.0, k.get("lo", 71.0), 800.0, p,
        k.get("tri", p), k.get("R", 25), p, k.get("nb", 210), p, k.get("unv", p), p, None, p,
        k.get("ws", big), 0)
    need_v = lib.fs2_f0_pyin_viterbi_ws_bytes(2, 17, 210)
    need = lib.fs2_f0_pyin_ws_bytes(2, 4096, 256, 210)
    bad = [
        lambda: cand(wav=None), lambda: cand(prior=None), lambda: cand(mass=None),
        lambda: cand(hop=0), lambda: cand(hop=1025), lambda: cand(S=0), lambda: cand(lo=40.0),
        lambda: cand(lo=900.0), lambda: cand(nb=0), lambda: cand(nb=1025),
        lambda: vit(mass=None), lambda: vit(tri=None), lambda: vit(path=None), lambda: vit(F=0),
        lambda: vit(nb=0), lambda: vit(nb=1025), lambda: vit(R=-1), lambda: vit(R=1024),
        lambda: vit(f0=p), lambda: vit(f0=p, cf0=p),  # a contour needs cand_f0 and the centres
        lambda: vit(ws=need_v - 1),
        lambda: full(wav=None), lambda: full(tri=None), lambda: full(unv=None),
        lambda: full(hop=0), lambda: full(lo=40.0), lambda: full(nb=1025), lambda: full(R=1024),
        lambda: full(ws=need - 1),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(L.KernelError):
            call()
            pytest.fail(f"call {k} was accepted")
    # an empty batch launches nothing and needs no operand
    assert lib.fs2_f0_pyin_candidates(None, None, 0, 4096, 256, 22050.0, 71.0, 800.0, None, 210,
                                      None, None, None, None, None, 0) == 0
    assert lib.fs2_f0_pyin_viterbi(None, None, None, 0, 17, 210, None, 25, None, None, None, None,
                                   None, 0, 0) == 0
    assert lib.fs2_f0_pyin(None, None, 0, 4096, 256, 22050.0, 71.0, 800.0, None, None, 25, None,
                           210, None, None, None, None, None, 0, 0) == 0
    # int16 back-pointers per (frame, state); masses, voiced, candidate f0, states before them
    assert need_v == 2 * 17 * 420 * 2
    n = 2 * 17
    assert need == n * 210 * 8 + n * 8 + n * 210 * 4 + n * 4 + need_v
    assert lib.fs2_f0_pyin_viterbi_ws_bytes(0, 17, 210) == 0
    assert lib.fs2_f0_pyin_viterbi_ws_bytes(2, 17, 1025) == 0
    assert lib.fs2_f0_pyin_ws_bytes(2, 4096, 0, 210) == 0


def test_wrappers_reject_host_tensors():
    K = importlib.import_module(NAME + ".kernels")
    prior, tri, centres = AUDIO.PitchExtractor(device="cpu", method="pyin").tables
    wav = torch.zeros(1, 2048)
    with pytest.raises(RuntimeError, match="GPU"):
        K.f0_pyin(wav, None, 256, 22050, 71.0, 800.0, prior, tri, centres)
    with pytest.raises(RuntimeError, match="GPU"):
        K.f0_pyin_candidates(wav, None, 256, 22050, 71.0, 800.0, prior, 210)
    with pytest.raises(RuntimeError, match="GPU"):
        K.f0_pyin_viterbi(torch.zeros(1, 3, 3, dtype=torch.float64),
                          torch.zeros(1, 3, dtype=torch.float64), None, tri)
