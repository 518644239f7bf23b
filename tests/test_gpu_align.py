"""The aligner on the GPU: the four kernels of csrc/align.hip against ``align_oracle``, one
training step against the model in plain torch, convergence on the oracle's synthetic corpus, and
``align.main`` end to end into ``Preprocessor.build_from_path``.

Tolerances: the project's fp32 bar for everything in floating point -- ``close()`` of
tests/test_gpu_parity.py, max abs error <= 1e-4 x the oracle's largest magnitude, the oracle in
fp64 from the same fp32 inputs -- and ``torch.equal`` for the MAS durations (one IEEE fp32 add
and one compare per cell: numpy gives the same bits).

Convergence.  ``align_oracle.oracle_agreement`` (the torch model on the CPU, 100 Adam steps of
batches of 8, temperature 0.05, omega 1) gave on seeds 0..4 a frame agreement between the MAS
path and the true path of 0.797, 0.885, 0.845, 0.826, 0.858 (untrained 0.571, 0.584, 0.586,
0.570, 0.578): mean 0.842, sample standard deviation 0.033, the spread.  The test trains seed 1
from the oracle's initial weights over the oracle's batches and asks for its agreement minus
twice that spread (trajectories differ by reduction order, not by more than seeds do), and for
0.70, clear of the untrained 0.60.  Boundary frames are ambiguous under a k = 3 query conv: the
agreement plateaus below 1.
"""
import copy
import importlib
import os
import wave

import numpy as np
import pytest
import torch

import align_oracle as O
import pitch_oracle as PO

NAME = "mid-attribute-speaker-generation_amd"
PKG = importlib.import_module(NAME)
K = importlib.import_module(NAME + ".kernels")
AL = importlib.import_module(NAME + ".aligner")
pytestmark = pytest.mark.gpu
DEV = "cuda"

LENS = [(1, 1), (1, 9), (7, 7), (7, 8), (64, 200), (65, 200), (130, 300)]  # (N, M)
B, A, TEMP = 3, 40, 0.05
SEED, SPREAD = 1, 0.033


def close(a, b, rtol=1e-4, what=""):
    """``close`` of tests/test_gpu_parity.py."""
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    scale = max(np.abs(b).max(), 1e-6)
    err = np.abs(a - b).max()
    print(f"{what}: max abs err {err:.3e} vs scale {scale:.3e}")
    assert err <= rtol * scale, f"{what}: max abs err {err:.3e} vs scale {scale:.3e}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _batch(N, M):
    """A ragged batch of three whose longest row is (N, M), padded past every row."""
    lens = [(N, M), (max(1, N // 2), max(1, N // 2, M - 3)), (max(1, N - 1), M)]
    return lens, max(n for n, _ in lens) + 3, max(m for _, m in lens) + 5


_CASES = {}


def case(N, M):
    """Inputs and fp64 oracle results of one (N, M), computed once and shared."""
    if (N, M) in _CASES:
        return _CASES[(N, M)]
    lens, T_s, T_m = _batch(N, M)
    rng = np.random.default_rng(100 * N + M)
    c = {"lens": lens, "T_s": T_s, "T_m": T_m,
         "q": rng.standard_normal((B, T_m, A)).astype(np.float32),
         "k": rng.standard_normal((B, T_s, A)).astype(np.float32),
         "g": rng.standard_normal((B, T_m, T_s)).astype(np.float32),
         "w": rng.uniform(0.01, 0.1, B).astype(np.float32),
         "src": np.asarray([n for n, _ in lens], np.int64),
         "mel": np.asarray([m for _, m in lens], np.int64)}
    for omega in (0.0, 1.0):
        lp, dq, dk = [], [], []
        for b, (n, m) in enumerate(lens):
            q = torch.from_numpy(c["q"][b]).requires_grad_()
            k = torch.from_numpy(c["k"][b]).requires_grad_()
            out = O.logprob(q, k, n, m, TEMP, omega)
            live = torch.zeros(T_m, T_s, dtype=torch.float64)
            live[:m, :n] = 1.0
            (out * torch.from_numpy(c["g"][b]).double() * live).sum().backward()
            lp.append(out.detach().numpy()), dq.append(q.grad.numpy()), dk.append(k.grad.numpy())
        c[omega] = {"logp": np.stack(lp), "dq": np.stack(dq), "dk": np.stack(dk)}
    # the loss kernels are fed the fp32 rounding of the oracle's log-probabilities
    c["logp32"] = c[1.0]["logp"].astype(np.float32)
    nll, grad = [], np.zeros((B, T_m, T_s))
    for b, (n, m) in enumerate(lens):
        v, g = O.forward_sum(c["logp32"][b], n, m)
        nll.append(v)
        grad[b, :m, :n] = g * float(c["w"][b])
    c["nll"], c["grad"] = np.asarray(nll), grad
    c["dur"] = np.zeros((B, T_s), np.int64)
    for b, (n, m) in enumerate(lens):
        c["dur"][b, :n] = O.mas(c["logp32"][b], n, m)
    _CASES[(N, M)] = c
    return c


def _dead(x, lens):
    """True where every cell past a row's (n, m) is exactly 0."""
    x = x.cpu().numpy()
    return all(not x[b, m:].any() and not x[b, :, n:].any() for b, (n, m) in enumerate(lens))


@pytest.mark.parametrize("N,M", LENS)
@pytest.mark.parametrize("omega", [0.0, 1.0], ids=["no-prior", "prior"])
def test_align_logprob_forward_and_backward(N, M, omega):
    c = case(N, M)
    q, k, g, src, mel = (_dev(c[x]) for x in ("q", "k", "g", "src", "mel"))
    logp = K.align_logprob(q, k, src, mel, TEMP, omega)
    close(logp, c[omega]["logp"], what=f"logp {N}x{M}")
    assert _dead(logp, c["lens"])
    dq, dk = K.align_logprob_bwd(q, k, g, src, mel, TEMP)
    close(dq, c[omega]["dq"], what=f"dq {N}x{M}")
    close(dk, c[omega]["dk"], what=f"dk {N}x{M}")
    for b, (n, m) in enumerate(c["lens"]):
        assert not dq[b, m:].any() and not dk[b, n:].any()
    # each row alone: the same bits
    for b in range(B):
        one = K.align_logprob(q[b:b + 1], k[b:b + 1], src[b:b + 1], mel[b:b + 1], TEMP, omega)
        assert torch.equal(one[0], logp[b])
        dq1, dk1 = K.align_logprob_bwd(q[b:b + 1], k[b:b + 1], g[b:b + 1], src[b:b + 1],
                                       mel[b:b + 1], TEMP)
        assert torch.equal(dq1[0], dq[b]) and torch.equal(dk1[0], dk[b])


@pytest.mark.parametrize("N,M", LENS)
def test_forward_sum(N, M):
    c = case(N, M)
    logp, src, mel, w = (_dev(c[x]) for x in ("logp32", "src", "mel", "w"))
    nll, grad = K.forward_sum(logp, src, mel, w, (c["src"], c["mel"]))
    close(nll, c["nll"], what=f"nll {N}x{M}")
    close(grad, c["grad"], what=f"grad {N}x{M}")
    assert _dead(grad, c["lens"])
    for b in range(B):
        n1, g1 = K.forward_sum(logp[b:b + 1], src[b:b + 1], mel[b:b + 1], w[b:b + 1])
        assert torch.equal(n1[0], nll[b]) and torch.equal(g1[0], grad[b])
    again = K.forward_sum(logp, src, mel, w)
    assert torch.equal(again[0], nll) and torch.equal(again[1], grad)  # run to run


@pytest.mark.parametrize("N,M", LENS)
def test_mas(N, M):
    c = case(N, M)
    logp, src, mel = (_dev(c[x]) for x in ("logp32", "src", "mel"))
    dur = K.mas(logp, src, mel, (c["src"], c["mel"]))
    assert dur.dtype == torch.int64 and torch.equal(dur.cpu(), torch.from_numpy(c["dur"]))
    for b, (n, m) in enumerate(c["lens"]):
        assert int(dur[b].sum()) == m and bool((dur[b, :n] >= 1).all())
    for b in range(B):
        assert torch.equal(K.mas(logp[b:b + 1], src[b:b + 1], mel[b:b + 1])[0], dur[b])


def test_mas_ties_take_the_diagonal():
    """Small integers: sums are exact, so equal-score paths tie exactly."""
    rng = np.random.default_rng(7)
    lens = [(5, 9), (7, 8), (70, 140)]
    T_s, T_m = 72, 143
    x = rng.integers(-1, 1, (3, T_m, T_s)).astype(np.float32)
    x[1] = 0.0  # every path ties
    want = np.zeros((3, T_s), np.int64)
    for b, (n, m) in enumerate(lens):
        want[b, :n] = O.mas(x[b], n, m)
    src, mel = np.asarray([n for n, _ in lens], np.int64), np.asarray([m for _, m in lens], np.int64)
    dur = K.mas(_dev(x), _dev(src), _dev(mel))
    assert torch.equal(dur.cpu(), torch.from_numpy(want))
    assert want[1, :7].tolist() == [2, 1, 1, 1, 1, 1, 1]  # all ties: down as soon as possible


def test_rows_without_a_path():
    """Fewer frames than phonemes: the wrappers raise where the lengths are on the host; on the
    device the row's nll is +inf, its gradient and its durations 0, and the other rows stand."""
    c = case(7, 8)
    logp, w = _dev(c["logp32"]), _dev(c["w"])
    src, mel = c["src"].copy(), c["mel"].copy()
    mel[0] = src[0] - 1
    for call in (lambda: K.mas(logp, _dev(src), _dev(mel), (src, mel)),
                 lambda: K.forward_sum(logp, _dev(src), _dev(mel), w, (src, mel))):
        with pytest.raises(RuntimeError, match="no monotonic path"):
            call()
    nll, grad = K.forward_sum(logp, _dev(src), _dev(mel), w)
    dur = K.mas(logp, _dev(src), _dev(mel))
    assert bool(torch.isinf(nll[0])) and float(nll[0]) > 0 and not grad[0].any() and not dur[0].any()
    close(nll[1:], c["nll"][1:], what="nll of the other rows")
    assert torch.equal(dur[1:].cpu(), torch.from_numpy(c["dur"][1:]))


# ------------------------------------------------------------------ the model
def _models(seed):
    """The oracle's torch model and an ``Aligner`` with the same weights."""
    ref = O.new_model(seed)
    model = AL.Aligner(O.N_SYMBOLS + 1, O.N_MELS, O.CHANNELS, O.ATTN_DIM, DEV)
    model.load_state_dict(ref.state_dict())
    return ref, model


def test_one_training_step_against_torch():
    """Seeded weights (``seeded.py``); loss and every parameter gradient against the plain-torch
    model on the CPU in fp64."""
    corpus = O.synth_corpus(0)
    ref = O.TorchAligner(O.N_SYMBOLS + 1, O.N_MELS, O.CHANNELS, O.ATTN_DIM)
    PKG.seeded.load_seeded_(ref)
    with torch.no_grad():
        ref.embedding.weight[0].zero_()  # padding_idx
    model = AL.Aligner(O.N_SYMBOLS + 1, O.N_MELS, O.CHANNELS, O.ATTN_DIM, DEV)
    model.load_state_dict(ref.state_dict())
    assert set(model.state_dict()) == set(ref.state_dict())
    ref = ref.double()
    texts, src_lens, mels, mel_lens = O.take(corpus, np.asarray([0, 3, 5, 9, 17]))
    want = ref.loss(texts, src_lens, mels.double(), mel_lens, O.TEMPERATURE, O.OMEGA)
    want.backward()
    tr = AL.AlignerTrainer(model, O.LR, O.TEMPERATURE, O.OMEGA)
    loss = tr.backward(texts.to(DEV), src_lens.to(DEV), mels.to(DEV), mel_lens.to(DEV))
    close(loss, want, what="loss")
    got = dict(model.named_parameters())
    for name, p in ref.named_parameters():
        close(got[name].grad, p.grad, what=name)
    assert not got["embedding.weight"].grad[0].any()
    again = tr.train_step(texts.to(DEV), src_lens.to(DEV), mels.to(DEV), mel_lens.to(DEV))
    assert torch.equal(again, loss) and tr.step == 1  # the same step, then the update


@pytest.fixture(scope="module")
def oracle_run():
    return O.oracle_agreement(SEED)


def test_convergence_on_the_synthetic_corpus(oracle_run):
    untrained, trained = oracle_run
    assert trained >= 0.80 and untrained <= 0.65  # conditions on the inputs
    corpus = O.synth_corpus(SEED)
    _, model = _models(SEED)
    tr = AL.AlignerTrainer(model, O.LR, O.TEMPERATURE, O.OMEGA)
    dev = {k: _dev(v) for k, v in corpus.items()}

    def take(idx):
        sl, ml = corpus["src_lens"][idx], corpus["mel_lens"][idx]
        i = _dev(idx)
        return (dev["texts"][i][:, :sl.max()].contiguous(), dev["src_lens"][i],
                dev["mels"][i][:, :ml.max()].contiguous(), dev["mel_lens"][i])

    losses = tr.fit([take(idx) for idx in O.batch_order(SEED)], O.STEPS)
    assert len(losses) == O.STEPS and tr.step == O.STEPS
    dur = tr.align(*take(np.arange(O.N_UTT))).cpu().numpy()
    got = O.agreement(dur, corpus)
    print(f"agreement {got:.3f}, oracle {trained:.3f} (untrained {untrained:.3f}); loss "
          f"{float(losses[0]):.4f} -> {float(losses[-1]):.4f}")
    assert float(losses[-1]) < float(losses[0])
    assert got >= trained - 2 * SPREAD
    assert got > 0.70


def test_save_and_load(tmp_path):
    corpus = O.synth_corpus(2)
    _, model = _models(2)
    tr = AL.AlignerTrainer(model, O.LR, O.TEMPERATURE, O.OMEGA)
    batch = tuple(t.to(DEV) for t in O.take(corpus, np.arange(4)))
    tr.train_step(*batch)
    tr.save(str(tmp_path / "a.pt"))
    want = tr.align(*batch)
    _, other = _models(3)
    tr2 = AL.AlignerTrainer(other).load(str(tmp_path / "a.pt"))
    assert tr2.step == 1 and torch.equal(tr2.align(*batch), want)
    assert torch.equal(tr2.train_step(*batch), tr.train_step(*batch))


# ------------------------------------------------------------------ end to end
UTTS = {"a0": ("spkA", 24000, 0.50, (120.0, 150.0), "a k o i"),
        "a1": ("spkA", 48000, 0.60, (200.0, 170.0), "{k a sp i o}"),
        "b0": ("spkB", 22050, 0.45, (230.0, 190.0), "o i"),
        "b1": ("spkB", 24000, 0.55, (160.0, 210.0), "i k a k o i a")}


def _write_wav(path, x, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(sr)
        w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())


def test_align_main_then_build_from_path(tmp_path, capsys):
    import yaml
    PRE, ALIGN, IO = (importlib.import_module(f"{NAME}.{m}") for m in ("preprocess", "align",
                                                                      "corpus_io"))
    raw, pre, cfg_dir = (str(tmp_path / d) for d in ("raw", "pre", "config"))
    os.makedirs(cfg_dir)
    for k, (speaker, sr, seconds, glide, phn) in UTTS.items():
        os.makedirs(os.path.join(raw, speaker), exist_ok=True)
        n = int(round(seconds * sr))
        x = PO.voice(n, glide[0] * PO.SR / sr, glide[1] * PO.SR / sr, seed=len(k) + n)
        _write_wav(os.path.join(raw, speaker, f"{k}.wav"), x, sr)
        with open(os.path.join(raw, speaker, f"{k}.lab"), "w") as f:
            f.write(f"text of {k}\n")
        with open(os.path.join(raw, speaker, f"{k}.phn"), "w") as f:
            f.write(phn + "\n")
    pp = copy.deepcopy(PKG.config.load_configs("JVS-VCTK")[0])
    pp.update(val_size=0.25, test_size=0.25, text={"text_cleaners": []}, accent={"use_accent": False})
    pp["mel"].update(mel_fmin=0, mel_fmax=8000)
    corpus_cfg = {"dataset": "toy", "path": {"raw_path": raw, "preprocessed_path": pre}}
    with open(os.path.join(cfg_dir, "preprocess.yaml"), "w") as f:
        yaml.safe_dump(pp, f)
    with open(os.path.join(cfg_dir, "preprocess_toy.yaml"), "w") as f:
        yaml.safe_dump(corpus_cfg, f)
    config = dict(corpus_cfg, preprocessing=pp)
    with pytest.raises(ValueError, match="TextGrid"):  # what the corpus lacked
        PRE.Preprocessor(config, batch=4, seed=3).build_from_path()
    # a hand-made alignment is left alone
    kept = os.path.join(pre, "TextGrid", "spkB", "b0.TextGrid")
    os.makedirs(os.path.dirname(kept))
    IO.write_textgrid(kept, ["o", "i"], [20, 15], 256, 22050)
    with open(kept, "rb") as f:
        kept_bytes = f.read()
    (written, left), = ALIGN.main(["--config", cfg_dir, "--corpus", "toy", "--steps", "5",
                                   "--batch", "2", "--seed", "4"])
    assert "wrote 3 TextGrids, left 1" in capsys.readouterr().out
    assert left == [kept] and open(kept, "rb").read() == kept_bytes
    assert sorted(os.path.basename(p) for p in written) == ["a0.TextGrid", "a1.TextGrid",
                                                            "b1.TextGrid"]
    aligned, rs = {}, importlib.import_module(NAME + ".audio").Resampler(22050, DEV)
    for p in written:
        k = os.path.basename(p).split(".")[0]
        tier = IO.read_textgrid(p)["phones"]
        phones = UTTS[k][4].strip("{}").split()
        assert [t for _, _, t in tier] == phones
        aligned[k] = PRE.durations_from_intervals(tier, 22050, 256)[1]
        assert len(aligned[k]) == len(phones) and min(aligned[k]) >= 1
        # the first L // hop frames of the file at the configured rate
        n_in = int(round(UTTS[k][2] * UTTS[k][1]))
        assert sum(aligned[k]) == rs.out_len(n_in, UTTS[k][1]) // 256
    out = PRE.Preprocessor(config, batch=4, seed=3).build_from_path()
    assert sum(len(o) for o in out) == 4
    for k, d in aligned.items():
        got = np.load(os.path.join(pre, "duration", f"{UTTS[k][0]}-duration-{k}.npy"))
        assert got.dtype == np.int64 and got.tolist() == d
    # a second run has nothing to do
    (written, left), = ALIGN.main(["--config", cfg_dir, "--corpus", "toy", "--steps", "5"])
    assert written == [] and len(left) == 4
