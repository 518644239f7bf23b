"""Optional positions of the aligner on the GPU: ``fs2_forward_sum_opt`` and ``fs2_mas_opt``
(``K.forward_sum`` / ``K.mas`` with ``optional=``) against ``align_sil_oracle``, one training step
against the model in plain torch, convergence on the oracle's corpus with pauses, and
``align.main --optional_sil sp`` end to end into ``Preprocessor.build_from_path``.

Tolerances as tests/test_gpu_align.py: ``close()`` (max abs error <= 1e-4 x the oracle's largest
magnitude, the oracle in fp64 from the same fp32 inputs) for the loss and its gradient,
``torch.equal`` for the durations (one IEEE fp32 add per cell, compares otherwise).

Convergence.  ``align_sil_oracle.oracle_run`` (the torch model on the CPU, 100 Adam steps of
batches of 8, temperature 0.05, the prior off, on ``synth_corpus_sil``) gave on seeds 0..4 a frame
agreement of 0.921, 0.933, 0.826, 0.807, 0.831 (mean 0.864, sample standard deviation 0.059, the
spread; untrained 0.095, 0.081, 0.093, 0.124, 0.106) and a pause accuracy of 0.958, 0.940, 0.899,
0.897, 0.950 (mean 0.929, sample standard deviation 0.029).  The test trains seed 1 from the
oracle's initial weights over the oracle's batches and asks for the oracle's agreement and pause
accuracy minus twice their spreads (trajectories differ by reduction order, not by more than
seeds do).  tests/test_align_sil_cpu.py holds the premise: what the same model reaches without
positions for the pauses, and what the prior does to them.
"""
import copy
import importlib
import os
import wave

import numpy as np
import pytest
import torch

import align_oracle as O
import align_sil_oracle as S
import pitch_oracle as PO

NAME = "mid-attribute-speaker-generation_amd"
PKG = importlib.import_module(NAME)
K = importlib.import_module(NAME + ".kernels")
AL = importlib.import_module(NAME + ".aligner")
pytestmark = pytest.mark.gpu
DEV = "cuda"

LENS = [(1, 1), (1, 9), (7, 7), (7, 8), (64, 200), (65, 200), (130, 300), (258, 300)]  # (N, M)
MASKS = ["alternate", "random", "first", "last", "chunk-edge"]
B, A, TEMP = 3, 40, 0.05
SPREAD, PAUSE_SPREAD = 0.059, 0.029


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
    """``test_gpu_align._batch``: a ragged batch of three whose longest row is (N, M)."""
    lens = [(N, M), (max(1, N // 2), max(1, N // 2, M - 3)), (max(1, N - 1), M)]
    return lens, max(n for n, _ in lens) + 3, max(m for _, m in lens) + 5


def mask_of(kind, n, rng):
    """One row's marks; never two neighbours, never all (a row of one position has none)."""
    m = np.zeros(n, np.uint8)
    if n == 1:
        return m
    if kind == "alternate":  # every other position from 0, and both ends
        m[0::2] = 1
        if n % 2 == 0:
            m[n - 2], m[n - 1] = 0, 1
    elif kind == "random":
        m[:] = rng.random(n) < 0.3
        for s in range(1, n):
            if m[s] and m[s - 1]:
                m[s] = 0
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[n - 1] = 1
    else:  # where the s - 2 reads cross a thread's chunk of 256 states (and a wave's 64)
        for s in (63, 65, 127, 129, 255, 257):
            if s < n:
                m[s] = 1
    return m


def rows_logp(lens, T_m, T_s, rng):
    """The oracle's log-probabilities (prior on) of random q, k, rounded to fp32."""
    out = np.zeros((len(lens), T_m, T_s), np.float32)
    for b, (n, m) in enumerate(lens):
        q = torch.from_numpy(rng.standard_normal((T_m, A)).astype(np.float32))
        k = torch.from_numpy(rng.standard_normal((T_s, A)).astype(np.float32))
        out[b] = O.logprob(q, k, n, m, TEMP, 1.0).numpy().astype(np.float32)
    return out


def reference(logp32, lens, masks, w):
    """nll, weighted gradient and durations of every row by the oracle."""
    nll, grad = [], np.zeros(logp32.shape)
    dur = np.zeros(logp32.shape[::2], np.int64)
    for b, (n, m) in enumerate(lens):
        v, g = S.forward_sum_opt(logp32[b], n, m, masks[b])
        nll.append(v)
        grad[b, :m, :n] = g * float(w[b])
        dur[b, :n] = S.mas_opt(logp32[b], n, m, masks[b])
    return np.asarray(nll), grad, dur


_LOGP, _CASES = {}, {}


def case(N, M, kind):
    """Inputs and oracle results of one (N, M, mask kind), computed once and shared."""
    if (N, M, kind) in _CASES:
        return _CASES[(N, M, kind)]
    lens, T_s, T_m = _batch(N, M)
    if (N, M) not in _LOGP:
        rng = np.random.default_rng(100 * N + M)
        _LOGP[(N, M)] = (rows_logp(lens, T_m, T_s, rng), rng.uniform(0.01, 0.1, B).astype(np.float32))
    logp32, w = _LOGP[(N, M)]
    rng = np.random.default_rng(7 * N + M + len(kind))
    masks = np.zeros((B, T_s), np.uint8)
    for b, (n, _) in enumerate(lens):
        masks[b, :n] = mask_of(kind, n, rng)
    for b, (n, _) in enumerate(lens):
        masks[b, n:] = rng.random(T_s - n) < 0.5  # past a row's N: never read
    c = {"lens": lens, "T_s": T_s, "T_m": T_m, "logp32": logp32, "w": w, "mask": masks,
         "src": np.asarray([n for n, _ in lens], np.int64),
         "mel": np.asarray([m for _, m in lens], np.int64)}
    c["nll"], c["grad"], c["dur"] = reference(logp32, lens, masks, w)
    _CASES[(N, M, kind)] = c
    return c


def _dead(x, lens):
    x = x.cpu().numpy()
    return all(not x[b, m:].any() and not x[b, :, n:].any() for b, (n, m) in enumerate(lens))


def _host(c):
    return (c["src"], c["mel"], c["mask"])


# ------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("N,M", LENS)
@pytest.mark.parametrize("kind", MASKS)
def test_forward_sum_opt(N, M, kind):
    c = case(N, M, kind)
    logp, src, mel, w, mask = (_dev(c[x]) for x in ("logp32", "src", "mel", "w", "mask"))
    nll, grad = K.forward_sum(logp, src, mel, w, _host(c), optional=mask)
    close(nll, c["nll"], what=f"nll {N}x{M} {kind}")
    close(grad, c["grad"], what=f"grad {N}x{M} {kind}")
    assert _dead(grad, c["lens"]) and bool(torch.isfinite(grad).all())
    for b in range(B):
        n1, g1 = K.forward_sum(logp[b:b + 1], src[b:b + 1], mel[b:b + 1], w[b:b + 1],
                               optional=mask[b:b + 1].contiguous())
        assert torch.equal(n1[0], nll[b]) and torch.equal(g1[0], grad[b])
    again = K.forward_sum(logp, src, mel, w, optional=mask)
    assert torch.equal(again[0], nll) and torch.equal(again[1], grad)  # run to run


@pytest.mark.parametrize("N,M", LENS)
@pytest.mark.parametrize("kind", MASKS)
def test_mas_opt(N, M, kind):
    c = case(N, M, kind)
    logp, src, mel, mask = (_dev(c[x]) for x in ("logp32", "src", "mel", "mask"))
    dur = K.mas(logp, src, mel, _host(c), optional=mask)
    assert dur.dtype == torch.int64 and torch.equal(dur.cpu(), torch.from_numpy(c["dur"]))
    for b, (n, m) in enumerate(c["lens"]):
        d, o = dur[b, :n].cpu().numpy(), c["mask"][b, :n]
        assert d.sum() == m and (d[o == 0] >= 1).all() and not dur[b, n:].any()
    for b in range(B):
        one = K.mas(logp[b:b + 1], src[b:b + 1], mel[b:b + 1], optional=mask[b:b + 1].contiguous())
        assert torch.equal(one[0], dur[b])
    assert torch.equal(K.mas(logp, src, mel, optional=mask), dur)


def test_at_the_limits():
    """One row of T_s = 1024, T_m = 2048, marks on every other position and both ends."""
    N, M = K.ALIGN_MAX_SRC, K.ALIGN_MAX_MEL
    rng = np.random.default_rng(9)
    z = (rng.standard_normal((1, M, N)) * 3.0).astype(np.float32)
    logp32 = torch.log_softmax(torch.from_numpy(z).double(), 2).float().numpy()
    mask = mask_of("alternate", N, rng)[None]
    w = np.float32([1.0 / M])
    nll, grad, dur = reference(logp32, [(N, M)], mask, w)
    src, mel = np.asarray([N], np.int64), np.asarray([M], np.int64)
    got = K.forward_sum(_dev(logp32), _dev(src), _dev(mel), _dev(w), (src, mel, mask),
                        optional=_dev(mask))
    close(got[0], nll, what="nll at the limits")
    close(got[1], grad, what="grad at the limits")
    d = K.mas(_dev(logp32), _dev(src), _dev(mel), (src, mel, mask), optional=_dev(mask))
    assert torch.equal(d.cpu(), torch.from_numpy(dur)) and int(d.sum()) == M


def test_fewer_frames_than_positions():
    """M below N but at or above the unmarked count: the path has to omit."""
    lens = [(7, 5), (7, 4), (258, 200), (9, 5)]
    T_s, T_m = 260, 203
    rng = np.random.default_rng(31)
    logp32 = rows_logp(lens, T_m, T_s, rng)
    masks = np.zeros((4, T_s), np.uint8)
    for b, (n, _) in enumerate(lens):
        masks[b, :n] = mask_of("alternate", n, rng)
    w = rng.uniform(0.01, 0.1, 4).astype(np.float32)
    nll, grad, dur = reference(logp32, lens, masks, w)
    assert np.isfinite(nll).all()
    src, mel = (np.asarray(x, np.int64) for x in zip(*lens))
    got = K.forward_sum(_dev(logp32), _dev(src), _dev(mel), _dev(w), (src, mel, masks),
                        optional=_dev(masks))
    close(got[0], nll, what="nll, M < N")
    close(got[1], grad, what="grad, M < N")
    assert _dead(got[1], lens)
    d = K.mas(_dev(logp32), _dev(src), _dev(mel), (src, mel, masks), optional=_dev(masks))
    assert torch.equal(d.cpu(), torch.from_numpy(dur))
    assert d.sum(1).cpu().tolist() == [m for _, m in lens]


def test_mas_opt_tie_rules():
    """Small integers: sums are exact, so equal-score paths tie exactly (tests/test_align_sil_cpu.py
    checks the oracle's choice among them against enumeration)."""
    rng = np.random.default_rng(7)
    lens = [(5, 9), (7, 8), (70, 140), (7, 5), (260, 300)]
    T_s, T_m = 262, 303
    x = rng.integers(-1, 1, (5, T_m, T_s)).astype(np.float32)
    x[1] = 0.0  # every path ties
    x[3] = 0.0
    masks = np.zeros((5, T_s), np.uint8)
    for b, (n, _) in enumerate(lens):
        masks[b, :n] = mask_of("alternate" if b != 2 else "random", n, rng)
    want = np.zeros((5, T_s), np.int64)
    for b, (n, m) in enumerate(lens):
        want[b, :n] = S.mas_opt(x[b], n, m, masks[b])
    src, mel = (np.asarray(v, np.int64) for v in zip(*lens))
    dur = K.mas(_dev(x), _dev(src), _dev(mel), optional=_dev(masks))
    assert torch.equal(dur.cpu(), torch.from_numpy(want))
    assert want[1, :7].tolist() == [2, 1, 1, 1, 1, 1, 1]  # all ties: nothing is omitted


@pytest.mark.parametrize("N,M", LENS + [(7, 5)])
def test_a_zero_mask_has_the_bits_of_the_plain_entries(N, M):
    lens, T_s, T_m = _batch(N, max(M, 1))
    rng = np.random.default_rng(100 * N + M)
    if M < N:
        lens = [(N, M), (3, 2), (2, 6)]  # rows without a path too
    logp = _dev(rows_logp([(n, max(m, n)) for n, m in lens], T_m, T_s, rng))
    src, mel = (_dev(np.asarray(v, np.int64)) for v in zip(*lens))
    w = _dev(rng.uniform(0.01, 0.1, B).astype(np.float32))
    zero = torch.zeros((B, T_s), dtype=torch.uint8, device=DEV)
    nll, grad = K.forward_sum(logp, src, mel, w)
    nll0, grad0 = K.forward_sum(logp, src, mel, w, optional=zero)
    assert torch.equal(nll0, nll) and torch.equal(grad0, grad)
    assert torch.equal(K.mas(logp, src, mel, optional=zero), K.mas(logp, src, mel))


def test_rows_without_a_path():
    """Fewer frames than unmarked positions: the wrappers raise where the lengths and the mask
    are on the host; on the device the row's nll is +inf, its gradient and durations 0 (never
    NaN), and the other rows stand."""
    c = case(7, 8, "alternate")
    logp, w, mask = _dev(c["logp32"]), _dev(c["w"]), _dev(c["mask"])
    src, mel = c["src"].copy(), c["mel"].copy()
    mel[0] = (src[0] - int(c["mask"][0, :src[0]].sum())) - 1
    host = (src, mel, c["mask"])
    for call in (lambda: K.mas(logp, _dev(src), _dev(mel), host, optional=mask),
                 lambda: K.forward_sum(logp, _dev(src), _dev(mel), w, host, optional=mask)):
        with pytest.raises(RuntimeError, match="no monotonic path"):
            call()
    nll, grad = K.forward_sum(logp, _dev(src), _dev(mel), w, optional=mask)
    dur = K.mas(logp, _dev(src), _dev(mel), optional=mask)
    assert bool(torch.isinf(nll[0])) and float(nll[0]) > 0
    assert not grad[0].any() and not dur[0].any() and bool(torch.isfinite(grad).all())
    close(nll[1:], c["nll"][1:], what="nll of the other rows")
    close(grad[1:], c["grad"][1:], what="grad of the other rows")
    assert torch.equal(dur[1:].cpu(), torch.from_numpy(c["dur"][1:]))


def test_invalid_masks_raise():
    c = case(7, 8, "first")
    logp, src, mel, w = (_dev(c[x]) for x in ("logp32", "src", "mel", "w"))
    for bad in ([0, 1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 1, 1, 0]):
        m = c["mask"].copy()
        m[0, :7] = bad
        for call in (lambda: K.forward_sum(logp, src, mel, w, (c["src"], c["mel"], m),
                                           optional=_dev(m)),
                     lambda: K.mas(logp, src, mel, (c["src"], c["mel"], m), optional=_dev(m))):
            with pytest.raises(ValueError, match="adjacent"):
                call()
    m = c["mask"].copy()
    m[1, :3] = [1, 0, 1]
    m[1, 1] = 1
    with pytest.raises(ValueError):
        K.mas(logp, src, mel, (c["src"], c["mel"], m), optional=_dev(m))
    one = np.ones((1, 1), np.uint8)  # a single position that is optional: none is left
    n1 = np.asarray([1], np.int64)
    with pytest.raises(ValueError, match="not optional"):
        K.mas(logp[:1, :, :1].contiguous(), _dev(n1), _dev(n1), (n1, n1, one), optional=_dev(one))
    with pytest.raises(RuntimeError, match="uint8"):
        K.mas(logp, src, mel, optional=_dev(c["mask"].astype(np.int64)))


# ------------------------------------------------------------------ the model
def _pair(ref):
    model = AL.Aligner(S.N_SYMBOLS + 2, S.N_MELS, O.CHANNELS, O.ATTN_DIM, DEV)
    model.load_state_dict(ref.state_dict())
    return model


def test_one_training_step_with_the_mask_against_torch():
    corpus = S.synth_corpus_sil(0)
    ref = O.TorchAligner(S.N_SYMBOLS + 2, S.N_MELS, O.CHANNELS, O.ATTN_DIM)
    PKG.seeded.load_seeded_(ref)
    with torch.no_grad():
        ref.embedding.weight[0].zero_()  # padding_idx
    model = _pair(ref)
    ref = ref.double()
    idx = np.asarray([0, 3, 5, 9, 17])
    texts, src_lens, mels, mel_lens, optional = S.take(corpus, idx)
    want = S.loss(ref, texts, src_lens, mels.double(), mel_lens, optional, S.TEMPERATURE, S.OMEGA)
    want.backward()
    tr = AL.AlignerTrainer(model, O.LR, S.TEMPERATURE, S.OMEGA)
    args = (texts.to(DEV), src_lens.to(DEV), mels.to(DEV), mel_lens.to(DEV))
    host = (src_lens.numpy(), mel_lens.numpy(), optional.numpy())
    loss = tr.backward(*args, host, optional.to(DEV))
    close(loss, want, what="loss")
    got = dict(model.named_parameters())
    for name, p in ref.named_parameters():
        close(got[name].grad, p.grad, what=name)
    again = tr.train_step(*args, optional=optional.to(DEV))
    assert torch.equal(again, loss) and tr.step == 1
    plain = tr.backward(*args)  # no mask: another loss
    assert not torch.equal(plain, loss)


@pytest.fixture(scope="module")
def oracle_run():
    return S.oracle_run(S.SEED, unmasked=False)


def test_convergence_on_the_corpus_with_pauses(oracle_run):
    r = oracle_run
    assert r["trained"] >= 0.85 and r["untrained"] <= 0.20 and r["pause"] >= 0.85  # the inputs
    corpus = S.synth_corpus_sil(S.SEED)
    ref = S.new_model(S.SEED)
    ref.load_state_dict(r["init"])
    model = _pair(ref)
    tr = AL.AlignerTrainer(model, O.LR, S.TEMPERATURE, S.OMEGA)
    dev = {k: _dev(v) for k, v in corpus.items()}

    def take(idx):
        sl, ml = corpus["src_lens"][idx], corpus["mel_lens"][idx]
        i = _dev(idx)
        return (dev["texts"][i][:, :sl.max()].contiguous(), dev["src_lens"][i],
                dev["mels"][i][:, :ml.max()].contiguous(), dev["mel_lens"][i],
                dev["optional"][i][:, :sl.max()].contiguous())

    losses = tr.fit([take(idx) for idx in O.batch_order(S.SEED, S.STEPS)], S.STEPS)
    assert len(losses) == S.STEPS and tr.step == S.STEPS
    batch = take(np.arange(S.N_UTT))
    dur = tr.align(*batch[:4], optional=batch[4]).cpu().numpy()
    got, pause = S.agreement(dur, corpus), S.pause_accuracy(dur, corpus)
    print(f"agreement {got:.3f}, oracle {r['trained']:.3f} (untrained {r['untrained']:.3f}); "
          f"pause accuracy {pause:.3f}, oracle {r['pause']:.3f}; loss {float(losses[0]):.4f} -> "
          f"{float(losses[-1]):.4f}")
    assert float(losses[-1]) < float(losses[0])
    assert got >= r["trained"] - 2 * SPREAD
    assert pause >= r["pause"] - 2 * PAUSE_SPREAD


# ------------------------------------------------------------------ end to end
# speaker, rate, (leading silence, voiced, gap, voiced, trailing silence) seconds, glide, .phn
UTTS = {"a0": ("spkA", 24000, (0.10, 0.25, 0.12, 0.25, 0.08), (120.0, 150.0), "a k | o i"),
        "a1": ("spkA", 48000, (0.08, 0.30, 0.10, 0.20, 0.10), (200.0, 170.0), "{k a | i o}"),
        "b0": ("spkB", 22050, (0.06, 0.20, 0.10, 0.20, 0.06), (230.0, 190.0), "o k | i a"),
        "b1": ("spkB", 24000, (0.10, 0.30, 0.15, 0.25, 0.12), (160.0, 210.0), "i k a | k o sp i a")}


def _write_wav(path, x, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(sr)
        w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())


def test_align_main_with_optional_silences_then_build_from_path(tmp_path, capsys):
    import yaml
    PRE, ALIGN, IO = (importlib.import_module(f"{NAME}.{m}") for m in ("preprocess", "align",
                                                                      "corpus_io"))
    raw, pre, cfg_dir = (str(tmp_path / d) for d in ("raw", "pre", "config"))
    os.makedirs(cfg_dir)
    samples = {}
    for k, (speaker, sr, parts, glide, phn) in UTTS.items():
        os.makedirs(os.path.join(raw, speaker), exist_ok=True)
        n = [int(round(p * sr)) for p in parts]
        x = PO.voice(sum(n), glide[0] * PO.SR / sr, glide[1] * PO.SR / sr, seed=len(k) + sum(n))
        x = np.asarray(x, np.float64).copy()
        x[:n[0]] = 0.0  # zero-padded edges and one inner gap
        x[n[0] + n[1]:n[0] + n[1] + n[2]] = 0.0
        x[sum(n) - n[4]:] = 0.0
        samples[k] = sum(n)
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
    common = ["--config", cfg_dir, "--corpus", "toy", "--steps", "5", "--batch", "2", "--seed", "4"]
    with pytest.raises(ValueError, match=r"unknown symbol '\|'"):  # without the flag, as before
        ALIGN.main(common)
    assert not os.path.exists(os.path.join(pre, "TextGrid"))
    capsys.readouterr()
    (written, left), = ALIGN.main(common + ["--optional_sil", "sp"])
    out = capsys.readouterr().out
    places = 0
    aligned, rs = {}, importlib.import_module(NAME + ".audio").Resampler(22050, DEV)
    assert len(written) == 4 and left == []
    kept_total = 0
    for p in written:
        k = os.path.basename(p).split(".")[0]
        phones, _, optional = ALIGN.parse_phn(
            os.path.join(raw, UTTS[k][0], f"{k}.phn"), None, "sp", True)
        places += sum(optional)
        tier = IO.read_textgrid(p)["phones"]
        assert all(e > s for s, e, _ in tier)  # no zero-length interval
        # the phones are the kept positions: all mandatory ones, in order, and some optional
        texts, it = [t for _, _, t in tier], iter(zip(phones, optional))
        for t in texts:
            for ph, o in it:
                if ph == t:
                    kept_total += o
                    break
                assert o, (k, texts, phones)  # only an optional position may be missing
            else:
                pytest.fail(f"{k}: {texts} is no subsequence of {phones}")
        assert all(o for _, o in it)
        frames = [int(np.round(e * 22050 / 256) - np.round(s * 22050 / 256)) for s, e, _ in tier]
        assert min(frames) >= 1
        assert sum(frames) == rs.out_len(samples[k], UTTS[k][1]) // 256
        got_p, got_d, start, end = PRE.durations_from_intervals(tier, 22050, 256)
        lead = frames[0] if texts[0] == "sp" else 0
        trail = frames[-1] if texts[-1] == "sp" else 0
        # the edge silences are trimmed, inner ones stay; the durations fill the trimmed waveform
        assert got_p == texts[bool(lead):len(texts) - bool(trail)]
        assert sum(got_d) == sum(frames) - lead - trail
        assert int(22050 * end) - int(22050 * start) == sum(got_d) * 256
        aligned[k] = got_d
    assert f"wrote 4 TextGrids, left 0; pauses kept {kept_total} of {places}" in out
    built = PRE.Preprocessor(config, batch=4, seed=3).build_from_path()
    assert sum(len(o) for o in built) == 4
    for k, d in aligned.items():
        got = np.load(os.path.join(pre, "duration", f"{UTTS[k][0]}-duration-{k}.npy"))
        assert got.dtype == np.int64 and got.tolist() == d
