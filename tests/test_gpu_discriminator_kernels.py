"""The discriminator's kernels (``csrc/lstm.hip``) through the C ABI against ``lstm_oracle``,
a float64 restatement on the CPU: the LSTM wavefront and the single-layer recurrence (every
layer's h, c, activated gates and gate gradients, and dx), the head with and without
dropout, the BCE rows, the 150-frame re-padding and the label repeat.

Every output buffer is NaN before the call, so an element the kernel skips shows.  Bars are
the project's fp32 bars, here against float64: h, act and emb within 2e-5 absolute
(``test_clf.py``), logits rtol 1e-4 / atol 1e-5 (``test_clf.py``), every other tensor within
1e-4 of the reference tensor's max-abs (``_close`` in ``test_embedder_train.py``)."""
import importlib

import numpy as np
import pytest
import torch

import lstm_oracle as lo

pytestmark = pytest.mark.gpu
K = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
G = importlib.import_module("mid-attribute-speaker-generation_amd.ge2e")
_L = importlib.import_module("mid-attribute-speaker-generation_amd._lib")
lib, KernelError = _L.lib, _L.KernelError
DEV, D = "cuda", 80
P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
ABS_BAR, REL_BAR = 2e-5, 1e-4


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def host(t):
    return t.detach().cpu().double().numpy()


def check_abs(got, want, tag, bar=ABS_BAR):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: unwritten or non-finite elements"
    err = np.abs(got - want).max()
    print(f"{tag}: abs err {err:.3e} (bar {bar:.1e})")
    assert err <= bar, (tag, err)
    return err


def check_peak(got, want, tag, bar=REL_BAR):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: unwritten or non-finite elements"
    err, peak = np.abs(got - want).max(), np.abs(want).max()
    print(f"{tag}: err / peak {err / peak if peak else err:.3e} (bar {bar:.1e}), peak {peak:.3e}")
    assert err <= bar * peak, (tag, err, peak)
    return err


# ------------------------------------------------------------------ the LSTM recurrences
def _lstm_inputs(N, T, H, L, mode):
    gen = torch.Generator().manual_seed(1000 * N + 10 * T + L + H)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.1  # noqa: E731
    w = {"w_ih0": mk(4 * H, D), "w_ih_up": mk(L - 1, 4 * H, H) if L > 1 else None,
         "w_hh": mk(L, 4 * H, H), "bias": mk(L, 4 * H)}
    x = torch.randn(N, T, D, generator=gen)
    dh = mk(N, T, H)
    if mode == "last":  # what _EmbedderFn.backward passes: only the last frame is read
        dh[:, :-1] = 0
    elif mode == "null":
        dh = None
    return w, x, dh


def _oracle(w, x, dh):
    up = None if w["w_ih_up"] is None else w["w_ih_up"].numpy()
    return lo.lstm_stack(x.numpy(), (w["w_ih0"].numpy(), up), w["w_hh"].numpy(),
                         w["bias"].numpy(), None if dh is None else dh.numpy())


def _run_stack(N, T, H, L, w, x, dh):
    rows = N * T
    dev = {k: None if v is None else v.to(DEV) for k, v in w.items()}
    tr = lambda t: None if t is None else t.transpose(-1, -2).contiguous()  # noqa: E731
    xd, dhd = x.to(DEV), None if dh is None else dh.to(DEV)
    out = {"gx": nan(rows, 4 * H), "h": nan(L, rows, H), "c": nan(L, rows, H),
           "act": nan(L, rows, 4 * H), "dgates": nan(L, rows, 4 * H), "dx": nan(rows, D)}
    dc = nan(L * 2 * N * H)
    lib.fs2_lstm_stack_fwd(P(xd), N, T, D, H, L, P(dev["w_ih0"]), P(dev["w_ih_up"]),
                           P(dev["w_hh"]), P(dev["bias"]), P(out["gx"]), P(out["h"]), P(out["c"]),
                           P(out["act"]), K.stream())
    w_ih0_t, w_ih_up_t, w_hh_t = tr(dev["w_ih0"]), tr(dev["w_ih_up"]), tr(dev["w_hh"])
    lib.fs2_lstm_stack_bwd(P(dhd), N, T, D, H, L, P(w_ih0_t), P(w_ih_up_t), P(w_hh_t),
                           P(out["act"]), P(out["c"]), P(out["dgates"]), P(dc), P(out["dx"]),
                           K.stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _run_layer(N, T, H, w, x, dh):
    rows = N * T
    xd, dhd = x.to(DEV), dh.to(DEV)
    w_ih, w_hh, bias = w["w_ih0"].to(DEV), w["w_hh"][0].to(DEV).contiguous(), w["bias"][0].to(DEV)
    out = {"gx": nan(rows, 4 * H), "h": nan(1, rows, H), "c": nan(1, rows, H),
           "act": nan(1, rows, 4 * H), "dgates": nan(1, rows, 4 * H), "dx": nan(rows, D)}
    dc = nan(2 * N * H)
    lib.fs2_lstm_layer_fwd(P(xd), N, T, D, H, P(w_ih), P(bias), P(w_hh), P(out["gx"]),
                           P(out["h"]), P(out["c"]), P(out["act"]), K.stream())
    w_ih_t, w_hh_t = w_ih.t().contiguous(), w_hh.t().contiguous()
    lib.fs2_lstm_layer_bwd(P(dhd), N, T, D, H, P(w_ih_t), P(w_hh_t), P(out["act"]), P(out["c"]),
                           P(out["dgates"]), P(dc), P(out["dx"]), K.stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


_LSTM = {}


def _lstm(kind, N, T, H, L, mode):
    """Two runs through the C ABI and the float64 oracle, once per case."""
    key = (kind, N, T, H, L, mode)
    if key not in _LSTM:
        w, x, dh = _lstm_inputs(N, T, H, L, mode)
        run = (lambda: _run_stack(N, T, H, L, w, x, dh)) if kind == "stack" else \
            (lambda: _run_layer(N, T, H, w, x, dh))
        _LSTM[key] = (run(), run(), _oracle(w, x, dh))
    return _LSTM[key]


def _compare_lstm(first, ref, N, T, H, L, tag):
    for l in range(L):
        shp = lambda a: host(a[l]).reshape(N, T, -1)  # noqa: E731
        check_abs(shp(first["h"]), ref["h"][l], f"{tag} h[{l}]")
        check_abs(shp(first["act"]), ref["act"][l], f"{tag} act[{l}]")
        check_peak(shp(first["c"]), ref["c"][l], f"{tag} c[{l}]")
        check_peak(shp(first["dgates"]), ref["dgates"][l], f"{tag} dgates[{l}]")
    check_peak(host(first["dx"]).reshape(N, T, D), ref["dx"], f"{tag} dx")
    assert torch.isfinite(first["gx"]).all()


# N, T, H, L, top gradient.  33/2: T < L (two layers out of range in one launch) and a second
# forward block row of one sequence; 32/3: full 32-sequence tiles, T = L; 16/5: the second
# 16-sequence B tile wholly invalid beside a full first one; 70/17: three forward and five
# backward block rows, ragged; 34/60: a long recurrence across block rows; L = 1 (w_ih_up =
# NULL), L = 2; H = 512: every split-K loop takes more trips.
STACK_CASES = [(33, 2, 256, 3, "full"), (32, 3, 256, 3, "full"), (16, 5, 256, 3, "full"),
               (70, 17, 256, 3, "full"), (70, 17, 256, 3, "last"), (34, 60, 256, 3, "full"),
               (17, 4, 256, 1, "full"), (17, 4, 256, 2, "full"), (17, 4, 256, 2, "null"),
               (5, 9, 512, 3, "full")]


@pytest.mark.parametrize("N,T,H,L,mode", STACK_CASES)
def test_lstm_stack_matches_float64_oracle(N, T, H, L, mode):
    first, _, ref = _lstm("stack", N, T, H, L, mode)
    if mode == "null":  # no top gradient: nothing to back-propagate, exactly
        assert not ref["dgates"].any() and not ref["dx"].any()
        assert (first["dgates"] == 0).all() and (first["dx"] == 0).all()
        print(f"stack {(N, T, H, L)} dh_out = NULL: dgates and dx exactly 0")
    if mode == "last":
        assert np.abs(ref["dgates"][0][:, 0]).max() > 0  # the gradient reaches the first frame
    _compare_lstm(first, ref, N, T, H, L, f"stack {(N, T, H, L)} {mode}")


@pytest.mark.parametrize("N,T,H,L,mode", STACK_CASES)
def test_lstm_stack_is_repeatable(N, T, H, L, mode):
    first, second, _ = _lstm("stack", N, T, H, L, mode)
    for k in first:  # NaN != NaN: an unwritten element fails here as well
        assert torch.equal(first[k], second[k]), k


LAYER_CASES = [(1, 1, 256), (16, 2, 256), (49, 5, 256), (3, 4, 512)]


@pytest.mark.parametrize("N,T,H", LAYER_CASES)
def test_lstm_layer_matches_float64_oracle(N, T, H):
    first, second, ref = _lstm("layer", N, T, H, 1, "full")
    _compare_lstm(first, ref, N, T, H, 1, f"layer {(N, T, H)}")
    for k in first:
        assert torch.equal(first[k], second[k]), k


# ------------------------------------------------------------------ the head
HID, PROJ, FRAMES, LDDX = 256, 64, 3, 256 + 16
# A ReLU whose pre-activation is within fp32 rounding of 0 may be decided differently in fp32
# and in float64, and the gradient jumps there.  fp32 rounding of a 64-term dot product of
# these magnitudes is about 2e-7; the inputs (fixed seeds, chosen on the CPU from the oracle
# alone) keep every pre-activation ten times further from 0, asserted before any comparison.
RELU_MARGIN = 2e-6
HEAD_SEEDS = {1: 0, 4: 0, 5: 0, 37: 0, 203: 4}  # n -> seed; margins 1e-4 .. 8e-3 without masks


def _head_inputs(n, seed):
    gen = torch.Generator().manual_seed(4000 + 10 * n + seed)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.2  # noqa: E731
    w = {"wp": mk(PROJ, HID), "bp": mk(PROJ), "w0": mk(PROJ, PROJ), "b0": mk(PROJ),
         "w1": mk(PROJ, PROJ), "b1": mk(PROJ), "w2": mk(1, PROJ), "b2": mk(1)}
    xbuf = torch.randn(n, FRAMES, HID, generator=gen)  # the head reads the last frame
    demb = torch.randn(n, PROJ, generator=gen)
    dlogit = torch.randn(n, generator=gen)
    return w, xbuf, demb, dlogit


def relu_margin(ref, m0=None, m1=None):
    """The smallest |pre-activation| among the units dropout keeps."""
    z = [np.abs(ref["z0"]), np.abs(ref["z1"])]
    for a, m in zip(z, (m0, m1)):
        if m is not None:
            a[m == 0] = np.inf
    return min(a.min() for a in z)


def _head_operands(w):
    d = {k: v.to(DEV).contiguous() for k, v in w.items()}
    t = lambda k: d[k].t().contiguous()  # noqa: E731
    keep = (d["wp"], t("wp"), d["bp"], d["w0"], t("w0"), d["b0"], d["w1"], t("w1"), d["b1"],
            d["w2"], d["b2"])
    return keep


def _run_head(n, keep, xbuf, p, seed, site, want_out, demb, dlogit, backward):
    """One fs2_clf_head call on the last frame of xbuf (n, FRAMES, HID): row stride
    FRAMES * HID in, LDDX out.  Returns emb, logit, dx (None where not asked for)."""
    emb = nan(n, PROJ) if want_out else None
    logit = nan(n) if want_out else None
    dx = nan(n, LDDX) if backward else None
    last = P(xbuf) + (FRAMES - 1) * HID * 4
    lib.fs2_clf_head(last, FRAMES * HID, n, *[P(t) for t in keep], p, P(seed), site, P(emb),
                     P(logit), P(demb), P(dlogit), P(dx), LDDX, K.stream())
    torch.cuda.synchronize()
    if dx is not None:  # the row padding is not the kernel's to write
        assert torch.isnan(dx[:, HID:]).all()
        dx = dx[:, :HID]
    return emb, logit, dx


def _check_head(got, ref, tag):
    emb, logit, dx = got
    if emb is not None:
        check_abs(host(emb), ref["emb"], f"{tag} emb")
        lg, want = host(logit), ref["logit"]
        assert np.isfinite(lg).all()
        err = np.abs(lg - want)
        print(f"{tag} logit: abs err {err.max():.3e} (bar 1e-5 + 1e-4 |want|, |want| up to "
              f"{np.abs(want).max():.3e})")
        assert (err <= 1e-5 + 1e-4 * np.abs(want)).all(), (tag, err.max())
    if dx is not None:
        check_peak(host(dx), ref["dx"], f"{tag} dx")


_HEAD = {}


def _head_ref(n, mode):
    if (n, mode) not in _HEAD:
        w, xbuf, demb, dlogit = _head_inputs(n, HEAD_SEEDS[n])
        ones = np.ones((n, PROJ))
        de = demb.numpy() if mode in ("demb", "both") else None
        dl = dlogit.numpy() if mode in ("dlogit", "both") else None
        _HEAD[(n, mode)] = lo.clf_head(xbuf[:, -1].numpy(), {k: v.numpy() for k, v in w.items()},
                                       ones, ones, de, dl)
    return _HEAD[(n, mode)]


@pytest.mark.parametrize("mode", ["forward", "demb", "dlogit", "both"])
@pytest.mark.parametrize("n", [1, 4, 5, 37])
def test_clf_head_matches_float64_oracle(n, mode):
    w, xbuf, demb, dlogit = _head_inputs(n, HEAD_SEEDS[n])
    ref = _head_ref(n, mode)
    margin = relu_margin(ref)
    print(f"n = {n}: smallest |pre-activation| {margin:.3e} (needs {RELU_MARGIN:.0e})")
    assert margin >= RELU_MARGIN
    keep, xd = _head_operands(w), xbuf.to(DEV)
    de = demb.to(DEV) if mode in ("demb", "both") else None
    dl = dlogit.to(DEV) if mode in ("dlogit", "both") else None
    # the wrapper's forward asks for emb and logit alone, its backward for dx alone
    got = _run_head(n, keep, xd, 0.0, None, 7, mode in ("forward", "both"), de, dl,
                    mode != "forward")
    assert (got[2] is None) == (mode == "forward")
    _check_head(got, ref, f"head n = {n} {mode}")
    again = _run_head(n, keep, xd, 0.0, None, 7, mode in ("forward", "both"), de, dl,
                      mode != "forward")
    for a, b in zip(got, again):
        assert a is None or torch.equal(a, b)


# ---- dropout: the masks are a function of (seed, site, row, layer, unit) alone, so probe
# weights read them out of the kernel itself and real weights are then held to the oracle
N_DROP, P_DROP = 203, 0.2
KEEP = float(np.float32(1) / (np.float32(1) - np.float32(P_DROP)))  # the kernel's 1 / (1 - p)


def _probe_masks(seed, site, xd, wp, bp):
    """m0, m1 (N_DROP, 64) as the kernel draws them at (seed, site), 128 launches."""
    n = N_DROP
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    o = lambda *s: torch.ones(*s, device=DEV)  # noqa: E731
    wpt = wp.t().contiguous()

    def logits(w0, b0, w1, b1, w2):
        keep = (wp, wpt, bp, w0, w0.t().contiguous(), b0, w1, w1.t().contiguous(), b1, w2, z(1))
        got = _run_head(n, keep, xd, P_DROP, seed, site, True, None, None, False)
        assert torch.isfinite(got[0]).all()
        return host(got[1])

    m1 = np.empty((n, PROJ))
    for j in range(PROJ):  # a0 = 0, a1 = m1, logit = m1[:, j]
        w2 = z(1, PROJ)
        w2[0, j] = 1
        m1[:, j] = logits(z(PROJ, PROJ), z(PROJ), z(PROJ, PROJ), o(PROJ), w2)
    rowsum = m1.sum(axis=1)
    assert (rowsum > 0).all()
    m0 = np.empty((n, PROJ))
    for j in range(PROJ):  # a0 = m0, z1[o] = m0[:, j], logit = m0[:, j] * sum_k m1[:, k]
        w1 = z(PROJ, PROJ)
        w1[:, j] = 1
        m0[:, j] = logits(z(PROJ, PROJ), o(PROJ), w1, z(PROJ), o(1, PROJ)) / rowsum
    return m0, m1


def _snap(m, tag):
    """Every entry 0 or 1 / (1 - p): m1 is read directly (one fp32 rounding), m0 through a
    64-term fp32 sum and a division (1e-5 covers 64 roundings of 2^-24)."""
    kept = np.abs(m - KEEP) <= 1e-5 * KEEP
    assert (kept | (m == 0)).all(), (tag, m[~(kept | (m == 0))][:8])
    return np.where(kept, KEEP, 0.0)


def test_clf_head_dropout_masks_and_backward():
    n = N_DROP
    w, xbuf, demb, dlogit = _head_inputs(n, HEAD_SEEDS[n])
    keep, xd = _head_operands(w), xbuf.to(DEV)
    seed = torch.tensor([0x1234567], dtype=torch.int64, device=DEV)
    seed2 = torch.tensor([0x1234568], dtype=torch.int64, device=DEV)
    site = 0x5E2E
    probe = lambda s, st: tuple(  # noqa: E731
        _snap(m, k) for m, k in zip(_probe_masks(s, st, xd, keep[0], keep[2]), ("m0", "m1")))
    m0, m1 = probe(seed, site)
    for name, m in (("m0", m0), ("m1", m1)):
        rate = (m != 0).mean()
        print(f"{name}: keep rate {rate:.4f} (0.8 +- 0.015)")
        assert abs(rate - (1 - P_DROP)) <= 0.015
    assert not np.array_equal(m0, m1)  # the two layers draw different elements
    same, other_site, other_seed = probe(seed, site), probe(seed, site + 1), probe(seed2, site)
    assert np.array_equal(same[0], m0) and np.array_equal(same[1], m1)
    for a in (other_site, other_seed):
        for mine, theirs in zip((m0, m1), a):  # independent draws agree on ~68% of elements
            assert 0.5 < (mine == theirs).mean() < 0.85
    ref = lo.clf_head(xbuf[:, -1].numpy(), {k: v.numpy() for k, v in w.items()}, m0, m1,
                      demb.numpy(), dlogit.numpy())
    margin = relu_margin(ref, m0, m1)
    print(f"smallest kept |pre-activation| {margin:.3e} (needs {RELU_MARGIN:.0e})")
    assert margin >= RELU_MARGIN
    got = _run_head(n, keep, xd, P_DROP, seed, site, True, demb.to(DEV), dlogit.to(DEV), True)
    _check_head(got, ref, f"head n = {n} p = {P_DROP}")
    ones = np.ones_like(m0)
    plain = lo.clf_head(xbuf[:, -1].numpy(), {k: v.numpy() for k, v in w.items()}, ones, ones,
                        demb.numpy(), dlogit.numpy())
    assert np.abs(plain["dx"] - ref["dx"]).max() > 100 * REL_BAR * np.abs(ref["dx"]).max()
    with pytest.raises(KernelError):  # host-side argument check: nothing is launched
        _run_head(n, keep, xd, P_DROP, None, site, True, None, None, False)


# ------------------------------------------------------------------ fs2_bce_logits
SPECIAL = [0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4]
TARGETS = [0.0, 1.0, 0.3]
_BCE = {}


def _bce_inputs(n):
    if n not in _BCE:
        gen = torch.Generator().manual_seed(600 + n)
        x = torch.randn(n, generator=gen) * 4
        y = torch.tensor(TARGETS)[torch.randint(0, 3, (n,), generator=gen)]
        k = min(n, 3 * len(SPECIAL))  # every special logit under every target
        x[:k] = torch.tensor([s for s in SPECIAL for _ in TARGETS])[:k]
        y[:k] = torch.tensor(TARGETS * len(SPECIAL))[:k]
        g = torch.tensor([0.37])
        ref = {"rows": lo.bce_rows(x.numpy(), y.numpy()),
               None: lo.dbce(x.numpy(), y.numpy(), 1.0, 1.0),
               "g": lo.dbce(x.numpy(), y.numpy(), g.numpy()[0], 2.5)}
        _BCE[n] = (x, y, g, ref)
    return _BCE[n]


def _check_bce(got, want, tag):
    got = host(got)
    assert np.isfinite(got).all(), tag
    bar = 8 * 2.0 ** -23 * np.maximum(1.0, np.abs(want))
    err = np.abs(got - want) / bar
    print(f"{tag}: worst |got - want| / (8 * 2^-23 * max(1, |want|)) = {err.max():.3f} (bar 1)")
    assert (err <= 1).all(), (tag, err.max(), int(err.argmax()))


@pytest.mark.parametrize("use_g", [None, "g"])
@pytest.mark.parametrize("mode", ["rows", "gradient", "both"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_bce_logits_matches_float64(n, mode, use_g):
    x, y, g, ref = _bce_inputs(n)
    xd, yd, gd = x.to(DEV), y.to(DEV), g.to(DEV) if use_g else None
    rows = nan(n) if mode != "gradient" else None
    d = nan(n) if mode != "rows" else None
    lib.fs2_bce_logits(P(xd), P(yd), n, P(rows), P(gd), 2.5 if use_g else 1.0, P(d), K.stream())
    torch.cuda.synchronize()
    if rows is not None:
        _check_bce(rows, ref["rows"], f"bce rows n = {n}")
    if d is not None:
        _check_bce(d, ref[use_g], f"bce gradient n = {n} g = {use_g}")


# ------------------------------------------------------------------ fs2_rows_repad
# the last shape is 2.88 M elements: past 8192 * 256, where the grid-stride loop starts
@pytest.mark.parametrize("B,Ts,Td,C", [(3, 7, 10, 5), (3, 10, 7, 5), (2, 150, 150, 80),
                                       (48, 620, 750, 80)])
def test_rows_repad_is_exact(B, Ts, Td, C):
    x = torch.randn(B, Ts, C, generator=torch.Generator().manual_seed(Ts)) + 5.0
    xd, y = x.to(DEV), nan(B, Td, C)
    lib.fs2_rows_repad(P(xd), B, Ts, Td, C, P(y), K.stream())
    torch.cuda.synchronize()
    want = lo.repad(x.numpy(), Td)
    got = y.cpu().numpy()
    print(f"repad {(B, Ts, Td, C)}: {int((got != want).sum())} of {want.size} elements differ")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("T", [150, 151, 300])
def test_chunk_mels_and_its_gradient_are_exact(T):
    B, C = 2, 80
    gen = torch.Generator().manual_seed(T)
    mel = (torch.randn(B, T, C, generator=gen) + 5.0).to(DEV).requires_grad_()
    y, r = G.chunk_mels(mel)
    assert r == T // 150 + 1 and y.shape == (B * r, 150, C)
    want = lo.repad(mel.detach().cpu().numpy(), r * 150).reshape(B * r, 150, C)
    assert np.array_equal(y.detach().cpu().numpy(), want)
    if T % 150 == 0:  # the reference's extra all-zero chunk
        assert not want.reshape(B, r, 150, C)[:, -1].any()
    dy = torch.randn(B * r, 150, C, generator=gen) + 5.0
    y.backward(dy.to(DEV))
    assert np.array_equal(mel.grad.cpu().numpy(), lo.repad(dy.view(B, r * 150, C).numpy(), T))


# ------------------------------------------------------------------ fs2_repeat_col
@pytest.mark.parametrize("B,ld,col,rep", [(5, 4, 2, 3), (300, 7, 6, 1), (1, 1, 0, 257)])
def test_repeat_col_is_exact(B, ld, col, rep):
    meta = torch.randn(B, ld, generator=torch.Generator().manual_seed(B))
    md, y = meta.to(DEV), nan(B * rep)
    lib.fs2_repeat_col(P(md), B, ld, col, rep, P(y), K.stream())
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), lo.repeat_col(meta.numpy(), col, rep))
