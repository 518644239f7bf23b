"""The ``rescnn`` speaker encoder on the GPU: every kernel of ``csrc/rescnn.hip`` against
``rescnn_oracle`` (plain torch on the CPU, float64), then the module, a training step and
bitwise repeatability.

Convolutions are compared BIT FOR BIT on integer-lattice data (inputs in [-4, 4], weights in
[-2, 2]: every fp32 partial sum is an exact integer far below 2^24, whatever the summation
order).  Everything else is compared with the measured rule: the float32 oracle's own maximum
error against the float64 oracle on the same input, times 4 -- the margin covers a different
but equally valid summation order.  Each comparison prints its figures.
"""
import importlib

import pytest
import torch

import rescnn_oracle as O

pytestmark = pytest.mark.gpu

G = importlib.import_module("mid-attribute-speaker-generation_amd.ge2e")
KN = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
T = importlib.import_module("mid-attribute-speaker-generation_amd.embedder_train")
lib = importlib.import_module("mid-attribute-speaker-generation_amd._lib").lib
DEV = "cuda"
SENTINEL = 777777.25  # finite, and no integer: an exact-integer result never equals it
GUARD = 64


def ptr(t):
    return None if t is None else t.data_ptr()


def guarded(shape):
    """An output buffer pre-filled with the sentinel, with a guard band on either side."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return flat, flat[GUARD:GUARD + n].view(shape)


def check_guard(flat, out, tag):
    torch.cuda.synchronize()
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), \
        f"{tag}: wrote outside the buffer"
    assert torch.isfinite(out).all() and not (out == SENTINEL).any(), f"{tag}: element not written"


def close(got, r64, r32, tag):
    """|got - r64| <= 4 max|r32 - r64|."""
    got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
    assert got.shape == r64.shape, (tag, got.shape, r64.shape)
    assert torch.isfinite(got).all(), f"{tag}: non-finite"
    own = (r32 - r64).abs().max().item()
    err = (got - r64).abs().max().item()
    print(f"{tag}: err {err:.3e}  f32-oracle err {own:.3e}  bound {4 * own:.3e}  "
          f"scale {r64.abs().max().item():.3e}")
    assert err <= 4 * own, f"{tag}: max abs err {err:.3e} > 4 x {own:.3e}"
    return err


# ---------------------------------------------------------------- convolutions, bitwise
K5 = [(5, 2, ci, co, h, w) for (h, w) in ((10, 13),) for ci, co in ((1, 16), (16, 32), (64, 128))]
K3 = [(3, 1, c, c, h, w) for (h, w) in ((5, 10), (6, 7)) for c in (16, 128)]
TINY = [(k, s, ci, co, h, w) for (h, w) in ((1, 1), (2, 3))
        for (k, s, ci, co) in ((5, 2, 1, 16), (5, 2, 16, 32), (3, 1, 16, 16))]
# more than 1024 output positions: the weight gradient runs in several slices
SLICED = [(3, 1, 16, 16, 20, 37), (5, 2, 1, 16, 40, 75)]
CONV_CASES = K5 + K3 + TINY + SLICED


def lattice(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


@pytest.fixture(scope="module")
def conv_refs():
    """Integer-lattice inputs and the float64 oracle's forward / gradients, once per case."""
    out = {}
    for case in CONV_CASES:
        k, s, ci, co, h, w = case
        gen = torch.Generator().manual_seed(hash(case) % (2 ** 31))
        x = lattice(gen, -4, 4, 3, ci, h, w).requires_grad_()
        wt = lattice(gen, -2, 2, co, ci, k, k).requires_grad_()
        b = lattice(gen, -2, 2, co).requires_grad_()
        y = O.conv2d(x, wt, b, s, k // 2)
        dy = lattice(gen, -4, 4, *y.shape)
        (y * dy).sum().backward()
        out[case] = dict(x=x.detach(), w=wt.detach(), b=b.detach(), y=y.detach(), dy=dy,
                         dx=x.grad, dw=wt.grad, db=b.grad)
    return out


def prep_weight(w):
    w = w.float().to(DEV).contiguous()
    wf, wb = torch.empty_like(w), torch.empty_like(w)
    lib.fs2_conv2d_weight_prep(ptr(w), w.shape[0], w.shape[1], w.shape[2], ptr(wf), ptr(wb),
                               KN.stream())
    return wf, wb


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k%ds%d_%dto%d_%dx%d" % c)
def test_conv2d_forward_dgrad_wgrad_bitwise(conv_refs, case):
    k, s, ci, co, h, w = case
    r = conv_refs[case]
    n, pad = 3, k // 2
    x = O.to_nwhc(r["x"]).float().to(DEV)
    dy = O.to_nwhc(r["dy"]).float().to(DEV)
    bias = r["b"].float().to(DEV)
    wf, wb = prep_weight(r["w"])
    ho, wo = r["y"].shape[2:]
    # forward
    flat, y = guarded((n, wo, ho, co))
    lib.fs2_conv2d_fwd(ptr(x), n, w, h, ci, ptr(wf), ptr(bias), co, k, s, pad, None, None, None, 0,
                       ptr(y), KN.stream())
    check_guard(flat, y, "fwd")
    assert torch.equal(y.cpu(), O.to_nwhc(r["y"]).float())
    # data gradient
    flat, dx = guarded((n, w, h, ci))
    lib.fs2_conv2d_dgrad(ptr(dy), n, w, h, ci, ptr(wb), co, k, s, pad, None, ptr(dx), KN.stream())
    check_guard(flat, dx, "dgrad")
    assert torch.equal(dx.cpu(), O.to_nwhc(r["dx"]).float())
    # weight and bias gradient
    nb = lib.fs2_conv2d_wgrad_ws_bytes(n, w, h, ci, co, k, s, pad)
    ws = torch.full((nb // 4,), float("nan"), device=DEV)
    flat, dw = guarded((co, ci, k, k))
    flat_b, db = guarded((co,))
    lib.fs2_conv2d_wgrad(ptr(x), ptr(dy), n, w, h, ci, co, k, s, pad, ptr(dw), ptr(db), 0, ptr(ws),
                         nb, KN.stream())
    check_guard(flat, dw, "wgrad")
    check_guard(flat_b, db, "bgrad")
    assert torch.equal(dw.cpu(), r["dw"].float())
    assert torch.equal(db.cpu(), r["db"].float())


def test_conv2d_epilogue_and_accumulation(conv_refs):
    """The eval epilogue (bias, folded scale / shift, + residual, ReLU, in that order), the
    data gradient's ``add`` operand and beta = 1 of the weight gradient; all exact on the
    lattice (scale a power of two)."""
    case = (3, 1, 16, 16, 6, 7)
    k, s, ci, co, h, w = case
    r = conv_refs[case]
    n, pad = 3, 1
    gen = torch.Generator().manual_seed(5)
    x = O.to_nwhc(r["x"]).float().to(DEV)
    dy = O.to_nwhc(r["dy"]).float().to(DEV)
    wf, wb = prep_weight(r["w"])
    scale = (2.0 ** torch.randint(-1, 2, (co,), generator=gen).double())
    shift = lattice(gen, -3, 3, co)
    res = lattice(gen, -40, 40, *r["y"].shape)
    want = torch.relu(r["y"] * scale[None, :, None, None] + shift[None, :, None, None] + res)
    assert (want == 0).any() and (want > 0).any()
    y = torch.full((n, w, h, co), SENTINEL, device=DEV)
    bk, sk, hk = (t.float().to(DEV) for t in (r["b"], scale, shift))
    rk = O.to_nwhc(res).float().to(DEV)
    lib.fs2_conv2d_fwd(ptr(x), n, w, h, ci, ptr(wf), ptr(bk), co, k, s, pad, ptr(sk), ptr(hk),
                       ptr(rk), 1, ptr(y), KN.stream())
    assert torch.equal(y.cpu(), O.to_nwhc(want).float())
    add = lattice(gen, -9, 9, *r["x"].shape)
    dx = torch.full((n, w, h, ci), SENTINEL, device=DEV)
    ak = O.to_nwhc(add).float().to(DEV)
    lib.fs2_conv2d_dgrad(ptr(dy), n, w, h, ci, ptr(wb), co, k, s, pad, ptr(ak), ptr(dx),
                         KN.stream())
    assert torch.equal(dx.cpu(), O.to_nwhc(r["dx"] + add).float())
    nb = lib.fs2_conv2d_wgrad_ws_bytes(n, w, h, ci, co, k, s, pad)
    ws = torch.empty(nb // 4, device=DEV)
    dw0, db0 = lattice(gen, -5, 5, co, ci, k, k), lattice(gen, -5, 5, co)
    dw, db = dw0.float().to(DEV), db0.float().to(DEV)
    lib.fs2_conv2d_wgrad(ptr(x), ptr(dy), n, w, h, ci, co, k, s, pad, ptr(dw), ptr(db), 1, ptr(ws),
                         nb, KN.stream())
    assert torch.equal(dw.cpu(), (r["dw"] + dw0).float())
    assert torch.equal(db.cpu(), (r["db"] + db0).float())


# ---------------------------------------------------------------- BatchNorm2d
def bn_oracle(z, gamma, beta, res, dout, rm, rv, dtype, calls=1):
    z, gamma, beta, dout = (t.to(dtype).clone() for t in (z, gamma, beta, dout))
    z.requires_grad_(), gamma.requires_grad_(), beta.requires_grad_()
    res = res.to(dtype).clone().requires_grad_() if res is not None else None
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    n = z.numel() // z.shape[1]
    for _ in range(calls):
        y, mean, var = O.batchnorm_train(z, gamma, beta)
        rm = 0.9 * rm + 0.1 * mean.detach()
        rv = 0.9 * rv + 0.1 * var.detach() * n / (n - 1)
    pre = y + res if res is not None else y
    out = torch.relu(pre)
    (out * dout).sum().backward()
    return dict(out=out.detach(), pre=pre.detach(), bn=y.detach(), dz=z.grad, dgamma=gamma.grad,
                dbeta=beta.grad, dres=res.grad if res is not None else None, rm=rm, rv=rv,
                mean=mean.detach(), rstd=1 / torch.sqrt(var.detach() + O.EPS))


@pytest.mark.parametrize("c", (16, 128))
@pytest.mark.parametrize("residual", (False, True))
def test_batchnorm2d_relu_residual(c, residual):
    """(N, H, W) = (3, 10, 13): 390 rows, two statistics blocks, the second partial.  Channel 3
    is constant (variance 0, rstd = 1 / sqrt(eps)); two calls move the running statistics."""
    n, h, w = 3, 10, 13
    gen = torch.Generator().manual_seed(c + residual)
    z = torch.randn(n, c, h, w, generator=gen) * 1.5 + 0.3
    z[:, 3] = 1.5
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.3
    res = torch.randn(n, c, h, w, generator=gen) if residual else None
    dout = torch.randn(n, c, h, w, generator=gen)
    rm0, rv0 = torch.randn(c, generator=gen) * 0.2, torch.rand(c, generator=gen) + 0.5
    r64 = bn_oracle(z, gamma, beta, res, dout, rm0, rv0, torch.float64, calls=2)
    r32 = bn_oracle(z, gamma, beta, res, dout, rm0, rv0, torch.float32, calls=2)
    assert r64["rstd"][3] == 1 / torch.sqrt(torch.tensor(O.EPS, dtype=torch.float64))
    if residual:  # the add comes BEFORE the ReLU: relu(bn) + res would differ
        other = torch.relu(r64["bn"]) + res.double()
        assert ((other - r64["out"]).abs() > 0.1).any()
    rows = n * h * w
    zk = O.to_nwhc(z).to(DEV)
    resk = O.to_nwhc(res).to(DEV) if residual else None
    g_, b_ = gamma.to(DEV), beta.to(DEV)
    rm, rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    stats = torch.full((2, c), SENTINEL, device=DEV)
    nb = lib.fs2_bn2d_ws_bytes(rows, c)
    ws = torch.full((nb // 4,), float("nan"), device=DEV)
    for _ in range(2):
        flat, out = guarded((n, w, h, c))
        lib.fs2_bn2d_fwd(ptr(zk), rows, c, ptr(g_), ptr(b_), O.EPS, O.MOMENTUM, ptr(rm), ptr(rv),
                         ptr(nbt), ptr(stats[0]), ptr(stats[1]), ptr(resk), 1, ptr(out), ptr(ws), nb,
                         KN.stream())
        check_guard(flat, out, "bn fwd")
    tag = f"bn c={c} res={residual}"
    close(O.from_nwhc(out), r64["out"], r32["out"], tag + " out")
    close(stats[0], r64["mean"], r32["mean"], tag + " mean")
    close(stats[1], r64["rstd"], r32["rstd"], tag + " rstd")
    close(rm, r64["rm"], r32["rm"], tag + " running_mean")
    close(rv, r64["rv"], r32["rv"], tag + " running_var")
    assert nbt.item() == 2
    assert torch.equal(out[..., 3].cpu(), O.to_nwhc(torch.relu(
        (beta[3] + (res[:, 3:4] if residual else 0)).float().expand(n, 1, h, w)))[..., 0])
    # backward
    doutk = O.to_nwhc(dout).to(DEV)
    flat_g, g = guarded((n, w, h, c))
    flat_z, dz = guarded((n, w, h, c))
    dgb = torch.full((2, c), SENTINEL, device=DEV)
    lib.fs2_bn2d_bwd(ptr(doutk), ptr(out), ptr(zk), ptr(stats[0]), ptr(stats[1]), ptr(g_), rows, c,
                     1, ptr(g), ptr(dz), ptr(dgb[0]), ptr(dgb[1]), ptr(ws), nb, KN.stream())
    check_guard(flat_g, g, "bn bwd g")
    check_guard(flat_z, dz, "bn bwd dz")
    close(O.from_nwhc(dz), r64["dz"], r32["dz"], tag + " dz")
    close(dgb[0], r64["dgamma"], r32["dgamma"], tag + " dgamma")
    close(dgb[1], r64["dbeta"], r32["dbeta"], tag + " dbeta")
    # g is the ReLU-masked upstream gradient, exactly: the residual branch's gradient
    mask = (out > 0).float()
    assert torch.equal(g, doutk * mask)
    sure = r64["pre"].abs() > 1e-4  # away from the ReLU's kink the mask is the oracle's
    assert torch.equal((O.from_nwhc(out).cpu() > 0)[sure], (r64["pre"] > 0)[sure])
    if residual:
        assert torch.equal(O.from_nwhc(g).cpu()[sure], r32["dres"][sure])


# ---------------------------------------------------------------- pool + dropout + flatten
def pool(x, p, seed):
    n, w, h, c = x.shape
    out = torch.full((n, c * h), SENTINEL, device=DEV)
    lib.fs2_pool_drop_fwd(ptr(x), n, w, h, c, p, ptr(seed), 0x5E2F, ptr(out), KN.stream())
    return out


def pool_bwd(d, shape, p, seed):
    n, w, h, c = shape
    dx = torch.full(shape, SENTINEL, device=DEV)
    lib.fs2_pool_drop_bwd(ptr(d), n, w, h, c, p, ptr(seed), 0x5E2F, ptr(dx), KN.stream())
    return dx


def test_pool_flatten_and_dropout():
    n, w, h, c = 8, 3, 5, 128
    gen = torch.Generator().manual_seed(11)
    a = torch.randn(n, c, h, w, generator=gen)
    ak = O.to_nwhc(a).to(DEV)
    plain = pool(ak, 0.0, None)
    close(plain, O.pool_flatten(a.double()), O.pool_flatten(a), "pool")
    d = torch.randn(n, c * h, generator=gen)
    a64 = a.double().requires_grad_()
    (O.pool_flatten(a64) * d.double()).sum().backward()
    a32 = a.clone().requires_grad_()
    (O.pool_flatten(a32) * d).sum().backward()
    dx = pool_bwd(d.to(DEV), (n, w, h, c), 0.0, None)
    close(O.from_nwhc(dx), a64.grad, a32.grad, "pool bwd")
    # dropout 0.5: 5120 features, sigma = sqrt(5120) / 2 = 35.8, 6 sigma = 215
    s1 = torch.tensor([1234567], dtype=torch.int64, device=DEV)
    s2 = torch.tensor([7654321], dtype=torch.int64, device=DEV)
    o1, o1b, o2 = pool(ak, 0.5, s1), pool(ak, 0.5, s1), pool(ak, 0.5, s2)
    assert (plain != 0).all()
    kept = o1 != 0
    print(f"dropout kept {int(kept.sum())} of {kept.numel()}")
    assert abs(int(kept.sum()) - 2560) <= 215
    assert torch.equal(o1[kept], 2 * plain[kept]) and (o1[~kept] == 0).all()
    assert torch.equal(o1, o1b) and not torch.equal(o1 != 0, o2 != 0)
    ones = torch.ones(n, c * h, device=DEV)
    dx = pool_bwd(ones, (n, w, h, c), 0.5, s1)  # (n, w, h, c): zero exactly where the output is
    dmask = dx.permute(0, 3, 2, 1).reshape(n, c * h, w)  # -> (n, c * h + h, w)
    assert torch.equal(dmask != 0, kept[:, :, None].expand(n, c * h, w))
    assert torch.equal(dmask[kept], torch.full_like(dmask[kept], 2.0 / w))


# ---------------------------------------------------------------- head at width 640
def test_head_640_forward_backward_and_weight_gradients():
    torch.manual_seed(3)
    m = G.SpeechEmbedder("cpu", architecture="rescnn")
    sd = m.state_dict()
    n = 5  # two blocks of four rows
    feat = torch.randn(n, 640) * 0.5
    demb, dlogit = torch.randn(n, 64), torch.randn(n)
    refs = {}
    for dt in (torch.float64, torch.float32):
        o = O.Oracle(sd, dt)
        f = feat.to(dt).clone().requires_grad_()
        emb, logit = o.head(f)
        ((emb * demb.to(dt)).sum() + (logit * dlogit.to(dt)).sum()).backward()
        refs[dt] = dict(emb=emb.detach(), logit=logit.detach(), dx=f.grad,
                        grads=[o.par[p + k].grad for p in O.Oracle.HEAD for k in ("weight", "bias")])
    r64, r32 = refs[torch.float64], refs[torch.float32]
    W = [sd[p + k].to(DEV) for p in O.Oracle.HEAD for k in ("weight", "bias")]
    tr = lambda t: t.t().contiguous()  # noqa: E731
    ops = (W[0], tr(W[0]), W[1], W[2], tr(W[2]), W[3], W[4], tr(W[4]), W[5], W[6], W[7])
    head = tuple(ptr(t) for t in ops)
    x = feat.to(DEV)
    emb, logit = torch.full((n, 64), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
    lib.fs2_clf_head_w(ptr(x), 640, n, 640, *head, 0.0, None, 1, ptr(emb), ptr(logit), None, None,
                       None, 0, KN.stream())
    close(emb, r64["emb"], r32["emb"], "head emb")
    close(logit, r64["logit"], r32["logit"], "head logit")
    de, dl = demb.to(DEV), dlogit.to(DEV)
    flat, dx = guarded((n, 640))
    lib.fs2_clf_head_w(ptr(x), 640, n, 640, *head, 0.0, None, 1, None, None, ptr(de), ptr(dl),
                       ptr(dx), 640, KN.stream())
    check_guard(flat, dx, "head dx")
    close(dx, r64["dx"], r32["dx"], "head dx")
    outs = [torch.full(g.shape, SENTINEL, device=DEV) for g in r64["grads"]]
    nb = lib.fs2_clf_head_w_wgrad_ws_bytes(n)
    ws = torch.full((nb // 4,), float("nan"), device=DEV)
    lib.fs2_clf_head_w_wgrad(ptr(x), 640, n, 640, *head, 0.0, None, 1, ptr(de), ptr(dl),
                             *[ptr(t) for t in outs], 0, ptr(ws), nb, KN.stream())
    names = [p + k for p in O.Oracle.HEAD for k in ("weight", "bias")]
    for name, got, a, b in zip(names, outs, r64["grads"], r32["grads"]):
        close(got, a, b, "head " + name)


# ---------------------------------------------------------------- the module
def randomise_(m, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.startswith("_feat_extractor.conv_layer"):
                continue  # aliases
            u = torch.rand(v.shape, generator=gen)
            if k.endswith("bn.weight"):
                v.copy_(0.5 + u)
            elif k.endswith(("bn.bias", "running_mean", "conv.bias")):
                v.copy_(0.6 * u - 0.3)
            elif k.endswith("running_var"):
                v.copy_(0.5 + 1.5 * u)
    return m


def new_module(weight_grads, seed=0):
    torch.manual_seed(seed)
    m = randomise_(G.SpeechEmbedder(DEV, weight_grads, "rescnn"), seed)
    m.feat_dropout = m.da_dropout = 0.0
    return m


def oracle_run(sd, x, langs, gemb, dtype, training=True, detach=False):
    o = O.Oracle(sd, dtype)
    xin = x.detach().to(dtype).clone().requires_grad_()
    out = o.forward(xin, training, detach)
    res = dict(emb=out["embeddings"].detach(), logit=out["da_lang_logits"].detach(), buf=o.buf)
    if langs is not None:
        loss = O.bce_sum(out["da_lang_logits"], langs)
        if gemb is not None:
            loss = loss + (out["embeddings"] * gemb.to(dtype)).sum()
        loss.backward()
        res["dx"] = xin.grad
        res["grads"] = {k: v.grad for k, v in o.par.items()}
    return res


def module_case(t_len):
    gen = torch.Generator().manual_seed(100 + t_len)
    x = torch.randn(4, t_len, 80, generator=gen)
    langs = torch.tensor([0.0, 1.0, 1.0, 0.0])
    gemb = torch.randn(4, 64, generator=gen)
    m = new_module(True, seed=t_len)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ref = {dt: oracle_run(sd, x, langs, gemb, dt) for dt in (torch.float64, torch.float32)}
    return dict(x=x, langs=langs, gemb=gemb, m=m, sd=sd, ref=ref)


@pytest.fixture(scope="module")
def case19():
    return module_case(19)


def check_all_grads(m, ref, tag):
    r64, r32 = ref[torch.float64]["grads"], ref[torch.float32]["grads"]
    named = dict(m.named_parameters())
    assert len(named) == 56
    for k, p in named.items():
        assert p.grad is not None, k
        close(p.grad, r64[k], r32[k], f"{tag} d {k}")


def test_module_training_forward_and_all_gradients(case19):
    c = case19
    m, ref = c["m"], c["ref"]
    m.train()
    x = c["x"].to(DEV).requires_grad_()
    out = m(x)
    close(out["embeddings"], ref[torch.float64]["emb"], ref[torch.float32]["emb"], "T19 emb")
    close(out["da_lang_logits"], ref[torch.float64]["logit"], ref[torch.float32]["logit"],
          "T19 logit")
    for k, v in m.state_dict().items():
        if k.endswith(("running_mean", "running_var")) and "conv_layer" not in k:
            close(v, ref[torch.float64]["buf"][k], ref[torch.float32]["buf"][k], "T19 " + k)
        elif k.endswith("num_batches_tracked"):
            assert v.item() == 1
    loss = G._BCESumFn.apply(out["da_lang_logits"], c["langs"].to(DEV)) + \
        (out["embeddings"] * c["gemb"].to(DEV)).sum()
    loss.backward()
    close(x.grad, ref[torch.float64]["dx"], ref[torch.float32]["dx"], "T19 dx")
    check_all_grads(m, ref, "T19")


def test_module_eval_forward(case19):
    c = case19
    m = new_module(False, seed=19)
    m.load_state_dict(c["sd"])
    m.eval()
    r = {dt: oracle_run(c["sd"], c["x"], None, None, dt, training=False)
         for dt in (torch.float64, torch.float32)}
    with torch.no_grad():
        out = m(c["x"].to(DEV))
    close(out["embeddings"], r[torch.float64]["emb"], r[torch.float32]["emb"], "eval emb")
    close(out["da_lang_logits"], r[torch.float64]["logit"], r[torch.float32]["logit"], "eval logit")
    for k, v in m.state_dict().items():  # nothing moved
        assert torch.equal(v.cpu(), c["sd"][k]), k
    emb = m.compute_embedding(c["x"].to(DEV))["embeddings"]
    assert torch.equal(emb, out["embeddings"])


def test_module_input_gradient_without_weight_grads(case19):
    """The ``--use_clf`` discriminator: BCE(logits, langs) back to the mel input only."""
    c = case19
    m = new_module(False, seed=19)
    m.load_state_dict(c["sd"])
    m.train()
    r = {dt: oracle_run(c["sd"], c["x"], c["langs"], None, dt)
         for dt in (torch.float64, torch.float32)}
    x = c["x"].to(DEV).requires_grad_()
    G._BCESumFn.apply(m(x)["da_lang_logits"], c["langs"].to(DEV)).backward()
    close(x.grad, r[torch.float64]["dx"], r[torch.float32]["dx"], "use_clf dx")
    assert all(p.grad is None for p in m.parameters())


def test_module_detach_trains_the_classifier_alone(case19):
    c = case19
    m = new_module(True, seed=19)
    m.load_state_dict(c["sd"])
    m.train()
    r = {dt: oracle_run(c["sd"], c["x"], c["langs"], None, dt, detach=True)
         for dt in (torch.float64, torch.float32)}
    out = m(c["x"].to(DEV), detach=True)
    assert not out["embeddings"].requires_grad
    G._BCESumFn.apply(out["da_lang_logits"], c["langs"].to(DEV)).backward()
    da = {id(p) for p in m.da_parameters()}
    for k, p in m.named_parameters():
        if id(p) in da:
            close(p.grad, r[torch.float64]["grads"][k], r[torch.float32]["grads"][k], "detach " + k)
        else:
            assert p.grad is None, k


def test_module_at_150_frames():
    """The true extents: W = 150, 75, 38, 19, 10."""
    c = module_case(150)
    m, ref = c["m"], c["ref"]
    m.train()
    x = c["x"].to(DEV).requires_grad_()
    out = m(x)
    close(out["embeddings"], ref[torch.float64]["emb"], ref[torch.float32]["emb"], "T150 emb")
    close(out["da_lang_logits"], ref[torch.float64]["logit"], ref[torch.float32]["logit"],
          "T150 logit")
    loss = G._BCESumFn.apply(out["da_lang_logits"], c["langs"].to(DEV)) + \
        (out["embeddings"] * c["gemb"].to(DEV)).sum()
    loss.backward()
    close(x.grad, ref[torch.float64]["dx"], ref[torch.float32]["dx"], "T150 dx")
    check_all_grads(m, ref, "T150")


def test_backward_is_bitwise_repeatable(case19):
    c = case19
    grads = []
    for _ in range(2):
        m = new_module(True, seed=19)
        m.load_state_dict(c["sd"])
        m.train()
        x = c["x"].to(DEV).requires_grad_()
        out = m(x)
        (G._BCESumFn.apply(out["da_lang_logits"], c["langs"].to(DEV)) +
         (out["embeddings"] * c["gemb"].to(DEV)).sum()).backward()
        grads.append([x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    assert len(grads[0]) == 57
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- training step
def oracle_step(sd, w, b, mels, langs, n_utt, dtype):
    """One batch of the training loop in the oracle, from the given state: the five scalars
    ``train_step`` returns (loss, da_loss, the norms of the main / ge2e / da gradients before
    clipping), the 58 gradients (both losses summed) and the BatchNorm buffers afterwards."""
    o = O.Oracle(sd, dtype)
    w = w.detach().cpu().to(dtype).clone().requires_grad_()
    b = b.detach().cpu().to(dtype).clone().requires_grad_()
    out = o.forward(mels.to(dtype), True)
    emb = out["embeddings"].view(mels.shape[0] // n_utt, n_utt, -1)
    loss = O.ge2e_softmax(emb, w, b)
    da = O.bce_sum(out["da_lang_logits"], langs)
    (loss + da).backward()
    norm = lambda ps: torch.cat([p.grad.flatten() for p in ps]).norm()  # noqa: E731
    scal = torch.stack([loss.detach(), da.detach(), norm(o.main_parameters()), norm([w, b]),
                        norm(o.da_parameters())])
    grads = {k: v.grad for k, v in o.par.items()}
    grads.update({"ge2e.w": w.grad, "ge2e.b": b.grad})
    return dict(scal=scal, grads=grads, buf=o.buf)


class AdamFromGradients:
    """``torch.optim.Adam`` + ``clip_grad_norm_`` in ``dtype`` on the CPU over clones of the
    initial parameters, fed gradients from outside: the three optimisers of
    ``train_speech_embedder.py:104-113``."""

    def __init__(self, init, groups, dtype):
        self.dtype = dtype
        self.par = {k: v.detach().cpu().to(dtype).clone().requires_grad_() for k, v in init.items()}
        self.opt = [(keys, torch.optim.Adam([self.par[k] for k in keys], lr=1e-3, weight_decay=wd),
                     clip) for keys, wd, clip in groups]

    def step(self, grads):
        for keys, opt, clip in self.opt:
            for k in keys:
                self.par[k].grad = grads[k].detach().cpu().to(self.dtype).clone()
            torch.nn.utils.clip_grad_norm_([self.par[k] for k in keys], clip)
            opt.step()


def close_ulp(got, r64, r32, tag, scale=None):
    """``close`` with a floor of one float32 ulp of the reference's largest magnitude (or of
    ``scale``, where the value is a difference of larger terms): two correct float32 results
    may round a value to neighbouring floats while the float32 oracle happens to land on the
    float64 value."""
    got, r64, r32 = got.detach().double().cpu(), r64.detach().double(), r32.detach().double()
    assert got.shape == r64.shape and torch.isfinite(got).all(), tag
    own = (r32 - r64).abs().max().item()
    err = (got - r64).abs().max().item()
    ulp = 2.0 ** -23 * (r64.abs().max().item() if scale is None else scale)
    bound = max(4 * own, ulp)
    print(f"{tag}: err {err:.3e}  f32-oracle err {own:.3e}  ulp {ulp:.3e}  bound {bound:.3e}")
    assert err <= bound, f"{tag}: max abs err {err:.3e} > max(4 x {own:.3e}, {ulp:.3e})"


SCALARS = ("loss", "da_loss", "norm main", "norm ge2e", "norm da")


def test_trainer_steps_a_rescnn_embedder():
    """Two ``train_step``s (``ge2e_backward=True``, 3 x 3 windows, T = 19, dropouts 0) against
    the oracle and ``torch.optim.Adam``, each step checked from the state the kernels
    entered it with:

    * the oracle (float64, float32) runs the batch from the module's own parameters and
      buffers before the step; each of the five returned scalars on its own (loss, da_loss,
      the three norms), each of the 58 gradients in the arenas (56 parameters, GE2E w and b,
      both backward passes summed) and every BatchNorm buffer after the step must be within
      4 x the float32 oracle's error (the scalars with a floor of one float32 ulp);
    * the update, tensor by tensor: the parameters after the step against
      ``torch.optim.Adam`` + ``clip_grad_norm_`` in float64, which keeps its moments over both
      steps and is fed the kernels' own gradients; bound 4 x the error of the same Adam in
      float32, floor one ulp.  A missing, doubled or wrongly signed update of any tensor is
      off by about lr = 1e-3, four to five orders above that bound.

    Why not one oracle trajectory over both steps: Adam's update lr g / (|g| + 1e-8) has the
    derivative lr 1e-8 / (|g| + 1e-8)^2, up to 1e5 lr where a clipped gradient element is near
    zero.  There the float32 rounding of the gradient decides a full step of 1e-3, for the
    float32 oracle as for the kernels (measured after two steps: 1.7e-3 for both), each
    tensor's largest deviation belongs to its one or two such elements, and a ratio of two
    independent roundings exceeds 4 with probability (2 / pi) atan(1 / 4) = 16 % per tensor;
    the second step's scalars and buffers inherit those deviations (measured: da_loss off by
    1.9e-6 where the float32 oracle happened to be off by 3.5e-8).  Anchoring every step at
    the kernels' state takes the amplification out and leaves what is to be checked: the
    gradients, the statistics and the update rule."""
    n_spk, n_utt, t_len = 3, 3, 19
    gen = torch.Generator().manual_seed(77)
    mels = torch.randn(n_spk * n_utt, t_len, 80, generator=gen)
    langs = torch.tensor([0.0, 0, 0, 1, 1, 1, 0, 0, 0])
    emb = new_module(True, seed=7)
    tr = T.EmbedderTrainer(embedder=emb, device=DEV, n_utt=n_utt)
    assert tr.optimizers["main"].arena.numel == sum(p.numel() for p in emb.main_parameters())
    emb.train()
    named = dict(emb.named_parameters())
    named.update({"ge2e.w": tr.criterion.w, "ge2e.b": tr.criterion.b})
    da_ids = {id(p) for p in emb.da_parameters()}
    groups = [([k for k, p in named.items() if id(p) not in da_ids and "ge2e" not in k], 1e-6, 3.0),
              (["ge2e.w", "ge2e.b"], 0.0, 1.0),
              ([k for k, p in named.items() if id(p) in da_ids], 1e-6, 3.0)]
    assert [len(g[0]) for g in groups] == [50, 2, 6]
    a64 = AdamFromGradients(named, groups, torch.float64)
    a32 = AdamFromGradients(named, groups, torch.float32)
    for step in range(2):
        sd = {k: v.detach().cpu().clone() for k, v in emb.state_dict().items()}
        before = {k: p.detach().clone() for k, p in named.items()}
        r64, r32 = (oracle_step(sd, before["ge2e.w"], before["ge2e.b"], mels, langs, n_utt, dt)
                    for dt in (torch.float64, torch.float32))
        got = torch.stack(tr.train_step(mels.to(DEV), langs.to(DEV), 0.0, ge2e_backward=True))
        # What fs2_ge2e_softmax returns cancels: the loss is a sum over the 9 windows of
        # log-sum-exp(S) - S_jj, differences of terms as large as |w| + |b|, and dw, db (so
        # their norm) are sums over 9 windows x 3 speakers of (softmax - one-hot) x cosine,
        # terms of up to 1 that nearly cancel once the loss is small.  Their rounding floor is
        # an ulp of the summed magnitudes, 9 (|w| + |b|) and 27, not of the small result.
        rows = mels.shape[0]
        lse = rows * (before["ge2e.w"].abs() + before["ge2e.b"].abs()).item()
        floors = {"loss": lse, "norm ge2e": rows * n_spk}
        for i, name in enumerate(SCALARS):
            close_ulp(got[i], r64["scal"][i], r32["scal"][i], f"step {step} {name}",
                      scale=floors.get(name))
        grads = {k: p.grad.detach().clone() for k, p in named.items()}
        for k, g in grads.items():
            if k.startswith("ge2e."):
                close_ulp(g, r64["grads"][k], r32["grads"][k], f"step {step} d {k}",
                          scale=rows * n_spk)
            else:
                close(g, r64["grads"][k], r32["grads"][k], f"step {step} d {k}")
        for k, v in emb.state_dict().items():
            if k.endswith(("running_mean", "running_var")) and "conv_layer" not in k:
                close(v, r64["buf"][k], r32["buf"][k], f"step {step} {k}")
            elif k.endswith("num_batches_tracked"):
                assert v.item() == step + 1
        a64.step(grads)
        a32.step(grads)
        for k, p in named.items():
            assert not torch.equal(p, before[k]), f"step {step}: {k} did not move"
            close_ulp(p, a64.par[k], a32.par[k], f"step {step} update {k}")
    # the evaluation paths take the same embedder: EER of one (N, M, T, 80) batch, a d-vector
    batch = torch.randn(2, 4, t_len, 80, generator=gen).to(DEV)
    eer = tr.evaluate_eer([batch])
    assert 0.0 <= eer <= 1.0
    mel = torch.randn(80, 200, generator=gen).to(DEV)
    dv = tr.dvector(mel)
    assert dv.shape == (64,) and torch.isfinite(dv).all()
    assert abs(dv.norm().item() - 1.0) < 1e-5
    assert emb.training  # the evaluation restored the mode
    state = {k: v.detach().cpu() for k, v in emb.state_dict().items()}
    wins = torch.stack([mel[:, s:s + 130].t() for s in (0, 65)]).cpu()
    e = O.Oracle(state).forward(wins, training=False)["embeddings"].mean(0)
    e32 = O.Oracle(state, torch.float32).forward(wins, training=False)["embeddings"].mean(0)
    close(dv, e / e.norm(), e32 / e32.norm(), "dvector")


# ---------------------------------------------------------------- dropout through the module
def test_module_feature_dropout_seed_and_site(case19):
    """``feat_dropout = 0.5`` with the classifier's dropout off: the key still advances per
    call (the masks of two calls differ), ``seed()`` keys the new site (the same seed repeats
    the call bit for bit, another does not), and the mask is the one ``fs2_pool_drop_fwd`` draws
    for (this call's key, ``site_feat``): with it as the oracle's keep-scale, embeddings,
    logits and the input gradient agree under the 4 x rule."""
    c = case19
    m = new_module(False, seed=19)
    m.load_state_dict(c["sd"])
    m.feat_dropout = 0.5
    m.train()
    x = c["x"].to(DEV)
    langs = c["langs"].to(DEV)

    def run(seed):
        m.load_state_dict(c["sd"])  # the running statistics back to the start
        m.seed(seed)
        xin = x.clone().requires_grad_()
        out = m(xin)
        key = m._seed_state[2:3].clone()
        G._BCESumFn.apply(out["da_lang_logits"], langs).backward()
        return out["embeddings"].detach(), out["da_lang_logits"].detach(), xin.grad, key

    e1, l1, g1, key = run(1234)
    with torch.no_grad():
        e_next = m(x)["embeddings"]  # a second call under the same seed: the next key
    e2, l2, g2, key2 = run(1234)
    e3 = run(4321)[0]
    assert torch.equal(e1, e2) and torch.equal(l1, l2) and torch.equal(g1, g2)
    assert torch.equal(key, key2)
    assert not torch.equal(e1, e_next) and not torch.equal(e1, e3)
    ones = torch.ones(4, 1, 5, 128, device=DEV)
    keep = torch.empty(4, 640, device=DEV)
    lib.fs2_pool_drop_fwd(ptr(ones), 4, 1, 5, 128, 0.5, ptr(key), m.site_feat, ptr(keep),
                          KN.stream())
    kept = int((keep != 0).sum())
    print(f"module dropout kept {kept} of 2560")
    assert ((keep == 0) | (keep == 2)).all() and abs(kept - 1280) <= 152  # 6 sigma = 6 sqrt(2560)/2
    ref = {}
    for dt in (torch.float64, torch.float32):
        o = O.Oracle(c["sd"], dt)
        xin = c["x"].detach().to(dt).clone().requires_grad_()
        out = o.forward(xin, True, keep=keep.cpu())
        O.bce_sum(out["da_lang_logits"], c["langs"]).backward()
        ref[dt] = (out["embeddings"].detach(), out["da_lang_logits"].detach(), xin.grad)
    for got, a, b, tag in zip((e1, l1, g1), ref[torch.float64], ref[torch.float32],
                              ("emb", "logit", "dx")):
        close(got, a, b, "dropout " + tag)


def test_eval_backward_raises_before_touching_gradients(case19):
    c = case19
    m = new_module(True, seed=19)
    m.load_state_dict(c["sd"])
    m.eval()
    out = m(c["x"].to(DEV).requires_grad_())
    with pytest.raises(NotImplementedError):
        G._BCESumFn.apply(out["da_lang_logits"], c["langs"].to(DEV)).backward()
    assert all(p.grad is None for p in m.parameters())


def test_eval_fold_follows_the_running_statistics(case19):
    """The folded scale / shift are cached beside the prepared weights; a training-mode
    forward moves the running statistics in place and must drop them."""
    c = case19
    m = new_module(False, seed=19)
    m.load_state_dict(c["sd"])
    x = c["x"].to(DEV)
    with torch.no_grad():
        m.eval()
        first, again = m(x)["embeddings"], m(x)["embeddings"]
        m.train()
        m(x)
        m.eval()
        after = m(x)["embeddings"]
    assert torch.equal(first, again) and not torch.equal(first, after)
    ref = {}
    for dt in (torch.float64, torch.float32):
        o = O.Oracle(c["sd"], dt)
        o.forward(c["x"], True)
        ref[dt] = o.forward(c["x"], False)["embeddings"].detach()
    close(after, ref[torch.float64], ref[torch.float32], "eval after a training forward")
