"""The GMM speaker-prior kernels of ``csrc/loss.hip`` (``gmm_head_fwd``, ``gmm_logprob``,
``gmm_head_bwd``, ``mean_k``, ``gmm_sample``) one by one, against a float64 torch-autograd
restatement of the whole head on the CPU:

    linear -> softmax / softplus -> GMMParams.log_prob(eps = float32 eps) -> sum_b g_b logp_b

whose gradients are the six weight gradients, and whose ``softmax(comp + log_mix)`` are the
responsibilities.  The inputs are float32 tensors upcast, so the kernels and the reference
see bit-identical inputs.  Tolerances are the project's own (``test_gmm_head_and_loss_vs_
reference``): 1e-5 of the reference's max-abs for pi / mu / sigma / sigma_pre / logp / mean,
1e-4 of it for the weight gradients, and 1e-5 absolute for the responsibilities; where a test
uses another bound its docstring derives it.
"""
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fs2_cpu

pytestmark = pytest.mark.gpu
KN = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
KernelError = importlib.import_module("mid-attribute-speaker-generation_amd._lib").KernelError
DEV = "cuda"
EPS32 = float(torch.finfo(torch.float32).eps)
GRADS = ("dw_pi", "db_pi", "dw_s", "db_s", "dw_mu", "db_mu")  # the C-ABI's order


def close(a, b, tol, tag, floor=0.0):
    """|a - b| <= tol * max|b| (or ``floor``, where a test derives an absolute bound)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{tag}: non-finite kernel output"
    scale = max(b.abs().max().item(), 1e-6) if b.numel() else 1.0
    err = (a - b).abs().max().item() if b.numel() else 0.0
    bound = max(tol * scale, floor)
    print(f"{tag}: err {err:.3e} scale {scale:.3e} bound {bound:.3e}")
    assert err <= bound, f"{tag}: max abs err {err:.3e} > {bound:.3e} (scale {scale:.3e})"
    return err


# ------------------------------------------------------------------ the reference
def ref_head(meta, W, e, K, D, g_logp=None, dtype=torch.float64):
    """The head in ``dtype`` on the CPU from float32 inputs: forward tensors, responsibilities
    and (with ``g_logp``) the gradients of sum_b g_b logp_b to the six weights."""
    w = [t.detach().cpu().to(dtype).requires_grad_() for t in W]
    w_pi, b_pi, w_s, b_s, w_mu, b_mu = w
    m, x = meta.cpu().to(dtype), e.cpu().to(dtype)
    pi = torch.softmax(F.linear(m, w_pi, b_pi), dim=1)
    pre = F.linear(m, w_s, b_s).view(-1, K, D)
    sigma = F.softplus(pre)  # threshold 20, as nn.Softplus() and the kernel
    mu = F.linear(m, w_mu, b_mu).view(-1, K, D)
    logp = fs2_cpu.GMMParams(pi, mu, sigma).log_prob(x, eps=EPS32)
    probs = pi / pi.sum(-1, keepdim=True)
    log_mix = torch.log_softmax(torch.log(probs.clamp(min=EPS32, max=1 - EPS32)), dim=-1)
    comp = (-((x[:, None, :] - mu) ** 2) / (2 * sigma ** 2) - torch.log(sigma)
            - math.log(math.sqrt(2 * math.pi))).sum(-1)
    assert torch.allclose(torch.logsumexp(comp + log_mix, -1), logp, rtol=1e-6 if dtype ==
                          torch.float32 else 1e-12)
    out = {"pi": pi, "mu": mu, "sigma": sigma, "sigma_pre": pre, "logp": logp, "probs": probs,
           "resp": torch.softmax(comp + log_mix, dim=-1)}
    if g_logp is not None:
        gr = torch.autograd.grad((g_logp.cpu().to(dtype) * logp).sum(), w, allow_unused=True)
        out.update({n: (torch.zeros_like(p) if g is None else g) for n, g, p in zip(GRADS, gr, w)})
    return {k: v.detach() for k, v in out.items()}


def make_inputs(B, I, K, D, seed):
    """Random head at (B, in_dim, K, D).  The components differ little (mu weights 0.1, sigma
    weights 0.2, both shrunk as 1 / sqrt(D) above D = 16) and e lies 0.3 from their mean, so
    that their log-densities differ by O(1) and the responsibilities are not one-hot: an error
    in one component's sum then shows in ``resp`` and in every gradient."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    meta = r(B, I)
    c = min(1.0, 4.0 / math.sqrt(D))  # keeps the sum over D of the components' differences O(1)
    W = [r(K, I) * 0.5, r(K) * 0.5, r(K * D, I) * 0.2 * c, -0.5 + 0.2 * c * r(K * D),
         r(K * D, I) * 0.1 * c, r(K * D) * 0.1 * c]
    mu = (F.linear(meta.double(), W[4].double(), W[5].double())).view(B, K, D)
    e = (mu.mean(1) + 0.3 * r(B, D).double()).float()
    g = 1.0 + 0.5 * r(B)  # non-uniform d loss / d logp
    return meta, W, e, g


def run_head(meta, W, e, K, D, denom=None):
    meta_d, e_d = meta.to(DEV).contiguous(), e.to(DEV).contiguous()
    W_d = [t.to(DEV).contiguous() for t in W]
    pi, mu, sigma, pre = KN.gmm_head_fwd(meta_d, *W_d, K, D)
    logp, resp, mean = KN.gmm_logprob(e_d, pi, mu, sigma, want_mean=True, denom=denom)
    return {"pi": pi, "mu": mu, "sigma": sigma, "sigma_pre": pre, "logp": logp, "resp": resp,
            "mean": mean, "meta": meta_d, "e": e_d}


def run_bwd(k, g, prefill):
    """gmm_head_bwd on the kernels' own forward tensors, into clones of ``prefill``."""
    bufs = [p.to(DEV).clone() for p in prefill]
    KN.gmm_head_bwd(k["meta"], k["e"], k["pi"], k["mu"], k["sigma"], k["sigma_pre"], k["resp"],
                    g.to(DEV).contiguous(), bufs)
    torch.cuda.synchronize()
    return bufs


def make_prefill(ref, seed, elementwise=False):
    """Non-zero float32 contents of the gradient buffers, of the gradients' own magnitude (so
    the 1e-4-of-scale bound on pre-fill + gradient is not loosened by a large pre-fill);
    ``elementwise`` scales each entry by its own gradient."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in GRADS:
        r = ref[n]
        u = torch.randn(r.shape, generator=gen, dtype=torch.float64)
        s = r.abs() if elementwise else (r.abs().max().item() or 1.0) * 0.5
        out.append((u * s).float())
    return out


# (B, in_dim, K, D): the smallest shapes that reach each written-out branch
SHAPES = {
    "shipped":   (4, 5, 3, 256),   # the shipped layout: 2KD = 1536 = 24 full blocks, one pi chunk
    "minimum":   (1, 1, 1, 1),     # K = 1: its single probability clamps to 1 - eps; one active lane
    "straddle":  (7, 8, 16, 5),    # KD = 80: block 1 holds mu and sigma outputs; 2KD = 160: last block
                                   # has 32 idle lanes (`act` false); B = 7 < 8 waves; in_dim, K at bounds
    "kd300":     (9, 3, 3, 100),   # KD = 300: not a multiple of 64, boundary and tail mid-block
    "chunks3":   (33, 2, 16, 8),   # CH = 256 / 16 = 16: pi chunks of 16, 16 and 1 rows
    "chunks2":   (86, 4, 3, 4),    # CH = 85: a second pi chunk of one row
    "d300":      (5, 2, 2, 300),   # D > 256: a second trip of the log-prob thread loop
    "d257":      (5, 2, 2, 257),   # ... whose second trip is one element
}
_CASES = {}


def case(name):
    """Inputs, float64 reference and kernel outputs of a shape; computed once."""
    if name not in _CASES:
        B, I, K, D = SHAPES[name]
        meta, W, e, g = make_inputs(B, I, K, D, seed=100 + len(name) + B)
        ref = ref_head(meta, W, e, K, D, g_logp=g)
        got = run_head(meta, W, e, K, D)
        torch.cuda.synchronize()
        _CASES[name] = {"in": (meta, W, e, g), "ref": ref, "got": got}
    return _CASES[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_head_fwd(name):
    """gmm_head_fwd: pi (thread 0's softmax over K), mu / sigma / sigma_pre (the KD loop of
    256 threads: one trip at KD <= 256, ragged trips at 300, 600, 768) at every in_dim."""
    c = case(name)
    for k in ("pi", "mu", "sigma", "sigma_pre"):
        close(c["got"][k], c["ref"][k], 1e-5, f"{name}.{k}")
    close(c["got"]["pi"].sum(1), torch.ones(SHAPES[name][0]), 1e-5, f"{name}.pi rows")


@pytest.mark.parametrize("name", list(SHAPES))
def test_logprob_and_resp(name):
    """gmm_logprob: per-component sums over D (one trip of the 256-thread loop, or two at
    D = 300 / 257), log_mix, logsumexp, responsibilities; K = 1 (resp = 1) to K = 16."""
    c = case(name)
    close(c["got"]["logp"], c["ref"]["logp"], 1e-5, f"{name}.logp")
    close(c["got"]["resp"], c["ref"]["resp"], 0.0, f"{name}.resp", floor=1e-5)
    close(c["got"]["resp"].sum(1), torch.ones(SHAPES[name][0]), 0.0, f"{name}.resp rows", floor=1e-5)
    r = c["ref"]["resp"]
    if SHAPES[name][2] > 1:  # the inputs do exercise the mixture: not every row is one-hot
        assert (r.max(1).values < 0.99).any(), "responsibilities are one-hot: inputs too easy"


@pytest.mark.parametrize("name", list(SHAPES))
def test_mean_denominators(name):
    """mean_k: sum_b logp_b / B without ``denom``, / denom[0] with one that is not B (the
    data-parallel global batch).  Against the float64 reference at 1e-5 of scale, and against
    the kernel's own logp at the bound of an in-order float32 sum: (B - 1) roundings of at
    most 2^-24 * sum|logp| each, plus one for the division."""
    c = case(name)
    meta, W, e, _ = c["in"]
    B, _, K, D = SHAPES[name]
    ref_sum = c["ref"]["logp"].sum()
    close(c["got"]["mean"], ref_sum / B, 1e-5, f"{name}.mean")
    den = torch.tensor([2.0 * B + 3.0], device=DEV)
    got = run_head(meta, W, e, K, D, denom=den)
    assert torch.equal(got["logp"], c["got"]["logp"])
    close(got["mean"], ref_sum / (2.0 * B + 3.0), 1e-5, f"{name}.mean/denom")
    own = got["logp"].double().cpu()
    bound = B * 2.0 ** -24 * own.abs().sum().item()
    for mean, d in ((c["got"]["mean"], float(B)), (got["mean"], 2.0 * B + 3.0)):
        assert abs(mean.double().item() * d - own.sum().item()) <= bound


def test_fill_from_denominator():
    """fs2_fill_from, the backward's d mean / d logp_b: g * scale without ``den`` and
    g * scale / den[0] with it, in every element (n = 300: two blocks); two float32 roundings,
    so 3e-7 relative."""
    g = torch.tensor(0.7531, device=DEV)
    den = torch.tensor([96.0], device=DEV)
    out = torch.full((300,), float("nan"), device=DEV)
    KN.lib.fs2_fill_from(KN.ptr(out), 300, KN.ptr(g), 1.0, KN.ptr(den), KN.stream())
    np.testing.assert_allclose(out.cpu().numpy(), np.full(300, 0.7531 / 96.0), rtol=3e-7)
    KN.lib.fs2_fill_from(KN.ptr(out), 300, KN.ptr(g), 1.0 / 48, None, KN.stream())
    np.testing.assert_allclose(out.cpu().numpy(), np.full(300, 0.7531 / 48.0), rtol=3e-7)


@pytest.mark.parametrize("name", list(SHAPES))
def test_head_bwd_accumulates(name):
    """gmm_head_bwd with a non-uniform g_logp into buffers pre-filled with random values:
    pre-fill + float64 autograd gradient, which pins the ``+=`` of all six outputs.  Shapes:
    see SHAPES (mu/sigma boundary inside a block, idle lanes of the last block, fewer rows than
    the 8 waves, one to three pi chunks, in_dim 1..8, K 1..16)."""
    c = case(name)
    pre = make_prefill(c["ref"], seed=7)
    got = run_bwd(c["got"], c["in"][3], pre)
    for n, buf, p in zip(GRADS, got, pre):
        close(buf, p.double() + c["ref"][n], 1e-4, f"{name}.{n}")
    if SHAPES[name][2] == 1:  # K = 1: log_mix is constant, the pi head gets no gradient
        assert torch.equal(got[0].cpu(), pre[0]) and torch.equal(got[1].cpu(), pre[1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_head_bwd_deterministic(name):
    """"Deterministic throughout": two calls from the same pre-fill agree bitwise."""
    c = case(name)
    pre = make_prefill(c["ref"], seed=8)
    a, b = run_bwd(c["got"], c["in"][3], pre), run_bwd(c["got"], c["in"][3], pre)
    for n, x, y in zip(GRADS, a, b):
        assert torch.equal(x, y), n


# ------------------------------------------------------------------ edge inputs, (6, 3, 4, 16)
EB, EI, EK, ED = 6, 3, 4, 16


def _edge_e(meta, W, spread, seed):
    """e at ``spread`` * (the smallest sigma of the column) from the components' mean."""
    ref = ref_head(meta, W, torch.zeros(EB, ED), EK, ED)
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(EB, ED, generator=gen, dtype=torch.float64)
    return (ref["mu"].mean(1) + spread * ref["sigma"].min(1).values * u).float()


def test_clamped_pi():
    """The probability clamp of ``log_mix`` and its zero-gradient branch in ``gmm_pi_gz``.
    The pi logits are [m0, m1, m2, 0] (identity weights), so the rows are: 0, 4 ordinary;
    1, 5 fully clamped (the dominant probability to 1 - eps, the others up to eps); 2 with one
    and 3 with two entries clamped up to eps beside unclamped ones.  The clamp's gradient is
    discontinuous at its bounds, so the float64 probabilities must stay away from them: none
    in [1e-9, 1e-5], none in [1 - 1e-5, 1) unless it clamps (asserted below).  Gradients
    through clamped entries are zero: the float64 autograd has that, and a g_logp that is
    non-zero only on the fully clamped rows must leave dw_pi / db_pi bitwise untouched."""
    gen = torch.Generator().manual_seed(21)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    meta = torch.tensor([[0.3, -0.2, 0.5], [30.0, 0.0, -30.0], [2.0, 1.0, -25.0],
                         [-28.0, -26.0, 1.0], [0.5, 0.1, -0.4], [-40.0, 35.0, -40.0]])
    w_pi = torch.zeros(EK, EI)
    w_pi[:3] = torch.eye(3)
    W = [w_pi, torch.zeros(EK), r(EK * ED, EI) * 0.01, -0.5 + 0.2 * r(EK * ED),
         r(EK * ED, EI) * 0.005, r(EK * ED) * 0.1]
    e = _edge_e(meta, W, 0.5, 22)
    g = 1.0 + 0.5 * r(EB)
    ref = ref_head(meta, W, e, EK, ED, g_logp=g)
    p = ref["probs"]
    assert not ((p >= 1e-9) & (p <= 1e-5)).any()
    assert not ((p >= 1 - 1e-5) & (p < 1 - EPS32)).any()
    low, high = p < EPS32, p > 1 - EPS32
    assert low.sum(1).tolist() == [0, 3, 1, 2, 0, 3] and high.sum(1).tolist() == [0, 1, 0, 0, 0, 1]
    got = run_head(meta, W, e, EK, ED)
    for k in ("pi", "mu", "sigma"):
        close(got[k], ref[k], 1e-5, f"clamp.{k}")
    close(got["logp"], ref["logp"], 1e-5, "clamp.logp")
    close(got["resp"], ref["resp"], 0.0, "clamp.resp", floor=1e-5)
    pre = make_prefill(ref, seed=23)
    out = run_bwd(got, g, pre)
    for n, buf, q in zip(GRADS, out, pre):
        close(buf, q.double() + ref[n], 1e-4, f"clamp.{n}")
    assert ref["dw_pi"].abs().max() > 0  # rows 0, 2, 3, 4 do carry a pi gradient
    g_cl = torch.tensor([0.0, 1.3, 0.0, 0.0, 0.0, -0.7])
    ref_cl = ref_head(meta, W, e, EK, ED, g_logp=g_cl)
    assert ref_cl["dw_pi"].abs().max() == 0 and ref_cl["db_pi"].abs().max() == 0
    out = run_bwd(got, g_cl, pre)
    assert torch.equal(out[0].cpu(), pre[0]) and torch.equal(out[1].cpu(), pre[1])
    for n, buf, q in list(zip(GRADS, out, pre))[2:]:
        close(buf, q.double() + ref_cl[n], 1e-4, f"clamp.rows15.{n}")


def test_sigma_pre_range():
    """sigma_pre from -6 to 25 (bias ramp, tiny weights): both arms of softplus (x > 20 -> x)
    and of its derivative (x > 20 -> 1).  Not below -6: sigma^-3 overflows float32 near -8 in
    the reference model too.

    sigma spans 2.5e-3 .. 25 and the gradients 1 / sigma of that, so a bound at the scale of
    the largest entry would not see the x > 20 arm at all.  Hence, besides the project's
    bounds: sigma elementwise to 1e-5 relative (sigma_pre carries at most in_dim + 1 = 4
    roundings of ulp(25) / 2 = 9.5e-7, i.e. 4e-6 absolute at the top, where d sigma / d x <= 1,
    and 4 * 2.4e-7 at x = -6, relative to sigma 4e-6 after expf and log1pf at 2 ulp each),
    and the sigma head's gradients by arm: the x > 20 outputs and the others each at 1e-4 of
    their own scale, from a pre-fill scaled element by element."""
    gen = torch.Generator().manual_seed(31)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    meta = r(EB, EI)
    ramp = torch.linspace(-6.0, 25.0, EK * ED)[torch.randperm(EK * ED, generator=gen)]
    W = [r(EK, EI) * 0.5, r(EK) * 0.5, r(EK * ED, EI) * 0.001, ramp, r(EK * ED, EI) * 0.001,
         r(EK * ED) * 0.001]
    e = _edge_e(meta, W, 0.7, 32)
    g = 1.0 + 0.5 * r(EB)
    ref = ref_head(meta, W, e, EK, ED, g_logp=g)
    x = ref["sigma_pre"]
    assert x.min() < -5.9 and x.max() > 24.9 and (x > 20).sum() >= EB * 5
    assert ((x > 19) & (x <= 20)).any() and ((x > 20) & (x < 21)).any()  # both sides of the arm
    got = run_head(meta, W, e, EK, ED)
    for k in ("pi", "mu", "sigma", "sigma_pre"):
        close(got[k], ref[k], 1e-5, f"range.{k}")
    rel = ((got["sigma"].double().cpu() - ref["sigma"]) / ref["sigma"]).abs().max().item()
    print(f"range.sigma: max relative err {rel:.3e}")
    assert rel <= 1e-5
    close(got["logp"], ref["logp"], 1e-5, "range.logp")
    close(got["resp"], ref["resp"], 0.0, "range.resp", floor=1e-5)
    pre = make_prefill(ref, seed=33, elementwise=True)
    out = dict(zip(GRADS, run_bwd(got, g, pre)))
    want = {n: q.double() + ref[n] for n, q in zip(GRADS, pre)}
    for n in GRADS:
        close(out[n], want[n], 1e-4, f"range.{n}")
    hi = W[3] > 20.5  # outputs whose sigma_pre is above 20 in every row (weights 0.001)
    assert (x.view(EB, -1)[:, hi] > 20).all() and (x.view(EB, -1)[:, ~hi & (W[3] < 19.5)] < 20).all()
    for n in ("dw_s", "db_s"):
        close(out[n].cpu()[hi], want[n][hi], 1e-4, f"range.{n}[x > 20]")
        close(out[n].cpu()[~hi], want[n][~hi], 1e-4, f"range.{n}[x <= 20]")


def test_small_sigma():
    """sigma ~ 1e-2 with |e - mu| ~ 1: every term of a component's log-density is ~ -5e3 and
    the gradients carry sigma^-2 and sigma^-3, so float32 cancellation is at its worst; the
    components are near-copies, so ``resp`` and every gradient depend on differences of O(1)
    between sums of ~ -1e5.  The project's bounds (1e-5 / 1e-4 of scale, 1e-5 absolute for
    resp) cannot all be met by float32 arithmetic here.  Each tensor's bound is therefore the
    project's or, where that is larger, 4 x the error of the same formula evaluated in float32
    torch on the CPU against the float64 reference (the kernel's summation order differs from
    torch's); nothing is derived from the kernel's output.  The test measures the float32
    error itself; on the development machine (x86-64, torch CPU) it was

        tensor   float32 error   scale     project bound   bound used
        logp     2.6e-02         1.0e+05   1.0e+00         1.0e+00 (project's)
        resp     2.9e-03         1         1.0e-05         1.2e-02
        dw_pi    4.7e-03         8.4e-01   8.4e-05         1.9e-02
        db_pi    3.5e-03         1.6e+00   1.6e-04         1.4e-02
        dw_s     1.1e+02         5.6e+04   5.6e+00         4.3e+02
        db_s     8.3e+01         6.5e+04   6.5e+00         3.3e+02
        dw_mu    1.3e+02         4.6e+04   4.6e+00         5.1e+02
        db_mu    1.3e+02         3.8e+04   3.8e+00         5.2e+02
    """
    gen = torch.Generator().manual_seed(41)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    meta = r(EB, EI)
    # the four components share sigma and differ in mu by ~2e-5 only: their log-densities,
    # ~ -1e5 each, then differ by O(1), and resp hangs on the last bits of the float32 sums
    W = [r(EK, EI) * 0.5, r(EK) * 0.5, (r(ED, EI) * 0.05).repeat(EK, 1),
         (-4.6 + 0.1 * r(ED)).repeat(EK), (r(ED, EI) * 0.002).repeat(EK, 1),
         (r(ED) * 0.002).repeat(EK) + 2e-5 * r(EK * ED)]
    ref0 = ref_head(meta, W, torch.zeros(EB, ED), EK, ED)
    sign = torch.where(torch.rand(EB, ED, generator=gen) < 0.5, -1.0, 1.0)
    e = (ref0["mu"].mean(1) + sign * (1.0 + 0.1 * torch.rand(EB, ED, generator=gen))).float()
    g = 1.0 + 0.5 * r(EB)
    ref = ref_head(meta, W, e, EK, ED, g_logp=g)
    assert 5e-3 < ref["sigma"].min() and ref["sigma"].max() < 2e-2
    f32 = ref_head(meta, W, e, EK, ED, g_logp=g, dtype=torch.float32)
    err32 = {k: (f32[k].double() - ref[k]).abs().max().item() for k in ("logp", "resp") + GRADS}
    print("small_sigma float32-torch error:", {k: f"{v:.2e}" for k, v in err32.items()})
    assert (ref["resp"].max(1).values < 0.9).sum() >= 3  # resp is not one-hot
    got = run_head(meta, W, e, EK, ED)
    for k in ("pi", "mu", "sigma"):
        close(got[k], ref[k], 1e-5, f"small.{k}")
    close(got["logp"], ref["logp"], 1e-5, "small.logp", floor=4 * err32["logp"])
    close(got["resp"], ref["resp"], 0.0, "small.resp", floor=max(1e-5, 4 * err32["resp"]))
    pre = make_prefill(ref, seed=43)
    for n, buf, q in zip(GRADS, run_bwd(got, g, pre), pre):
        close(buf, q.double() + ref[n], 1e-4, f"small.{n}", floor=4 * err32[n])


# ------------------------------------------------------------------ refusals
def test_refusals():
    """FS2_CHECK_ARG failures surface as KernelError before any launch: K = 17 and
    in_dim = 9 for gmm_head_fwd / gmm_head_bwd, K = 17 for gmm_logprob (the kernels' stack
    arrays hold 16 components and the backward unrolls to 8 inputs).  Every buffer has the
    size the call describes."""
    def head(B, I, K, D):
        z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        return z(B, I), [z(K, I), z(K), z(K * D, I), z(K * D), z(K * D, I), z(K * D)]

    for I, K in ((3, 17), (9, 4)):
        B, D = 2, 4
        meta, W = head(B, I, K, D)
        with pytest.raises(KernelError):
            KN.gmm_head_fwd(meta, *W, K, D)
        o = lambda *s: torch.ones(*s, device=DEV)  # noqa: E731
        with pytest.raises(KernelError):
            KN.gmm_head_bwd(meta, o(B, D), o(B, K) / K, o(B, K, D), o(B, K, D), o(B, K, D),
                            o(B, K) / K, o(B), [torch.zeros_like(w) for w in W])
    o = lambda *s: torch.ones(*s, device=DEV)  # noqa: E731
    with pytest.raises(KernelError):
        KN.gmm_logprob(o(2, 4), o(2, 17) / 17, o(2, 17, 4), o(2, 17, 4))
    KN.gmm_logprob(o(2, 4), o(2, 16) / 16, o(2, 16, 4), o(2, 16, 4))  # the bound itself is accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------ gmm_sample
def _mixture(B, K, D, seed, sigma=None):
    gen = torch.Generator().manual_seed(seed)
    pi = torch.rand(B, K, generator=gen) + 0.05
    mu = torch.randn(B, K, D, generator=gen) * 3
    sg = torch.full((B, K, D), float(sigma)) if sigma is not None else torch.rand(B, K, D, generator=gen) + 0.1
    return (pi / pi.sum(1, keepdim=True)).to(DEV), mu.to(DEV), sg.to(DEV)


def test_sample_ties_comp_to_out():
    """sigma = 0: out[b] is mu[b, comp[b]] bitwise (so ``comp`` is the component ``out`` was
    drawn from) and comp lies in [0, K); B * D = 1330 elements, six blocks, D odd."""
    B, K, D = 190, 5, 7
    pi, mu, sg = _mixture(B, K, D, 1, sigma=0.0)
    out, comp = KN.gmm_sample(pi, mu, sg, 1234, 5)
    comp = comp.long()
    assert comp.min() >= 0 and comp.max() < K
    assert len(comp.unique()) > 1
    assert torch.equal(out, mu[torch.arange(B, device=DEV), comp])


def test_sample_single_component():
    """K = 1 always picks component 0, whatever the (unnormalised) weight."""
    B, D = 70, 3
    pi = torch.full((B, 1), 0.3, device=DEV)
    _, mu, sg = _mixture(B, 1, D, 2, sigma=0.0)
    out, comp = KN.gmm_sample(pi, mu, sg, 99)
    assert torch.equal(comp, torch.zeros_like(comp)) and torch.equal(out, mu[:, 0])


def test_sample_is_a_function_of_seed_and_offset():
    """The same (seed, offset) twice is bitwise equal; another seed, or another offset, gives
    another draw (offset and offset + 1 feed the component and the noise streams, so offset
    + 1 and offset + 2 are both tried)."""
    pi, mu, sg = _mixture(40, 4, 9, 3)
    a, ca = KN.gmm_sample(pi, mu, sg, 7, 11)
    b, cb = KN.gmm_sample(pi, mu, sg, 7, 11)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    for seed, off in ((8, 11), (7, 12), (7, 13), (7 + 2 ** 40, 11), (7, 11 + 2 ** 40)):
        c, _ = KN.gmm_sample(pi, mu, sg, seed, off)
        assert (c != a).float().mean() > 0.9, (seed, off)


def test_sample_batch_invariance():
    """Row b depends only on (b, seed, offset) and its own parameters: rows 0..4 of a B = 50
    call equal a B = 5 call on the first five rows, bitwise (synthesis draws one speaker the
    same whatever else is in the batch)."""
    pi, mu, sg = _mixture(50, 3, 6, 4)
    big, cbig = KN.gmm_sample(pi, mu, sg, 31337, 2)
    small, csmall = KN.gmm_sample(pi[:5].contiguous(), mu[:5].contiguous(), sg[:5].contiguous(),
                                  31337, 2)
    assert torch.equal(big[:5], small) and torch.equal(cbig[:5], csmall)


def test_sample_unnormalised_pi():
    """pi rows that sum to 2.5 with distinct ratios, a zero-probability component in the
    middle and one at the end; B = 20000 independent rows, fixed seed.  Each component's count
    is Binomial(B, p_k), p = pi / sum, so its frequency lies within 5 standard deviations
    sqrt(p (1 - p) / B) of p_k except with probability 6e-7 per component; the zero-probability
    components are never drawn (u < sum always ends the walk before the trailing one)."""
    B, D = 20000, 2
    w = torch.tensor([0.25, 0.5, 0.0, 0.75, 1.0, 0.0])
    K = w.numel()
    assert w.sum().item() == 2.5
    pi = w.repeat(B, 1).to(DEV)
    mu = torch.arange(K, dtype=torch.float32).view(1, K, 1).expand(B, K, D).contiguous().to(DEV)
    out, comp = KN.gmm_sample(pi, mu, torch.zeros(B, K, D, device=DEV), 2024, 0)
    assert torch.equal(out[:, 0], comp.float()) and torch.equal(out[:, 1], comp.float())
    freq = torch.bincount(comp.long().cpu(), minlength=K).double() / B
    p = (w / w.sum()).double()
    sd = torch.sqrt(p * (1 - p) / B)
    print("freq", freq.tolist(), "p", p.tolist(), "5 sd", (5 * sd).tolist())
    assert freq[2] == 0 and freq[5] == 0
    assert ((freq - p).abs() <= 5 * sd).all()
