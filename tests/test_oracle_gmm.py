"""The ``eps`` argument of the oracle mixture (``fs2_cpu.GMMParams.log_prob``), on the CPU.

The GMM kernels clamp mixture probabilities at float32 eps as the float32 reference model
does; a float64 evaluation of the oracle is a reference for them only if it keeps that clamp
instead of moving it to float64's 2.2e-16.  tests/test_gpu_gmm.py relies on this."""
import numpy as np
import torch
import torch.distributions as TD

from conftest import load_golden
from oracle import fs2_cpu

EPS32 = float(torch.finfo(torch.float32).eps)


def test_float64_log_prob_with_float32_eps_reproduces_golden():
    """Float64 arithmetic on the captured float32 pi / mu / sigma / e, float32 clamp: the
    reference's own float32 ``log_prob`` to 1e-6 relative."""
    g = load_golden("g4_ops.npz")
    pi, mu, sigma, e = (torch.from_numpy(g[f"gmm.{k}"]).double() for k in ("pi", "mu", "sigma", "e"))
    lp = fs2_cpu.GMMParams(pi, mu, sigma).log_prob(e, eps=EPS32)
    assert lp.dtype == torch.float64
    np.testing.assert_allclose(lp.numpy(), g["gmm.logp"], rtol=1e-6)


def test_default_eps_is_the_dtype_eps():
    """``eps=None`` keeps the old behaviour: the clamp of the tensors' own dtype."""
    gen = torch.Generator().manual_seed(3)
    pi = torch.tensor([[0.0, 0.5, 0.25, 0.25]])
    mu, sigma = torch.randn(1, 4, 8, generator=gen) * 10, torch.rand(1, 4, 8, generator=gen) + 0.5
    e = mu[:, 0] + 0.1  # on the zero-probability component, so the clamp decides logp
    for dt in (torch.float32, torch.float64):
        p = fs2_cpu.GMMParams(pi.to(dt), mu.to(dt), sigma.to(dt))
        assert torch.equal(p.log_prob(e.to(dt)), p.log_prob(e.to(dt), eps=torch.finfo(dt).eps))
    p64 = fs2_cpu.GMMParams(pi.double(), mu.double(), sigma.double())
    assert not torch.allclose(p64.log_prob(e.double()), p64.log_prob(e.double(), eps=EPS32),
                              rtol=1e-3, atol=0)


def test_clamped_case_equals_mixture_same_family():
    """K = 4 with one pi entry of 0 (clamped up to eps) against torch.distributions in
    float32, with and without the explicit float32 eps; rows 1.. put e on the zero-probability
    component so that the clamped term carries the result."""
    gen = torch.Generator().manual_seed(11)
    B, K, D = 5, 4, 6
    pi = torch.rand(B, K, generator=gen) + 0.1
    pi[:, 2] = 0.0
    pi = pi / pi.sum(-1, keepdim=True)
    mu = torch.randn(B, K, D, generator=gen) * 3
    sigma = torch.rand(B, K, D, generator=gen) * 0.5 + 0.2
    e = mu[:, 1] + 0.1 * torch.randn(B, D, generator=gen)
    e[1:] = mu[1:, 2] + 0.05
    want = TD.MixtureSameFamily(TD.Categorical(pi),
                                TD.Independent(TD.Normal(mu, sigma), 1)).log_prob(e)
    p = fs2_cpu.GMMParams(pi, mu, sigma)
    np.testing.assert_allclose(p.log_prob(e).numpy(), want.numpy(), rtol=1e-6)
    np.testing.assert_allclose(p.log_prob(e, eps=EPS32).numpy(), want.numpy(), rtol=1e-6)
    # and the float64 evaluation with the float32 clamp agrees with it, which the float64
    # clamp does not (log(2.2e-16) instead of log(1.2e-7) on the rows the clamp carries)
    p64 = fs2_cpu.GMMParams(pi.double(), mu.double(), sigma.double())
    np.testing.assert_allclose(p64.log_prob(e.double(), eps=EPS32).numpy(), want.numpy(), rtol=1e-5)
    assert (p64.log_prob(e.double())[1:] - want[1:].double()).abs().min() > 10
