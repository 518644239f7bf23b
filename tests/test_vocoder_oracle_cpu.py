"""The vocoder kernels' oracle (tests/vocoder_oracle.py) checked without a GPU: against the
generator restatement that g9 pins to the reference, the exact-lattice condition its bitwise
GPU comparisons rest on, and the int16 rule at its edges."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocoder_oracle as VO
from oracle import hifigan_cpu


def test_oracle_slices_match_generator_forward():
    """With the bf16 roundings off, resblock1 (three kernel sizes folded into the running
    average) and conv_post reproduce generator_forward on a one-stage generator."""
    g = torch.Generator().manual_seed(11)
    C, B, T, ks, dils = 32, 2, 24, (3, 7, 11), ((1, 3, 5), (2, 1, 4), (1, 3, 5))
    h = {"upsample_rates": [2], "upsample_kernel_sizes": [4], "resblock_kernel_sizes": list(ks),
         "resblock_dilation_sizes": [list(d) for d in dils]}
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    sd = {"conv_pre.weight": rn(2 * C, 80, 7, scale=1 / math.sqrt(560)), "conv_pre.bias": rn(2 * C, scale=0.1),
          "ups.0.weight": rn(2 * C, C, 4, scale=1 / math.sqrt(4 * C)), "ups.0.bias": rn(C, scale=0.1),
          "conv_post.weight": rn(1, C, 7, scale=1 / math.sqrt(7 * C)), "conv_post.bias": rn(1, scale=0.1)}
    for j, k in enumerate(ks):
        for name in ("convs1", "convs2"):
            for m in range(3):
                sd[f"resblocks.{j}.{name}.{m}.weight"] = rn(C, C, k, scale=1 / math.sqrt(C * k))
                sd[f"resblocks.{j}.{name}.{m}.bias"] = rn(C, scale=0.1)
    mel = rn(B, 80, T)
    want = hifigan_cpu.generator_forward(sd, h, mel).reshape(-1)

    x = F.conv1d(mel, sd["conv_pre.weight"], sd["conv_pre.bias"], padding=3)
    x = F.conv_transpose1d(F.leaky_relu(x, 0.1), sd["ups.0.weight"], sd["ups.0.bias"], stride=2,
                           padding=1)
    T2 = 2 * T
    rows = x.transpose(1, 2).reshape(B * T2, C)
    xs, hc = None, None
    for j, (k, dil) in enumerate(zip(ks, dils)):
        P = lambda name, what: [sd[f"resblocks.{j}.{name}.{m}.{what}"] for m in range(3)]
        fin = j == len(ks) - 1
        xs, hc = VO.resblock1(rows, P("convs1", "weight"), P("convs2", "weight"),
                              P("convs1", "bias"), P("convs2", "bias"), k, dil, T=T2, acc_in=xs,
                              scale=1 / 3 if fin else 1.0, alpha2=0.01 if fin else None,
                              dtype=torch.float32, bf16=False)
    wav, _, _ = VO.conv_post(hc, sd["conv_post.weight"], sd["conv_post.bias"], T=T2,
                             max_wav=32768.0)
    # the tolerance test_oracle_matches_reference allows the same CPU convs
    np.testing.assert_allclose(wav.numpy(), want.double().numpy(), rtol=0, atol=1e-4)


@pytest.mark.parametrize("case", VO.lattice_cases(), ids=str)
def test_lattice_sums_are_exact(case):
    """Every lattice case of the GPU tests: the emulation with fp32 and with fp64 conv
    accumulation agree bitwise, every conv's sum of magnitudes spans at most 22 bits above the
    lowest bit a product can set (two bits below fp32's 24), and the bf16 rounding points
    really round (almost no output is bf16-exact)."""
    C, B, T, k, dil = case
    x, w1, w2, b1, b2 = VO.lattice_for(case)
    spans = []
    v64, h64 = VO.resblock1(x, w1, w2, b1, b2, k, dil, T=T, alpha2=0.1, dtype=torch.float64,
                            spans=spans)
    v32, h32 = VO.resblock1(x, w1, w2, b1, b2, k, dil, T=T, alpha2=0.1, dtype=torch.float32)
    assert torch.equal(v64, v32) and torch.equal(h64, h32)
    assert len(spans) == 6 and max(spans) <= 2 ** 22, math.log2(max(spans))
    assert (v64.to(torch.bfloat16).float() == v64).float().mean().item() < 1e-3
    assert v64.unique().numel() > 10000


PCM_CASES = {
    # wav: (pcm at max_wav 32768, at 32767)
    1.0: (-32768, 32767),               # 32768 wraps in 16 bits
    -1.0: (-32768, -32767),
    1.0 - 2.0 ** -24: (32767, 32766),   # 32767 * (1 - 2^-24) rounds to 32767 - 2^-9 in fp32
    -(1.0 - 2.0 ** -24): (-32767, -32766),
    0.99996: (32766, 32765),
    -0.99996: (-32766, -32765),
    1e-6: (0, 0),
    -1e-6: (0, 0),                      # toward zero, not floor
    0.0: (0, 0),
}


def test_pcm_of_edges():
    wav = np.array(list(PCM_CASES), dtype=np.float32)
    assert wav[2] < 1.0 and wav[2] == np.nextafter(np.float32(1), np.float32(0))
    for col, max_wav in enumerate((32768.0, 32767.0)):
        got = VO.pcm_of(wav, max_wav)
        assert got.dtype == np.int16
        assert got.tolist() == [v[col] for v in PCM_CASES.values()], max_wav
        # the same rule in Python integers: exact product (24 + 16 bits fit a double), one
        # rounding to fp32, int() truncation, two's-complement wrap
        for w, p in zip(wav, got):
            i = int(np.float32(float(w) * max_wav))
            assert p == (i + 32768) % 65536 - 32768
