"""The vocoder's hand-written kernels, each against a plain CPU reference
(tests/vocoder_oracle.py, itself checked by tests/test_vocoder_oracle_cpu.py):

* fs2_resblock1_fused on exact-lattice inputs -- every fp32 partial sum is representable, so
  the summation order cannot matter and xs / hc are compared BITWISE with the oracle -- over
  every tap count, the 64-row receptive limit, one-tile utterances, the epilogue modes, the
  persistent tile loop, the lens skip and the per-conv path; a signed case measured against
  the fp32 emulation's own error; the refusals;
* fs2_vocoder_post against fp64 within the fp32 dot product's bound, its int16 rule, lens
  and blocks that span utterances;
* fs2_conv_gemm_ex with lens / FS2_EPI_SKIP_NOSTORE at the vocoder's shapes.

"Not written" is asserted against a finite sentinel (-777 and its bf16 image)."""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import vocoder_oracle as VO

pytestmark = pytest.mark.gpu
K = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
DEV = "cuda"
SENT = -777.0
BF = torch.bfloat16
ERR_ARG, ERR_DTYPE = -1, -3  # include/fs2hip.h


def sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def assert_bitwise(got, want, what):
    """Bitwise equality of two 2-D tensors; a failure names the rows and channels, since a
    structural bug is localized and a summation-order effect is not."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if torch.equal(g, w):
        return
    bad = g != w
    rows = bad.any(1).nonzero().flatten().tolist()
    chans = bad.any(0).nonzero().flatten().tolist()
    diff = (got.detach().cpu().double() - want.detach().cpu().double()).abs().max().item()
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in {len(rows)} rows "
        f"(first {rows[:6]}, last {rows[-3:]}) and {len(chans)} channels (first {chans[:6]}); "
        f"max |diff| {diff:.3e}")


def prep(w, dtype=BF):
    """(c_out, c_in, k) fp32 conv weight -> the compute layout fs2_conv_weight_prep writes."""
    c_out, c_in, k = w.shape
    wf = torch.empty(c_out * c_in * k, dtype=dtype, device=DEV)
    K.weight_prep(w.to(DEV).contiguous(), c_out, c_in, k, w_fwd=wf)
    return wf


def prior(rows, C, seed):
    """Earlier contents of xs on the lattice (integers in [1, 8])."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 9, (rows, C), generator=g).float()


# ------------------------------------------------------------------ fs2_resblock1_fused
class Block:
    """One ResBlock1 problem: CPU tensors for the oracle, device tensors for the kernel."""

    def __init__(self, case, tensors):
        self.case = case
        self.C, self.B, self.T, self.k, self.dil = case
        self.rows = self.B * self.T
        self.cpu = tensors
        x, w1, w2, b1, b2 = tensors
        self.x = x.to(DEV)
        self.w1, self.w2 = [prep(w) for w in w1], [prep(w) for w in w2]
        self.b1, self.b2 = [b.to(DEV) for b in b1], [b.to(DEV) for b in b2]

    def oracle(self, **kw):
        x, w1, w2, b1, b2 = self.cpu
        return VO.resblock1(x, w1, w2, b1, b2, self.k, self.dil, T=self.T, **kw)

    def fused(self, xs, acc=0, scale=1.0, store_xs=1, hc=None, alpha2=0.1, lens=None):
        rc = K.resblock1_fused(self.x, self.rows, self.T, self.C, self.k, self.dil, self.w1,
                               self.w2, self.b1, self.b2, xs, acc, scale, store_xs, hc, alpha2,
                               lens)
        torch.cuda.synchronize()
        return rc


@functools.lru_cache(maxsize=None)
def lattice_block(case):
    return Block(case, VO.lattice_for(case))


@functools.lru_cache(maxsize=None)
def lattice_ref(case):
    """(out, hc) of the plain block on the lattice: acc 0, scale 1; computed once."""
    return lattice_block(case).oracle(alpha2=0.1)


R_ = VO.tile_rows
STORE_CASES = (
    [(32, 2, 512, k, (1, 3, 5)) for k in (3, 5, 7, 9, 11)] +      # two tiles per utterance
    [(64, 3, 256, k, (1, 3, 5)) for k in (3, 5, 7, 9, 11)] +
    [(C, 2, 2 * R_(C), k, d) for C in (32, 64)                    # radius 64, 64, non-monotone
     for k, d in ((9, (1, 5, 7)), (3, (21, 20, 20)), (5, (5, 1, 3)))] +
    [(C, 4, R_(C), 11, (1, 3, 5)) for C in (32, 64)])              # one tile per utterance


@pytest.mark.parametrize("case", STORE_CASES, ids=str)
def test_resblock1_lattice_bitwise(case):
    """Every tap instantiation at both widths (a start edge, an interior seam, an end edge and
    a neighbouring utterance that must not leak), the full 64-row halo (k=9 (1,5,7) and k=3
    (21,20,20) both have radius 64), a non-monotone dilation order, and utterances of one
    tile: xs and hc bitwise equal to the oracle."""
    assert case in VO.lattice_cases()  # its exactness is asserted on the CPU
    blk = lattice_block(case)
    assert K.resblock1_supported(blk.C, blk.T, blk.k, blk.dil)
    xs, hc = sent(blk.rows, blk.C), sent(blk.rows, blk.C, dtype=BF)
    blk.fused(xs, hc=hc, alpha2=0.1)
    want_v, want_hc = lattice_ref(case)
    assert_bitwise(xs, want_v, f"xs {case}")
    assert_bitwise(hc, want_hc, f"hc {case}")


@pytest.mark.parametrize("C", [32, 64])
def test_resblock1_epilogue_modes(C):
    """(acc, scale, store_xs, hc, alpha2) in every combination the generator uses: each branch
    of the final store, xs untouched when store_xs = 0, xs + out read before it is written."""
    case = (C, 2, 2 * R_(C), 7, (1, 3, 5))
    assert case in VO.lattice_cases()
    blk = lattice_block(case)
    old = prior(blk.rows, C, seed=5)
    for acc, scale, store_xs, with_hc, alpha2 in ((0, 1.0, 1, False, None), (1, 1.0, 1, False, None),
                                                  (1, 1 / 3, 0, True, 0.01), (0, 0.5, 1, True, 0.1)):
        xs = old.to(DEV) if acc or not store_xs else sent(blk.rows, C)
        before = xs.clone()
        hc = sent(blk.rows, C, dtype=BF) if with_hc else None
        blk.fused(xs, acc=acc, scale=scale, store_xs=store_xs, hc=hc,
                  alpha2=0.1 if alpha2 is None else alpha2)
        want_v, want_hc = blk.oracle(acc_in=old if acc else None, scale=scale, alpha2=alpha2)
        mode = f"C={C} acc={acc} scale={scale:.3f} store_xs={store_xs}"
        assert_bitwise(xs, want_v if store_xs else before, "xs " + mode)
        if with_hc:
            assert_bitwise(hc, want_hc, "hc " + mode)


@pytest.mark.parametrize("C", [32, 64])
def test_resblock1_persistent_tile_loop(C):
    """More tiles than compute units (CUs + 44): the `tile += gridDim.x` loop and the barrier
    at its end, accumulating into xs."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = VO.persistent_case(C, n_cu)
    blk = lattice_block(case)
    assert blk.rows // R_(C) == n_cu + 44
    old = prior(blk.rows, C, seed=6)
    xs = old.to(DEV)
    blk.fused(xs, acc=1, scale=1.0)
    want_v, _ = blk.oracle(acc_in=old)
    assert_bitwise(xs, want_v, f"xs {case}")


@pytest.mark.parametrize("C", [32, 64])
def test_resblock1_lens_skips_whole_padding_tiles(C):
    """lens = [4R, R+1, R, 0]: a tile whose first row is >= lens stores nothing (xs keeps its
    contents, hc the sentinel); every other tile is bitwise the lens=None launch on all of its
    rows, those past lens included."""
    R = R_(C)
    case = (C, 4, 4 * R, 7, (1, 3, 5))
    assert case in VO.lattice_cases()
    blk = lattice_block(case)
    T = blk.T
    lens_l = [4 * R, R + 1, R, 0]
    lens = torch.tensor(lens_l, dtype=torch.int64, device=DEV)
    skipped = torch.zeros(blk.rows, dtype=torch.bool)
    for u, n in enumerate(lens_l):
        for t0 in range(0, T, R):
            if t0 >= n:
                skipped[u * T + t0:u * T + t0 + R] = True
    # [2R, 4R) of utterance 1, [R, 4R) of utterance 2, all of utterance 3
    assert skipped.view(4, 4, R)[:, :, 0].tolist() == [[False] * 4, [False, False, True, True],
                                                       [False, True, True, True], [True] * 4]
    old = prior(blk.rows, C, seed=7)
    want_v, _ = blk.oracle(acc_in=old)
    full = old.to(DEV)
    blk.fused(full, acc=1)
    assert_bitwise(full, want_v, "xs, lens=None")
    xs = old.to(DEV)
    blk.fused(xs, acc=1, lens=lens)
    assert_bitwise(xs, torch.where(skipped[:, None], old, full.cpu()), "xs, acc=1 with lens")
    # hc only
    _, want_hc = blk.oracle(alpha2=0.1)
    xs, hc_full, hc = sent(blk.rows, C), sent(blk.rows, C, dtype=BF), sent(blk.rows, C, dtype=BF)
    blk.fused(xs, store_xs=0, hc=hc_full)
    assert_bitwise(hc_full, want_hc, "hc, lens=None")
    blk.fused(xs, store_xs=0, hc=hc, lens=lens)
    assert_bitwise(hc, torch.where(skipped[:, None], sent(1, 1, dtype=BF).cpu(), hc_full.cpu()),
                   "hc only with lens")
    assert_bitwise(xs, sent(blk.rows, C), "xs with store_xs=0")


def per_conv_resblock(blk, xs, scale, hc, alpha2, acc):
    """One ResBlock1 as the unfused branch of Generator.forward_rows launches it: six
    fs2_conv_gemm_ex calls, the last folding the running sum (ADD_AUX | ACC_Y, scale, y2)."""
    rows, seq, C, k = blk.rows, blk.T, blk.C, blk.k
    pad = lambda d: (k * d - d) // 2
    cur = blk.x
    cur_l = torch.where(cur >= 0, cur, cur * 0.1).to(BF)  # the upsample conv's y2
    for m, d in enumerate(blk.dil):
        t_c = torch.empty(rows, C, dtype=BF, device=DEV)
        K.conv_gemm_ex(cur_l, blk.w1[m], rows, seq, C, C, k, pad(d), dilation=d, bias=blk.b1[m],
                       flags=K.EPI_LRELU, alpha=0.1, out=t_c)
        if m < 2:
            nxt = torch.empty(rows, C, dtype=torch.float32, device=DEV)
            nxt_l = torch.empty(rows, C, dtype=BF, device=DEV)
            K.conv_gemm_ex(t_c, blk.w2[m], rows, seq, C, C, k, pad(1), bias=blk.b2[m],
                           flags=K.EPI_ADD_AUX, aux=cur, out=nxt, y2=nxt_l, alpha2=0.1)
            cur, cur_l = nxt, nxt_l
        else:
            K.conv_gemm_ex(t_c, blk.w2[m], rows, seq, C, C, k, pad(1), bias=blk.b2[m],
                           flags=K.EPI_ADD_AUX | (K.EPI_ACC_Y if acc else 0), aux=cur, out=xs,
                           y2=hc, scale=scale, alpha2=alpha2)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [32, 64])
def test_resblock1_fused_per_conv_and_oracle_agree_bitwise(C):
    """Three ways to one block on the lattice -- the fused launch, the six per-conv launches
    and the oracle -- as the stage's last resblock (running sum in, 1/3, slope-0.01 copy
    out): bitwise equal, which is what the 2e-3 waveform comparison of the two GPU paths
    could only approximate."""
    case = (C, 2, 2 * R_(C), 7, (1, 3, 5))
    blk = lattice_block(case)
    old = prior(blk.rows, C, seed=8)
    want_v, want_hc = blk.oracle(acc_in=old, scale=1 / 3, alpha2=0.01)
    xs_f, hc_f = old.to(DEV), sent(blk.rows, C, dtype=BF)
    blk.fused(xs_f, acc=1, scale=1 / 3, hc=hc_f, alpha2=0.01)
    xs_u, hc_u = old.to(DEV), sent(blk.rows, C, dtype=BF)
    per_conv_resblock(blk, xs_u, 1 / 3, hc_u, 0.01, acc=True)
    assert_bitwise(xs_u, want_v, "per-conv xs against the oracle")
    assert_bitwise(hc_u, want_hc, "per-conv hc against the oracle")
    assert_bitwise(xs_f, want_v, "fused xs against the oracle")
    assert_bitwise(hc_f, want_hc, "fused hc against the oracle")
    assert_bitwise(xs_f, xs_u, "fused xs against per-conv")


@pytest.mark.parametrize("C,k", [(32, 11), (64, 7)])
def test_resblock1_signed_within_fp32_emulation_error(C, k, capsys):
    """Signed data (the negative leaky-ReLU branches, signed bias and residual adds): a bf16
    rounding point that flips under another fp32 summation order moves the chain, so the
    kernel is held to 4x the error of the fp32-accumulating emulation against the
    fp64-accumulating one, in rms and in max.  The factor covers a different order: a
    different, similarly sized set of flipped roundings, the maximum being one late flip of a
    large element.  hc is bitwise bf16(lrelu(kernel's own xs, 0.01)).

    Measured on an MI355X, as fractions of the output peak (kernel / fp32 emulation):
      C=32 k=11  rms 3.13e-05 / 1.98e-05 = 1.6x   max 4.26e-04 / 3.43e-04 = 1.2x
      C=64 k=7   rms 5.95e-05 / 7.44e-05 = 0.8x   max 7.17e-04 / 9.53e-04 = 0.8x"""
    R = R_(C)
    B, T, dil = 2, 2 * R, (1, 3, 5)
    g = torch.Generator().manual_seed(21 + C)
    x = torch.randn(B * T, C, generator=g)
    W = lambda: [(torch.randn(C, C, k, generator=g) / math.sqrt(C * k)).to(BF).float()
                 for _ in range(3)]
    Bs = lambda: [0.1 * torch.randn(C, generator=g) for _ in range(3)]
    blk = Block((C, B, T, k, dil), (x, W(), W(), Bs(), Bs()))
    v64, _ = blk.oracle(alpha2=0.01, dtype=torch.float64)
    v32, _ = blk.oracle(alpha2=0.01, dtype=torch.float32)
    xs, hc = sent(B * T, C), sent(B * T, C, dtype=BF)
    blk.fused(xs, hc=hc, alpha2=0.01)
    got = xs.cpu()
    peak = v64.abs().max().item()
    err = lambda a: ((a.double() - v64.double()).pow(2).mean().sqrt().item() / peak,
                     (a.double() - v64.double()).abs().max().item() / peak)
    (k_rms, k_max), (e_rms, e_max) = err(got), err(v32)
    with capsys.disabled():
        print(f"\nresblock1 signed C={C} k={k}: kernel rms {k_rms:.2e} max {k_max:.2e} ; "
              f"fp32 emulation rms {e_rms:.2e} max {e_max:.2e} (of peak {peak:.2f})")
    assert (got < 0).float().mean() > 0.2 and e_rms > 0
    assert k_rms <= 4 * e_rms, (k_rms, e_rms)
    assert k_max <= 4 * e_max, (k_max, e_max)
    assert_bitwise(hc, VO._lrelu(got, 0.01).to(BF), "hc of the kernel's own xs")


def raw_fused(x, rows, T, C, k, dil, w1, w2, b1, b2, xs, acc, scale, store_xs, hc, alpha2):
    """fs2_resblock1_fused without the wrapper's exception: the return code; None = NULL."""
    P = lambda ts: (ctypes.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in ts])
    d = (ctypes.c_int * 3)(*dil)
    pw1, pw2, pb1, pb2 = P(w1), P(w2), P(b1), P(b2)
    rc = K.lib.load().fs2_resblock1_fused(
        K.ptr(x), rows, T, C, k, ctypes.addressof(d), ctypes.addressof(pw1),
        ctypes.addressof(pw2), ctypes.addressof(pb1), ctypes.addressof(pb2), K.ptr(xs), acc, scale,
        store_xs, K.ptr(hc), alpha2, None, K.stream())
    torch.cuda.synchronize()
    return rc


def test_resblock1_supported_and_refusals():
    """fs2_resblock1_supported's limits, and fs2_resblock1_fused refusing each unsupported
    shape and malformed call with FS2_ERR_ARG before anything is launched (outputs keep the
    sentinel); rows = 0 is a no-op."""
    d135 = (1, 3, 5)
    unsupported = [(16, 512, 3, d135), (48, 512, 3, d135), (128, 512, 3, d135),
                   (32, 256 + 16, 3, d135), (64, 128 + 16, 3, d135),
                   (32, 512, 1, d135), (32, 512, 4, d135), (32, 512, 13, d135),
                   (32, 512, 3, (1, 0, 5)),
                   (32, 512, 3, (21, 21, 20)), (64, 512, 3, (21, 21, 20))]  # radius 65
    for C, T, k, dil in unsupported:
        assert not K.resblock1_supported(C, T, k, dil), (C, T, k, dil)
    for C in (32, 64):
        assert K.resblock1_supported(C, 512, 3, (21, 20, 20))  # radius 64
        assert K.resblock1_supported(C, 512, 9, (1, 5, 7))
        assert K.resblock1_supported(C, 512, 11, d135)
    # buffers large enough for any shape above, so even a wrongly accepted call stays in bounds
    CM, KM, rows_max = 128, 13, 1024
    x = torch.zeros(rows_max, CM, device=DEV)
    w = [torch.zeros(CM * CM * KM, dtype=BF, device=DEV) for _ in range(3)]
    b = [torch.zeros(CM, device=DEV) for _ in range(3)]
    xs, hc = sent(rows_max, CM), sent(rows_max, CM, dtype=BF)

    def refused(rows, T, C, k, dil, *, w2=w, store_xs=1, with_hc=True, what=""):
        rc = raw_fused(x, rows, T, C, k, dil, w, w2, b, b, xs, 0, 1.0, store_xs,
                       hc if with_hc else None, 0.1)
        assert rc == ERR_ARG, (what, rc)
        assert K.lib.load().fs2_last_error()  # a message is left
        assert_bitwise(xs, sent(rows_max, CM), "xs after refusal " + what)
        assert_bitwise(hc, sent(rows_max, CM, dtype=BF), "hc after refusal " + what)

    for C, T, k, dil in unsupported:
        refused(2 * T, T, C, k, dil, what=f"C={C} T={T} k={k} dil={dil}")
    refused(512 + 256, 512, 32, 3, d135, what="rows not whole utterances")
    refused(512, 512, 32, 3, d135, store_xs=0, with_hc=False, what="no output")
    refused(512, 512, 32, 3, d135, w2=[w[0], None, w[2]], what="null conv pointer")
    assert raw_fused(x, 0, 512, 32, 3, d135, w, w, b, b, xs, 0, 1.0, 1, hc, 0.1) == 0
    assert_bitwise(xs, sent(rows_max, CM), "xs after rows = 0")
    assert_bitwise(hc, sent(rows_max, CM, dtype=BF), "hc after rows = 0")


# ------------------------------------------------------------------ fs2_vocoder_post
POST_SHAPES = [(5, 100),  # 500 rows: blocks span three utterances, the last block is partial
               (1, 256), (2, 259), (3, 1), (2, 3), (1, 700)]


def post_inputs(B, T, c_in, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, c_in, generator=g).to(dtype)
    w = torch.randn(1, c_in, 7, generator=g) / math.sqrt(7 * c_in)
    b = torch.tensor([0.05])
    return x, w, b


def run_post(x, w, b, T, max_wav=32768.0, pcm=True, lens=None):
    wav, p = K.vocoder_post(x.to(DEV), x.shape[0], T, x.shape[1], w.reshape(-1).to(DEV),
                            b.to(DEV), max_wav, pcm=pcm, lens=lens)
    torch.cuda.synchronize()
    return wav.cpu(), None if p is None else p.cpu().numpy()


@pytest.mark.parametrize("c_in", [1, 7, 32, 64])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_vocoder_post_against_fp64(dtype, c_in):
    """conv_post + tanh against fp64 on the same (fp32 or bf16) input values, at shapes whose
    256-row blocks span utterances, end partial, or hold utterances shorter than the 7 taps.
    Bound per sample: 7 c_in 2^-24 sum|w x| for the fp32 dot product (tanh' <= 1) plus 4 2^-24
    for tanhf at |v| <= 1.  c_in = 64 stages 68,864 B of dynamic LDS, past 64 KiB: the runtime
    takes it without an opt-in (a refusal would surface as a launch error).  The int16 output is the
    documented rule applied to the kernel's own wav, at both max_wav values the corpus
    configurations use; pcm=None changes nothing."""
    for n, (B, T) in enumerate(POST_SHAPES):
        x, w, b = post_inputs(B, T, c_in, dtype, seed=100 * c_in + n)
        want, _, mag = VO.conv_post(x, w, b, T=T, max_wav=32768.0)
        bound = 7 * c_in * 2.0 ** -24 * mag + 4 * 2.0 ** -24
        for max_wav in (32768.0, 32767.0):
            wav, pcm = run_post(x, w, b, T, max_wav)
            excess = ((wav.double() - want).abs() - bound).max().item()
            assert excess <= 0, (B, T, excess)
            assert np.array_equal(pcm, VO.pcm_of(wav.numpy(), max_wav)), (B, T, max_wav)
        wav2, none = run_post(x, w, b, T, pcm=False)
        assert none is None
        assert torch.equal(bits(wav2), bits(wav)), (B, T)


def test_vocoder_post_pcm_edges():
    """A saturated tanh: wav is exactly +-1.0f, whose int16 wraps to -32768 at max_wav 32768
    and is +-32767 at 32767; a tiny negative sample truncates toward zero to 0, not to -1."""
    x = torch.tensor([[20.0], [-20.0], [-1e-5], [1e-5], [0.5], [-0.5], [0.0], [3.0]])
    w = torch.zeros(1, 1, 7)
    w[0, 0, 3] = 1.0  # centre tap: v[r] = x[r]
    b = torch.zeros(1)
    for max_wav, first in ((32768.0, [-32768, -32768, 0, 0]), (32767.0, [32767, -32767, 0, 0])):
        wav, pcm = run_post(x, w, b, 8, max_wav)
        assert wav[0].item() == 1.0 and wav[1].item() == -1.0
        assert -1.0 < wav[2].item() * max_wav < 0.0
        assert pcm[:4].tolist() == first, (max_wav, pcm.tolist())
        assert np.array_equal(pcm, VO.pcm_of(wav.numpy(), max_wav))
    # the same through large weights and bias, over 32 bf16 channels
    x = torch.ones(8, 32).to(BF)
    w = torch.full((1, 32, 7), 0.5)
    for bias, value, p in ((0.0, 1.0, -32768), (-200.0, -1.0, -32768)):
        wav, pcm = run_post(x, w, torch.tensor([bias]), 8)
        assert (wav == value).all() and (pcm == p).all()


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,lens_l", [
    # block [256, 512) starts in utterance 2's padding and holds utterance 3's valid rows
    (5, 100, [100, 0, 1, 99, 37]),
    # whole blocks of padding (the early return), [1024, 1280) over two utterances; block
    # [512, 768) ends utterance 0 and holds the 10 valid rows of utterance 1
    (3, 600, [600, 10, 0])])
def test_vocoder_post_lens(B, T, lens_l, dtype):
    """Rows t >= lens are exactly 0.0f / 0, rows t < lens bitwise the lens=None launch."""
    x, w, b = post_inputs(B, T, 32, dtype, seed=77)
    full_w, full_p = run_post(x, w, b, T)
    lens = torch.tensor(lens_l, dtype=torch.int64, device=DEV)
    wav, pcm = run_post(x, w, b, T, lens=lens)
    keep = (torch.arange(B * T) % T) < torch.tensor(lens_l).repeat_interleave(T)
    assert 0 < keep.sum() < B * T and (full_w != 0).all()
    want_w = torch.where(keep, full_w, torch.zeros_like(full_w))  # +0.0f: all bits zero
    assert torch.equal(bits(wav), bits(want_w))
    assert np.array_equal(pcm, np.where(keep.numpy(), full_p, 0).astype(np.int16))
    # the oracle's lens rule names the same rows
    want, _, _ = VO.conv_post(x, w, b, T=T, max_wav=32768.0, lens=lens_l)
    assert torch.equal(want != 0, wav != 0)


def test_vocoder_post_refusals():
    """c_in outside [1, 64] is refused before any launch, an unknown dtype is FS2_ERR_DTYPE,
    rows = 0 is a no-op; the outputs keep the sentinel."""
    post = K.lib.load().fs2_vocoder_post
    rows, T = 300, 100
    x = torch.zeros(rows, 80, device=DEV)
    w, b = torch.zeros(7 * 80, device=DEV), torch.zeros(1, device=DEV)
    wav = sent(rows, 1)
    pcm = torch.full((rows, 1), 777, dtype=torch.int16, device=DEV)

    def call(dtype, n, c_in):
        rc = post(dtype, x.data_ptr(), n, T, c_in, None, w.data_ptr(), b.data_ptr(), 32768.0,
                  wav.data_ptr(), pcm.data_ptr(), K.stream())
        torch.cuda.synchronize()
        assert_bitwise(wav, sent(rows, 1), f"wav after c_in={c_in} dtype={dtype} rows={n}")
        assert (pcm == 777).all()
        return rc

    assert call(K.F32, rows, 65) == ERR_ARG
    assert call(K.BF16, rows, 65) == ERR_ARG
    assert call(K.F32, rows, 0) == ERR_ARG
    assert call(7, rows, 32) == ERR_DTYPE
    assert call(K.F32, 0, 32) == 0


# ------------------------------------------------------------------ fs2_conv_gemm_ex + lens
LRELU, AUXACC = K.EPI_LRELU, K.EPI_ADD_AUX | K.EPI_ACC_Y
GEMM_CASES = [  # c_in, c_out, taps, dilation, pad, epilogue flags, out, y2
    (128, 128, 11, 5, 25, LRELU, "bf16", False),    # convs1 of the 128-channel stage
    (128, 128, 3, 1, 1, AUXACC, "f32", True),       # a resblock's last conv: running sum + copy
    (64, 64, 7, 3, 9, AUXACC, "f32", True),
    (32, 32, 11, 1, 5, LRELU, "bf16", False),
    (64, 2 * 32, 3, 1, 1, 0, None, True),           # ConvTranspose1d as the 3-tap phase conv
]


@pytest.mark.parametrize("mode", [0, -1], ids=["halo", "tapmajor"])
@pytest.mark.parametrize("c_in,c_out,taps,dil,pad,epi,out_kind,with_y2", GEMM_CASES)
def test_conv_gemm_ex_lens(c_in, c_out, taps, dil, pad, epi, out_kind, with_y2, mode):
    """The length-aware vocoder convs at B = 3, T = 1024, lens = [1024, 300, 0], with tuning
    knob 6 at 0 (halo kernels where eligible) and -1 (tap-major):

    1. rows t < lens are bitwise the lens=None launch, in out and y2;
    2. a padded row is, as a whole row, either the lens=None row or the skipped value: with
       FS2_EPI_SKIP_NOSTORE the buffer's earlier contents, else the epilogue of a zero
       accumulator without bias (aux under ADD_AUX, then ACC_Y, scale, LRELU; y2 of that);
    3. the skip happens: the tallest row tile of these kernels is 256 rows
       (conv_gemm_halo<256, 128, ...> in csrc/gemm_glds.hip, chosen by csrc/conv_plan.hpp; the
       vocoder instantiations use 128 and 64), so any tiling puts rows [768, 1024) of
       utterance 1 and [256, 768) of utterance 2 in all-padding tiles;
    4. the fp32 path ignores lens."""
    B, T = 3, 1024
    rows, lens_l = B * T, [1024, 300, 0]
    g = torch.Generator().manual_seed(c_in + taps)
    rn = lambda *s: torch.randn(*s, generator=g)
    x32 = rn(rows, c_in).to(BF).float()
    w = (rn(c_out, c_in, taps) / math.sqrt(c_in * taps)).to(BF).float()
    bias = (0.1 * rn(c_out)).to(DEV)
    aux, y_old = rn(rows, c_out), rn(rows, c_out)
    scale, alpha, alpha2 = (1 / 3, 0.1, 0.01) if epi & K.EPI_ACC_Y else (1.0, 0.1, 0.1)
    lens = torch.tensor(lens_l, dtype=torch.int64, device=DEV)
    t = torch.arange(rows) % T
    valid = t < torch.tensor(lens_l).repeat_interleave(T)
    u = torch.arange(rows) // T
    must_skip = ((u == 1) & (t >= 768)) | ((u == 2) & (t >= 256) & (t < 768))

    def launch(dt, flags, lens_):
        """-> (out, y2) on the CPU (None where not produced), and their earlier contents."""
        x = x32.to(dt).to(DEV)
        wf = prep(w, dt)
        if out_kind is None:
            out = None
        elif epi & K.EPI_ACC_Y:
            out = y_old.to(DEV)
        else:
            out = sent(rows, c_out, dtype=BF if (out_kind == "bf16" and dt == BF) else torch.float32)
        y2 = sent(rows, c_out, dtype=dt) if with_y2 else None
        before = tuple(None if o is None else o.cpu() for o in (out, y2))
        K.lib.fs2_set_tuning(6, mode)
        try:
            K.conv_gemm_ex(x, wf, rows, T, c_in, c_out, taps, pad, dilation=dil, bias=bias,
                           flags=flags, aux=aux.to(DEV) if epi & K.EPI_ADD_AUX else None, out=out,
                           y2=y2, alpha=alpha, scale=scale, alpha2=alpha2, lens=lens_)
            torch.cuda.synchronize()
        finally:
            K.lib.fs2_set_tuning(6, 0)
        return tuple(None if o is None else o.cpu() for o in (out, y2)), before

    def zero_acc_rows(dtypes):
        """The epilogue of a zero accumulator without bias, per output."""
        v = torch.zeros(rows, c_out)
        if epi & K.EPI_ADD_AUX:
            v = v + aux
        if epi & K.EPI_ACC_Y:
            v = (v + y_old) * torch.tensor(scale, dtype=torch.float32)
        if epi & K.EPI_LRELU:
            v = VO._lrelu(v, alpha)
        return (None if dtypes[0] is None else v.to(dtypes[0]),
                None if dtypes[1] is None else VO._lrelu(v, alpha2).to(dtypes[1]))

    full, _ = launch(BF, epi, None)
    for flags in (epi | K.EPI_SKIP_NOSTORE, epi):
        got, before = launch(BF, flags, lens)
        nostore = bool(flags & K.EPI_SKIP_NOSTORE)
        skipped_value = before if nostore else zero_acc_rows(
            [None if o is None else o.dtype for o in got])
        choice = []
        for name, o, f, s in zip(("out", "y2"), got, full, skipped_value):
            if o is None:
                continue
            what = f"{name}, nostore={nostore}"
            ob, fb, sb = bits(o), bits(f), bits(s)
            is_full, is_skip = (ob == fb).all(1), (ob == sb).all(1)
            assert is_full[valid].all(), f"{what}: {int((~is_full[valid]).sum())} valid rows differ"
            neither = ~(is_full | is_skip) & ~valid
            assert not neither.any(), (f"{what}: padded rows neither computed nor skipped: "
                                       f"{neither.nonzero().flatten().tolist()[:8]}")
            assert is_skip[must_skip].all(), (f"{what}: rows of all-padding tiles not skipped: "
                                              f"{(~is_skip & must_skip).nonzero().flatten().tolist()[:8]}")
            assert not (fb == sb).all(1).any()  # the two alternatives are distinguishable
            choice.append(is_skip)
        if len(choice) == 2:
            assert torch.equal(choice[0], choice[1]), "out and y2 disagree on the skipped rows"
    # 4. fp32: exact path, no skipping
    full32, _ = launch(torch.float32, epi, None)
    for flags in (epi | K.EPI_SKIP_NOSTORE, epi):
        got32, _ = launch(torch.float32, flags, lens)
        for name, o, f in zip(("out", "y2"), got32, full32):
            if o is not None:
                assert_bitwise(o, f, f"fp32 {name} with lens")
