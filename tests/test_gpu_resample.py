"""The resampler on the GPU (fs2_resample, kernels.resample, audio.Resampler) against the oracles
of resample_oracle.py.

Tolerance rule, the one of test_gpu_melspec.py and test_gpu_pitch.py: a sample is compared with
the float64 oracle under max(4 x max|ref32 - oracle64| on that same row, 4 fp32 ulps of the
value); every live sample of every row is compared.  Nothing here is compared with resampy or
soxr: neither is installed, and resampy interpolates its filter table where this kernel evaluates
the window exactly.

The kernel's tile is 4 P outputs, P = L ceil(256 / L) (L itself above 256): 1 176 at L = 147,
1 764 at L = 441, 1 024 at L = 1 and 2.  So the longest row has 5 200 samples (2 389 outputs at
48 000 Hz, the fewest: three tiles at every ratio), and three more rows per ratio end just
before, at and just after the first tile boundary.  192 000 -> 8 000 Hz (a span too long for
four outputs per thread) takes the kernel's other instance, tile 256.
"""
import importlib

import numpy as np
import pytest
import torch

import resample_oracle as O

NAME = "mid-attribute-speaker-generation_amd"
pytestmark = pytest.mark.gpu

SR_OUT = 22050
RATES = (48000, 24000, 16000, 44100, 11025)
BASE, S = [1, 2, 293, 700], 5200
LONG = 7  # the row of S samples; 3 is the 700-sample one
_CACHE = {}


def _mod(name):
    return importlib.import_module(f"{NAME}.{name}")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tile(L):
    return 4 * (L * -(-256 // L) if L <= 256 else L)


def _lens(sr_in):
    """Lengths 1 and 2 (shorter than one filter span), 293, 700 (every phase at least twice),
    the longest with fewer outputs than a tile, the shortest with a tile's and with more, and S."""
    L, M = O.ratio(sr_in, SR_OUT)
    tile = _tile(L)
    edge = [max(n for n in range(1, S) if O.n_out(n, L, M) < tile),
            min(n for n in range(1, S) if O.n_out(n, L, M) >= tile),
            min(n for n in range(1, S) if O.n_out(n, L, M) > tile)]
    return BASE + edge + [S]


def _rows(sr_in):
    if ("rows", sr_in) not in _CACHE:
        rng = np.random.default_rng(21)
        _CACHE["rows", sr_in] = [(0.3 * rng.standard_normal(n)).astype(np.float32)
                                 for n in _lens(sr_in)]
    return _CACHE["rows", sr_in]


def _batch(sr_in):
    """The eight rows in (8, S); what follows a row is 0.1 sigma noise, not zeros."""
    rows = _rows(sr_in)
    wav = (0.1 * np.random.default_rng(22).standard_normal((len(rows), S))).astype(np.float32)
    for b, x in enumerate(rows):
        wav[b, :len(x)] = x
    return wav


def _run(sr_in, wav, lens=None, first=None, count=None, cols=None, sr_out=SR_OUT):
    """K.resample into NaN-prefilled outputs -> numpy (out, out_lens)."""
    K = _mod("kernels")
    table, L, M, half = O.table32(sr_in, sr_out)
    w = _dev(wav)
    B, n = w.shape
    cols = O.n_out(n, L, M) if cols is None else cols
    out = (torch.full((B, cols), float("nan"), device="cuda"),
           torch.full((B,), -1, dtype=torch.int64, device="cuda"))
    i64 = lambda v: None if v is None else _dev(np.asarray(v, np.int64))  # noqa: E731
    K.resample(w, i64(lens), _dev(table), L, M, half, first=i64(first), count=i64(count), out=out)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _full(sr_in):
    if ("full", sr_in) not in _CACHE:
        _CACHE["full", sr_in] = _run(sr_in, _batch(sr_in), _lens(sr_in))
    return _CACHE["full", sr_in]


def _check(tag, rows, y, n, sr_in, sr_out):
    """Every live sample of every row against the oracle under the rule of the module docstring;
    returns the largest deviation and the smallest bound."""
    compared, worst, bound = 0, 0.0, np.inf
    for b, x in enumerate(rows):
        k = int(n[b])
        assert not y[b, k:].any()  # exactly 0 past the row's length
        want, ref = O.oracle64(x, sr_in, sr_out), O.ref32(x, sr_in, sr_out)
        assert len(want) == k
        tol = O.rule(ref, want)
        dev = np.abs(y[b, :k].astype(np.float64) - want)
        print(f"{tag} len {len(x)}: outputs {k} dev {dev.max():.3e} bound {tol.min():.3e} "
              f"ref32 dev {np.abs(ref - want).max():.3e}")
        assert (dev <= tol).all(), (tag, len(x))
        compared += k
        worst, bound = max(worst, dev.max()), min(bound, tol.min())
    assert compared == int(np.sum(n))
    return worst, bound


@pytest.mark.parametrize("sr_in", RATES)
def test_ragged_batch_matches_oracle(sr_in):
    L, M = O.ratio(sr_in, SR_OUT)
    lens = _lens(sr_in)
    y, n = _full(sr_in)
    assert np.isfinite(y).all()
    assert n.tolist() == [-(-k * L // M) for k in lens]
    assert y.shape == (len(lens), -(-S * L // M))
    tile = _tile(L)
    assert n[4] < tile <= n[5] <= tile + 1 and tile < n[6] <= tile + 2 and n[LONG] > 2 * tile
    worst, bound = _check(f"{sr_in} -> {SR_OUT}", _rows(sr_in), y, n, sr_in, SR_OUT)
    print(f"{sr_in} -> {SR_OUT}: largest deviation {worst:.3e}, smallest bound {bound:.3e}")
    if L > 1:  # every phase occurs, at least twice on the 700-sample row
        phases = np.bincount((np.arange(n[3]) * M) % L, minlength=L)
        assert phases.min() >= 2
    assert np.abs(y[LONG]).max() > 0.1


def test_long_span_ratio_takes_the_other_instance():
    """192 000 -> 8 000 Hz: L = 1, M = 24, 3 243 taps per output; four outputs per thread would
    need 27 797 samples in LDS, so a thread computes one (tile 256)."""
    lens = [1, 700, 6130, 6150, 20000]  # 1, 30, 256, 257 and 834 outputs
    rng = np.random.default_rng(23)
    rows = [(0.3 * rng.standard_normal(k)).astype(np.float32) for k in lens]
    wav = (0.1 * rng.standard_normal((len(lens), lens[-1]))).astype(np.float32)
    for b, x in enumerate(rows):
        wav[b, :len(x)] = x
    y, n = _run(192000, wav, lens, sr_out=8000)
    assert np.isfinite(y).all() and n.tolist() == [1, 30, 256, 257, 834]
    _check("192000 -> 8000", rows, y, n, 192000, 8000)
    y1, n1 = _run(192000, rows[3][None], sr_out=8000)
    assert np.array_equal(y1[0], y[3, :257])
    yw, nw = _run(192000, wav, lens, [0, 7, 250, 250, 600], [9, 9, 9, 9, 400], cols=300, sr_out=8000)
    assert nw.tolist() == [1, 9, 6, 7, 234]
    assert np.array_equal(yw[4, :234], y[4, 600:834]) and np.array_equal(yw[3, :7], y[3, 250:257])


@pytest.mark.parametrize("sr_in", RATES)
def test_bitwise_identities(sr_in):
    L, M = O.ratio(sr_in, SR_OUT)
    lens, tile = _lens(sr_in), _tile(L)
    y, n = _full(sr_in)
    again = _run(sr_in, _batch(sr_in), lens)
    assert np.array_equal(again[0], y) and np.array_equal(again[1], n)
    for b, x in enumerate(_rows(sr_in)):  # alone, S = its own length: nothing past len is read
        y1, n1 = _run(sr_in, x[None])
        assert n1[0] == n[b] == y1.shape[1]
        assert np.array_equal(y1[0], y[b, :n[b]])
    # windows: inside the row, across a tile boundary, starting in the last tile, and empty
    first = [0, 1, 137, 137, 137, tile - 3, 137, 137]
    count = [5, 5, 500, 500, 500, 500, 500, 500]
    yw, nw = _run(sr_in, _batch(sr_in), lens, first, count, cols=517)
    for b in range(len(lens)):
        k = max(min(count[b], int(n[b]) - min(first[b], int(n[b]))), 0)
        assert nw[b] == k
        assert np.array_equal(yw[b, :k], y[b, first[b]:first[b] + k]) and not yw[b, k:].any()
    assert nw[LONG] == 500 and np.array_equal(yw[LONG, :500], y[LONG, 137:637])
    total = int(n[LONG])
    last = (total - 1) // tile * tile + 1
    assert last > 2 * tile
    yw, nw = _run(sr_in, _batch(sr_in)[LONG:], lens[LONG:], [last], [10 ** 6], cols=tile + 9)
    assert nw[0] == total - last and np.array_equal(yw[0, :nw[0]], y[LONG, last:total])
    assert not yw[0, nw[0]:].any()
    yw, nw = _run(sr_in, _batch(sr_in)[3:5], lens[3:5], [137, 10 ** 9], [0, 7], cols=9)
    assert nw.tolist() == [0, 0] and not yw.any() and not np.isnan(yw).any()
    yw, nw = _run(sr_in, _batch(sr_in)[LONG:], lens[LONG:], None, [300], cols=300)  # count alone
    assert nw[0] == 300 and np.array_equal(yw[0], y[LONG, :300])


def test_resampler_entry_points():
    A = _mod("audio")
    rs = A.Resampler(SR_OUT)
    for sr_in in (48000, 16000):
        wav, lens = _dev(_batch(sr_in)), _lens(sr_in)
        y, n = _full(sr_in)
        got = rs(wav, lens, sr_in)
        assert np.array_equal(got[0].cpu().numpy(), y) and got[1].tolist() == n.tolist()
        dev_lens = rs(wav, _dev(np.asarray(lens, np.int64)), sr_in)
        assert torch.equal(dev_lens[0], got[0]) and torch.equal(dev_lens[1], got[1])
        assert rs.out_len(700, sr_in) == n[3]
    first, count = [0, 0, 10, 137, 137, 137, 137, 137], [9, 9, 20, 500, 400, 400, 400, 400]
    cut, k = rs(wav, lens, 16000, first=first, count=count)  # 700 samples give 965 outputs
    assert cut.shape == (8, 500) and k.tolist() == [2, 3, 20, 500, 400, 400, 400, 400]
    assert np.array_equal(cut[3].cpu().numpy(), y[3, 137:637])
    assert np.array_equal(cut[LONG, :400].cpu().numpy(), y[LONG, 137:537]) and not cut[LONG, 400:].any()
    whole = rs(wav, None, 16000)  # lens None: S for every row
    assert whole[1].tolist() == [int(n[LONG])] * 8
    assert np.array_equal(whole[0][LONG].cpu().numpy(), y[LONG])
    assert len(rs._tables) == 2  # one device table per sr_in, kept


def test_equal_rates_launch_nothing():
    rs = _mod("audio").Resampler(SR_OUT)
    wav, lens = _dev(_batch(48000)), _lens(48000)
    out, n = rs(wav, lens, SR_OUT)
    assert out is wav and n.tolist() == lens and not rs._tables


def test_argument_errors():
    K, KernelError = _mod("kernels"), _mod("_lib").KernelError
    table, L, M, half = O.table32(48000, SR_OUT)
    wav, tab = _dev(_batch(48000)), _dev(table)
    with pytest.raises(KernelError, match="coprime"):
        K.resample(wav, None, tab, 2 * L, 2 * M, half)
    with pytest.raises(KernelError, match="taps"):
        K.resample(wav, None, _dev(table[:-1]), L, M, half)
    with pytest.raises(KernelError, match="missing operand"):
        _mod("_lib").lib.fs2_resample(wav.data_ptr(), None, 8, S, None, len(table), L, M, half, None,
                                      None, wav.data_ptr(), 16, wav.data_ptr(), None)
    with pytest.raises(RuntimeError):
        K.resample(wav, None, tab.double(), L, M, half)
    with pytest.raises(RuntimeError):
        K.resample(wav.cpu(), None, tab, L, M, half)  # no CPU path
    with pytest.raises(ValueError):
        _mod("audio").Resampler(SR_OUT)(wav, _lens(48000)[:LONG] + [S + 1], 48000)
