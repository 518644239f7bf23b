"""Tensor-level wrappers over the C-ABI (``include/fs2hip.h``).

Each wrapper checks device/dtype/contiguity on the host, allocates outputs and workspaces
from PyTorch's caching allocator, and launches on the current HIP stream.  The storage type
of a GEMM/attention operand is taken from the tensor (float32 -> exact f32 MFMA path,
bfloat16 -> bf16 MFMA path, fp32 accumulation either way).  Norm/embedding kernels always
compute in fp32 and can emit a bf16 *compute copy* of their output (``copy=torch.bfloat16``)
for the next GEMM.  There is no PyTorch-math fallback: a wrong input raises, a missing
library raises.
"""
import ctypes

import torch

from ._lib import lib

F32 = 0
BF16 = 1
F64 = 2
EPI_BIAS, EPI_RELU, EPI_ADD_AUX, EPI_RELU_MASK_AUX, EPI_OUT_BF16, EPI_AUX_BF16 = 1, 2, 4, 8, 16, 32
EPI_LRELU, EPI_ACC_Y, EPI_Y2, EPI_SKIP_NOSTORE = 64, 128, 256, 512
_CODE = {torch.float32: F32, torch.bfloat16: BF16}


_DEV_INDEX = []


def stream():
    """Raw handle of the calling thread's current HIP stream (one device per process)."""
    if not _DEV_INDEX:
        _DEV_INDEX.append(torch.cuda.current_device())
    return torch._C._cuda_getCurrentRawStream(_DEV_INDEX[0])


def ptr(t):
    return None if t is None else t.data_ptr()


def _dev(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise RuntimeError("fs2 kernels need tensors on the GPU (no CPU path exists)")
            if not t.is_contiguous():
                raise RuntimeError("fs2 kernels need contiguous tensors")


def code(dtype):
    try:
        return _CODE[dtype]
    except KeyError:
        raise RuntimeError(f"unsupported compute dtype {dtype}") from None


def seed_arg(seed, device):
    """Dropout seed as the device pointer the kernels read: a device int64 tensor is passed
    through (the model's per-step seed), a host int is uploaded (tests, one-off calls)."""
    if torch.is_tensor(seed):
        if not seed.is_cuda or seed.dtype != torch.int64:
            raise RuntimeError("seed tensor must be a CUDA int64 tensor")
        return seed
    return torch.tensor([int(seed) & (2 ** 63 - 1)], dtype=torch.int64, device=device)


def ws(nbytes, device):
    return torch.empty(max(int(nbytes) // 4, 1), dtype=torch.float32, device=device)


def _copy(shape, copy, device):
    return None if copy is None else torch.empty(shape, dtype=copy, device=device)


# ------------------------------------------------------------------ GEMM / conv
def conv_gemm(x, wk, rows, seq_len, c_in, c_out, taps, pad, bias=None, flags=0, aux=None,
              out=None, ldx=None, out_dtype=torch.float32, lens=None):
    """y = conv(x) (+bias, epilogue flags); x/wk fp32 or bf16 (same), y fp32 or bf16.
    ``lens``: all-padding row tiles are not computed (see fs2_conv_gemm)."""
    _dev(x, wk, bias, aux, lens)
    if x.dtype != wk.dtype:
        raise RuntimeError(f"conv_gemm operand dtypes differ: {x.dtype} vs {wk.dtype}")
    if out is None:
        out = torch.empty(rows, c_out, dtype=out_dtype, device=x.device)
    if bias is not None:
        flags |= EPI_BIAS
    if out.dtype == torch.bfloat16:
        flags |= EPI_OUT_BF16
    if aux is not None and aux.dtype == torch.bfloat16:
        flags |= EPI_AUX_BF16
    lib.fs2_conv_gemm(code(x.dtype), ptr(x), ldx or c_in, ptr(wk), ptr(out), c_out, rows, seq_len,
                      c_in, c_out, taps, pad, ptr(lens), ptr(bias), flags, ptr(aux), c_out,
                      stream())
    return out


def conv_gemm_ln(x, wk, rows, seq_len, c_in, c_out, taps, pad, gamma, beta, bias=None, res=None,
                 lens=None, p_in=0.0, seed=0, site_in=0, copy=torch.bfloat16, res_ln=None,
                 want_out=True):
    """bf16 conv/Linear with the post-LayerNorm fused in (fs2_conv_gemm_ln): returns
    ``ln_fwd(conv_gemm(x) + bias, res=res, p_in=...)``'s (out fp32, out compute copy, xhat,
    rstd), bitwise, without the fp32 intermediate.  ``res_ln`` / ``want_out``: as ``ln_fwd``."""
    rx, rg, rb = res_ln if res_ln is not None else (None, None, None)
    _dev(x, wk, gamma, beta, bias, res, lens, rx, rg, rb)
    if x.dtype != torch.bfloat16 or wk.dtype != torch.bfloat16:
        raise RuntimeError("conv_gemm_ln: bf16 operands only")
    out = torch.empty(rows, c_out, dtype=torch.float32, device=x.device) if want_out else None
    out_t = _copy((rows, c_out), copy, x.device)
    xhat = torch.empty(rows, c_out, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    sd = seed_arg(seed, x.device) if p_in > 0 else None
    lib.fs2_conv_gemm_ln_nres(ptr(x), c_in, ptr(wk), rows, seq_len, c_in, c_out, taps, pad,
                              ptr(lens), ptr(bias), ptr(res), ptr(rx), ptr(rg), ptr(rb),
                              ptr(gamma), ptr(beta), ptr(out), ptr(out_t), ptr(xhat), ptr(rstd),
                              p_in, ptr(sd), site_in, stream())
    return out, out_t, xhat, rstd


def conv_gemm_ln_bwd(x, wk, rows, seq_len, c_in, c_out, taps, pad, xhat, rstd, gamma, dgamma,
                     dbeta, aux=None, lens=None, p_in=0.0, seed=0, site_in=0, dres=None,
                     dres_add=False, dbias_in=None, copy=torch.bfloat16):
    """bf16 conv/Linear whose output (+ aux) is a post-LayerNorm's upstream gradient, with that
    LayerNorm's backward in the epilogue (fs2_conv_gemm_ln_bwd): returns ``ln_bwd(conv_gemm(x,
    flags=ADD_AUX, aux=aux), ...)``'s (dy compute copy, dres); dgamma / dbeta / dbias_in
    accumulate."""
    _dev(x, wk, aux, xhat, rstd, gamma, dgamma, dbeta, dbias_in, lens, dres)
    if x.dtype != torch.bfloat16 or wk.dtype != torch.bfloat16:
        raise RuntimeError("conv_gemm_ln_bwd: bf16 operands only")
    if dres is None:
        dres = torch.empty(rows, c_out, dtype=torch.float32, device=x.device)
    dy_t = _copy((rows, c_out), copy, x.device)
    n = lib.fs2_ln_bwd_ws_bytes(rows, c_out)
    w = ws(n, x.device)
    sd = seed_arg(seed, x.device) if p_in > 0 else None
    lib.fs2_conv_gemm_ln_bwd(ptr(x), c_in, ptr(wk), rows, seq_len, c_in, c_out, taps, pad,
                             ptr(lens), ptr(aux), ptr(xhat), ptr(rstd), ptr(gamma), ptr(dgamma),
                             ptr(dbeta), ptr(dbias_in), p_in, ptr(sd), site_in, ptr(dres),
                             int(dres_add), ptr(dy_t), ptr(w), n, stream())
    return dy_t, dres


def conv_gemm_ex(x, wk, rows, seq_len, c_in, c_out, taps, pad, dilation=1, bias=None, flags=0,
                 aux=None, out=None, y2=None, alpha=0.1, scale=1.0, alpha2=0.1, lens=None):
    """Dilated conv with the vocoder epilogue (fs2_conv_gemm_ex): out and/or y2 (the
    leaky-ReLU'd compute copy, dtype of x) must be given; ACC_Y reads ``out`` first.
    ``lens`` (int64 per utterance, rows of this resolution): tiles past it may be skipped."""
    _dev(x, wk, bias, aux, out, y2, lens)
    if x.dtype != wk.dtype:
        raise RuntimeError(f"conv_gemm_ex operand dtypes differ: {x.dtype} vs {wk.dtype}")
    if out is None and y2 is None:
        raise RuntimeError("conv_gemm_ex: give out and/or y2")
    if any(t is not None and t.data_ptr() == x.data_ptr() for t in (out, y2)):
        raise RuntimeError("conv_gemm_ex: an output must not be the input buffer (other blocks "
                           "of the launch read its rows as their taps' halo)")
    if y2 is not None:
        if y2.dtype != x.dtype or y2.shape != (rows, c_out):
            raise RuntimeError("conv_gemm_ex: y2 must be (rows, c_out) in the compute dtype")
        flags |= EPI_Y2
    if bias is not None:
        flags |= EPI_BIAS
    if out is not None and out.dtype == torch.bfloat16:
        flags |= EPI_OUT_BF16
    if aux is not None and aux.dtype == torch.bfloat16:
        flags |= EPI_AUX_BF16
    lib.fs2_conv_gemm_ex(code(x.dtype), ptr(x), c_in, ptr(wk), ptr(out), c_out, rows, seq_len,
                         c_in, c_out, taps, pad, dilation, ptr(lens), ptr(bias), flags, ptr(aux),
                         c_out, alpha, scale, ptr(y2), alpha2, stream())
    return out, y2


def convT_weight_prep(w, bias, stride):
    """ConvTranspose1d (c_in, c_out, 2*stride) weight -> (stride*c_out, c_in, 3) conv weight
    and the phase-tiled bias (fs2_convT_weight_prep)."""
    _dev(w, bias)
    c_in, c_out, k = w.shape
    if k != 2 * stride:
        raise RuntimeError(f"convT_weight_prep: kernel {k} != 2 * stride {stride}")
    wc = torch.empty(stride * c_out, c_in, 3, dtype=torch.float32, device=w.device)
    bc = torch.empty(stride * c_out, dtype=torch.float32, device=w.device)
    lib.fs2_convT_weight_prep(ptr(w), ptr(bias), c_in, c_out, stride, ptr(wc), ptr(bc), stream())
    return wc, bc


def resblock1_supported(channels, seq_len, kernel_size, dilations):
    d = (ctypes.c_int * 3)(*dilations)
    return bool(lib.fs2_resblock1_supported(channels, seq_len, kernel_size, ctypes.addressof(d)))


def resblock1_fused(x, rows, seq_len, channels, kernel_size, dilations, w1, w2, b1, b2, xs,
                    acc, scale, store_xs=True, hc=None, alpha2=0.1, lens=None):
    """One HiFi-GAN ResBlock1 in one launch (fs2_resblock1_fused): x (rows, C) fp32 ->
    xs (= (xs + out) * scale when acc, else out * scale) and / or hc (bf16 leaky ReLU)."""
    _dev(x, xs, hc, lens, *w1, *w2, *b1, *b2)
    if x.dtype != torch.float32 or xs.dtype != torch.float32:
        raise RuntimeError("resblock1_fused: x and xs are fp32")
    if any(w.dtype != torch.bfloat16 for w in (*w1, *w2)):
        raise RuntimeError("resblock1_fused: bf16 weights (fs2_conv_weight_prep)")
    P = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
    d = (ctypes.c_int * 3)(*dilations)
    pw1, pw2, pb1, pb2 = P(w1), P(w2), P(b1), P(b2)
    rc = lib.fs2_resblock1_fused(ptr(x), rows, seq_len, channels, kernel_size,
                                 ctypes.addressof(d), ctypes.addressof(pw1), ctypes.addressof(pw2),
                                 ctypes.addressof(pb1), ctypes.addressof(pb2), ptr(xs), int(acc),
                                 float(scale), int(store_xs), ptr(hc), float(alpha2), ptr(lens),
                                 stream())
    return rc


def vocoder_post(x, rows, seq_len, c_in, w, bias, max_wav_value=32768.0, pcm=True, lens=None):
    _dev(x, w, bias, lens)
    wav = torch.empty(rows, dtype=torch.float32, device=x.device)
    p = torch.empty(rows, dtype=torch.int16, device=x.device) if pcm else None
    lib.fs2_vocoder_post(code(x.dtype), ptr(x), rows, seq_len, c_in, ptr(lens), ptr(w), ptr(bias),
                         max_wav_value, ptr(wav), ptr(p), stream())
    return wav, p


def weight_prep(w, c_out, c_in, taps, w_fwd=None, w_bwd=None):
    _dev(w)
    dt = (w_fwd if w_fwd is not None else w_bwd).dtype
    lib.fs2_conv_weight_prep(code(dt), ptr(w), c_out, c_in, taps, ptr(w_fwd), ptr(w_bwd), stream())


def conv_wgrad(dy, x, dw, rows, seq_len, c_in, c_out, taps, pad, db=None, ws_buf=None,
               on_stream=None, lens=None):
    """dw (+)= conv weight gradient; db (+)= column sums of dy when given (same launch).
    ``ws_buf``: caller-owned fp32 workspace (else one is allocated on the current stream)."""
    _dev(dy, x, dw, db)
    if dy.dtype != x.dtype:
        raise RuntimeError(f"conv_wgrad operand dtypes differ: {dy.dtype} vs {x.dtype}")
    n = lib.fs2_conv_wgrad_ws_bytes(rows, c_in, c_out, taps)
    if ws_buf is not None:
        if ws_buf.numel() * 4 < n:
            raise RuntimeError("conv_wgrad: workspace too small")
        w, n = ws_buf, ws_buf.numel() * 4
    else:
        w = ws(n, dy.device)
    lib.fs2_conv_wgrad(code(dy.dtype), ptr(dy), c_out, ptr(x), c_in, ptr(dw), ptr(db), rows,
                       seq_len, c_in, c_out, taps, pad, ptr(lens), ptr(w), n,
                       stream() if on_stream is None else on_stream)


def _k1_jobs(jobs):
    """ctypes int64 table {dy, ldy, x, ldx, dw, db, c_in, c_out} per job (host memory)."""
    arr = (ctypes.c_int64 * (8 * len(jobs)))()
    for j, (dy, x, dw, db, c_in, c_out) in enumerate(jobs):
        _dev(dy, x, dw, db)
        if dy.dtype != x.dtype:
            raise RuntimeError(f"conv_wgrad_k1_multi operand dtypes differ: {dy.dtype} vs {x.dtype}")
        arr[8 * j:8 * j + 8] = [dy.data_ptr(), c_out, x.data_ptr(), c_in, dw.data_ptr(),
                                0 if db is None else db.data_ptr(), c_in, c_out]
    return arr


def conv_wgrad_k1_multi_ws_bytes(jobs, rows):
    return lib.fs2_conv_wgrad_k1_multi_ws_bytes(_k1_jobs(jobs), len(jobs), rows)


def conv_wgrad_k1_multi(jobs, rows, seq_len, lens=None, ws_buf=None, on_stream=None):
    """Several k = 1 weight gradients over the same rows in one grouped launch:
    jobs = [(dy, x, dw, db_or_None, c_in, c_out), ...] (at most 4); dw (+)= dy^T x, db (+)=
    column sums of dy.  ``ws_buf``: caller-owned fp32 workspace."""
    arr = _k1_jobs(jobs)
    n = lib.fs2_conv_wgrad_k1_multi_ws_bytes(arr, len(jobs), rows)
    if ws_buf is not None:
        if ws_buf.numel() * 4 < n:
            raise RuntimeError("conv_wgrad_k1_multi: workspace too small")
        w, n = ws_buf, ws_buf.numel() * 4
    else:
        w = ws(n, jobs[0][0].device)
    lib.fs2_conv_wgrad_k1_multi(code(jobs[0][0].dtype), arr, len(jobs), rows, seq_len, ptr(lens),
                                ptr(w), n, stream() if on_stream is None else on_stream)


def colsum(x, rows, cols, out, accumulate=True):
    _dev(x, out)
    n = lib.fs2_colsum_ws_bytes(rows, cols)
    w = ws(n, x.device)
    lib.fs2_colsum(code(x.dtype), ptr(x), cols, rows, cols, ptr(out), int(accumulate), ptr(w), n,
                   stream())


def cast_bf16(x):
    _dev(x)
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    lib.fs2_cast_bf16(ptr(x), ptr(y), x.numel(), stream())
    return y


# ------------------------------------------------------------------ vocoder training
def _f32(name, *ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{name}: fp32 tensors expected, got {t.dtype}")


def conv_wgrad_dil(dy, x, dw, rows, seq_len, c_in, c_out, taps, pad, dilation=1, db=None,
                   ws_buf=None):
    """dw (c_out, c_in, taps) += the weight gradient of a dilated conv; db += column sums of dy
    when given (fs2_conv_wgrad_dil).  dy (rows, c_out) and x (rows, c_in) fp32 or bf16 (same)."""
    _dev(dy, x, dw, db, ws_buf)
    if dy.dtype != x.dtype:
        raise RuntimeError(f"conv_wgrad_dil operand dtypes differ: {dy.dtype} vs {x.dtype}")
    _f32("conv_wgrad_dil", dw, db)
    if dy.numel() != rows * c_out or x.numel() != rows * c_in or \
            dw.numel() != c_out * c_in * taps or (db is not None and db.numel() != c_out):
        raise RuntimeError("conv_wgrad_dil: dy (rows, c_out), x (rows, c_in), dw (c_out, c_in, taps), "
                           "db (c_out)")
    n = lib.fs2_conv_wgrad_dil_ws_bytes(rows, c_in, c_out, taps)
    if ws_buf is not None:
        if ws_buf.numel() * 4 < n:
            raise RuntimeError("conv_wgrad_dil: workspace too small")
        w, n = ws_buf, ws_buf.numel() * 4
    else:
        w = ws(n, dy.device)
    lib.fs2_conv_wgrad_dil(code(dy.dtype), ptr(dy), c_out, ptr(x), c_in, ptr(dw), ptr(db), rows,
                           seq_len, c_in, c_out, taps, pad, dilation, ptr(w), n, stream())


def lrelu_bwd(v, dy, alpha, out=None, accumulate=False):
    """dx (+)= dy * (v > 0 ? 1 : alpha) (fs2_lrelu_bwd): v fp32 or bf16, dy / dx fp32."""
    _dev(v, dy, out)
    _f32("lrelu_bwd", dy, out)
    if v.numel() != dy.numel():
        raise RuntimeError("lrelu_bwd: v and dy differ in size")
    if out is None:
        if accumulate:
            raise RuntimeError("lrelu_bwd: accumulate needs out")
        out = torch.empty(dy.shape, dtype=torch.float32, device=dy.device)
    elif out.numel() != dy.numel():
        raise RuntimeError("lrelu_bwd: out and dy differ in size")
    lib.fs2_lrelu_bwd(code(v.dtype), ptr(v), ptr(dy), ptr(out), dy.numel(), float(alpha),
                      int(bool(accumulate)), stream())
    return out


def vocoder_post_bwd(x, wav, d_wav, rows, seq_len, c_in, w, dw, db, want_dx=True):
    """Backward of ``vocoder_post`` (fs2_vocoder_post_bwd): returns dx (rows, c_in) fp32 (or
    None); dw (c_in * 7) and db (1) accumulate."""
    _dev(x, wav, d_wav, w, dw, db)
    _f32("vocoder_post_bwd", wav, d_wav, w, dw, db)
    if x.numel() != rows * c_in or wav.numel() != rows or d_wav.numel() != rows or \
            w.numel() != 7 * c_in or dw.numel() != 7 * c_in or db.numel() != 1:
        raise RuntimeError("vocoder_post_bwd: x (rows, c_in), wav / d_wav (rows), w / dw (c_in * 7), db (1)")
    dx = torch.empty(rows, c_in, dtype=torch.float32, device=x.device) if want_dx else None
    n = lib.fs2_vocoder_post_bwd_ws_bytes(rows, c_in)
    buf = ws(n, x.device)
    lib.fs2_vocoder_post_bwd(code(x.dtype), ptr(x), ptr(wav), ptr(d_wav), rows, seq_len, c_in,
                             ptr(w), ptr(dx), ptr(dw), ptr(db), ptr(buf), n, stream())
    return dx


def convT_wgrad_fold(dwc, dbc, dw, db, stride):
    """The phase-form gradient (stride * c_out, c_in, 3) added into the ConvTranspose1d layout
    dw (c_in, c_out, 2 * stride); db (c_out) += the phase sums of dbc (fs2_convT_wgrad_fold)."""
    _dev(dwc, dbc, dw, db)
    _f32("convT_wgrad_fold", dwc, dbc, dw, db)
    c_in, c_out, k = dw.shape
    if k != 2 * stride or dwc.numel() != stride * c_out * c_in * 3 or (dbc is None) != (db is None) or \
            (dbc is not None and (dbc.numel() != stride * c_out or db.numel() != c_out)):
        raise RuntimeError("convT_wgrad_fold: dwc (stride * c_out, c_in, 3), dw (c_in, c_out, 2 * stride)")
    lib.fs2_convT_wgrad_fold(ptr(dwc), ptr(dbc), c_in, c_out, stride, ptr(dw), ptr(db), stream())


def melspec_bwd(wav, lens, d_mel, hop, window, twiddle, fb, n_mels, n_fft=1024, out=None):
    """d_wav (B, S), the pull-back of d_mel (B, n_mels, F) through ``melspec``'s mel output
    (clip and log_mag off; fs2_melspec_bwd).  Operands as ``melspec`` takes them."""
    first, count, off, w = fb
    _dev(wav, lens, d_mel, window, twiddle, first, count, off, w, out)
    _f32("melspec_bwd", wav, d_mel, out)
    if wav.dim() != 2:
        raise RuntimeError("melspec_bwd: wav is f32 (B, S)")
    if lens is not None and (lens.dtype != torch.int64 or lens.numel() != wav.shape[0]):
        raise RuntimeError("melspec_bwd: lens is int64 (B)")
    _tables_f32("melspec_bwd", window, twiddle)
    if (first.dtype, count.dtype, off.dtype, w.dtype) != (torch.int32,) * 3 + (torch.float32,) or \
            not first.numel() == count.numel() == off.numel() == int(n_mels):
        raise RuntimeError("melspec_bwd: filterbank is (first, count, offset) int32 (n_mels) + f32 weights")
    B, S = wav.shape
    hop = int(hop)
    F = 1 + S // hop
    if d_mel.numel() != B * int(n_mels) * F:
        raise RuntimeError(f"melspec_bwd: d_mel is (B, n_mels, {F})")
    if out is None:
        out = torch.empty((B, S), dtype=torch.float32, device=wav.device)
    elif out.numel() != B * S:
        raise RuntimeError("melspec_bwd: out is f32 (B, S)")
    n = lib.fs2_melspec_bwd_ws_bytes(B, S, hop)
    buf = ws(n, wav.device)
    lib.fs2_melspec_bwd(ptr(wav), ptr(lens), B, S, int(n_fft), hop, ptr(window), ptr(twiddle),
                        ptr(first), ptr(count), ptr(off), ptr(w), w.numel(), int(n_mels),
                        ptr(d_mel), ptr(out), ptr(buf), n, stream())
    return out


def mel_l1(a, b, grad=True):
    """(loss (1,) = mean |a - b| on the device, d_a = sign(a - b) / N or None) (fs2_mel_l1)."""
    _dev(a, b)
    _f32("mel_l1", a, b)
    if a.numel() != b.numel() or a.numel() == 0:
        raise RuntimeError("mel_l1: a and b must have the same, non-zero size")
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    d_a = torch.empty(a.shape, dtype=torch.float32, device=a.device) if grad else None
    n = lib.fs2_mel_l1_ws_bytes()
    buf = ws(n, a.device)
    lib.fs2_mel_l1(ptr(a), ptr(b), a.numel(), ptr(loss), ptr(d_a), ptr(buf), n, stream())
    return loss, d_a


# ------------------------------------------------------------------ attention
def attn_fwd(qkv, lens, batch, seq_len, heads, d_head, scale):
    _dev(qkv, lens)
    o = torch.empty(batch * seq_len, heads * d_head, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(batch * heads, seq_len, dtype=torch.float32, device=qkv.device)
    lib.fs2_attn_fwd(code(qkv.dtype), ptr(qkv), ptr(o), ptr(lse), ptr(lens), batch, seq_len, heads,
                     d_head, scale, stream())
    return o, lse


def attn_bwd(qkv, o, d_o, lse, lens, batch, seq_len, heads, d_head, scale):
    _dev(qkv, o, d_o, lse, lens)
    if not (qkv.dtype == o.dtype == d_o.dtype):
        raise RuntimeError("attn_bwd operands must share a dtype")
    dqkv = torch.empty_like(qkv)
    n = lib.fs2_attn_bwd_ws_bytes(batch, seq_len, heads)
    w = ws(n, qkv.device)
    lib.fs2_attn_bwd(code(qkv.dtype), ptr(qkv), ptr(o), ptr(d_o), ptr(lse), ptr(dqkv), ptr(lens),
                     batch, seq_len, heads, d_head, scale, ptr(w), n, stream())
    return dqkv


# ------------------------------------------------------------------ LayerNorm
def ln_fwd(y, gamma, beta, res=None, lens=None, seq_len=1, p_in=0.0, p_out=0.0, seed=0,
           site_in=0, site_out=0, dot_w=None, dot_b=None, copy=None, res_ln=None, want_out=True):
    """Returns (out fp32, out compute copy or None, xhat, rstd, dot).  ``res_ln`` = (xhat,
    gamma, beta) of the LayerNorm that produced the residual, masked by the same ``lens``,
    instead of ``res`` (fs2_ln_fwd_nres: the residual is rebuilt, bitwise what that LayerNorm
    wrote, and its masked rows are never read).  ``want_out=False``: no fp32 output (None)."""
    rx, rg, rb = res_ln if res_ln is not None else (None, None, None)
    _dev(y, gamma, beta, res, lens, dot_w, dot_b, rx, rg, rb)
    rows, d = y.shape
    out = torch.empty_like(y) if want_out else None
    out_t = _copy(y.shape, copy, y.device)
    xhat = torch.empty_like(y)
    rstd = torch.empty(rows, dtype=torch.float32, device=y.device)
    dot = torch.empty(rows, dtype=torch.float32, device=y.device) if dot_w is not None else None
    sd = seed_arg(seed, y.device) if (p_in > 0 or p_out > 0) else None
    lib.fs2_ln_fwd_nres(BF16 if copy is not None else F32, ptr(y), ptr(res), ptr(rx), ptr(rg),
                        ptr(rb), ptr(gamma), ptr(beta), ptr(out), ptr(out_t), ptr(xhat), ptr(rstd),
                        ptr(lens), seq_len, rows, d, p_in, p_out, ptr(sd), site_in, site_out,
                        ptr(dot_w), ptr(dot_b), ptr(dot), stream())
    return out, out_t, xhat, rstd, dot


def ln_bwd(xhat, rstd, gamma, beta, dgamma, dbeta, dout=None, ddot=None, dot_w=None,
           dw_dot=None, db_dot=None, lens=None, seq_len=1, p_in=0.0, p_out=0.0, seed=0,
           site_in=0, site_out=0, relu_y=None, dres=None, copy=None, dbias_in=None,
           dres_add=True):
    """Returns (dy fp32, dy compute copy or None); dbias_in (+)= column sums of dy.
    With a compute copy the fp32 dy is not produced (None): only the copy feeds the GEMMs."""
    _dev(xhat, rstd, gamma, beta, dout, ddot, dot_w, relu_y, dres, lens)
    rows, d = xhat.shape
    dy = torch.empty_like(xhat) if copy is None else None
    dy_t = _copy(xhat.shape, copy, xhat.device)
    n = lib.fs2_ln_bwd_ws_bytes(rows, d)
    w = ws(n, xhat.device)
    sd = seed_arg(seed, xhat.device) if (p_in > 0 or p_out > 0) else None
    lib.fs2_ln_bwd(BF16 if copy is not None else F32, ptr(dout), ptr(ddot), ptr(dot_w), ptr(xhat),
                   ptr(rstd), ptr(gamma), ptr(beta), ptr(lens), seq_len, rows, d, p_in, p_out,
                   ptr(sd), site_in, site_out, ptr(relu_y), ptr(dy), ptr(dy_t), ptr(dres),
                   int(dres_add), ptr(dgamma), ptr(dbeta), ptr(dw_dot), ptr(db_dot), ptr(dbias_in),
                   ptr(w), n, stream())
    return dy, dy_t


# ------------------------------------------------------------------ BatchNorm
def bn_fwd(z, gamma, beta, running_mean, running_var, act_tanh, p, seed, site, res=None,
           eps=1e-5, momentum=0.1, copy=None, want_out=True, num_batches_tracked=None):
    """(out fp32 or None when only the copy is wanted, out copy or None, mean, rstd);
    ``num_batches_tracked`` (device int64) is incremented in the statistics launch."""
    _dev(z, gamma, beta, running_mean, running_var, res, num_batches_tracked)
    rows, c = z.shape
    out = torch.empty_like(z) if (want_out or copy is None) else None
    out_t = _copy(z.shape, copy, z.device)
    mean = torch.empty(c, dtype=torch.float32, device=z.device)
    rstd = torch.empty(c, dtype=torch.float32, device=z.device)
    n = lib.fs2_bn_ws_bytes(rows, c)
    w = ws(n, z.device)
    sd = seed_arg(seed, z.device) if p > 0 else None
    lib.fs2_bn_fwd(BF16 if copy is not None else F32, ptr(z), rows, c, ptr(gamma), ptr(beta), eps,
                   momentum, ptr(running_mean), ptr(running_var), ptr(mean), ptr(rstd),
                   int(act_tanh), p, ptr(sd), site, ptr(res), ptr(out), ptr(out_t), ptr(w), n,
                   ptr(num_batches_tracked), stream())
    return out, out_t, mean, rstd


def bn_eval_fwd(z, gamma, beta, running_mean, running_var, act_tanh, res=None, eps=1e-5,
                copy=None, want_out=True):
    """Eval-mode BatchNorm1d (running statistics, no dropout): (out or None, out copy or None)."""
    _dev(z, gamma, beta, running_mean, running_var, res)
    rows, c = z.shape
    out = torch.empty_like(z) if (want_out or copy is None) else None
    out_t = _copy(z.shape, copy, z.device)
    mean = torch.empty(c, dtype=torch.float32, device=z.device)
    rstd = torch.empty(c, dtype=torch.float32, device=z.device)
    lib.fs2_bn_eval_fwd(BF16 if copy is not None else F32, ptr(z), rows, c, ptr(gamma), ptr(beta),
                        eps, ptr(running_mean), ptr(running_var), ptr(mean), ptr(rstd),
                        int(act_tanh), ptr(res), ptr(out), ptr(out_t), stream())
    return out, out_t


def bn_bwd(dout, z, mean, rstd, gamma, beta, dgamma, dbeta, act_tanh, p, seed, site, copy=None):
    _dev(dout, z, mean, rstd, gamma, beta, dgamma, dbeta)
    rows, c = z.shape
    dz = torch.empty_like(z) if copy is None else None  # with a copy only it feeds the GEMMs
    dz_t = _copy(z.shape, copy, z.device)
    n = lib.fs2_bn_ws_bytes(rows, c)
    w = ws(n, z.device)
    sd = seed_arg(seed, z.device) if p > 0 else None
    lib.fs2_bn_bwd(BF16 if copy is not None else F32, ptr(dout), ptr(z), ptr(mean), ptr(rstd),
                   ptr(gamma), ptr(beta), rows, c, int(act_tanh), p, ptr(sd), site, ptr(dz),
                   ptr(dz_t), ptr(dgamma), ptr(dbeta), ptr(w), n, stream())
    return dz, dz_t


# ------------------------------------------------------------------ embeddings / adaptor
def encoder_embed(texts, accents, word_emb, accent_emb, posenc, batch, seq_len, d, copy=None):
    _dev(texts, accents, word_emb, accent_emb, posenc)
    out = torch.empty(batch * seq_len, d, dtype=torch.float32, device=word_emb.device)
    out_t = _copy(out.shape, copy, out.device)
    lib.fs2_encoder_embed_fwd(ptr(texts), ptr(accents), ptr(word_emb), ptr(accent_emb), ptr(posenc),
                              batch, seq_len, d, ptr(out), ptr(out_t), stream())
    return out, out_t


def embedding_fwd(ids, table):
    _dev(ids, table)
    n, d = ids.numel(), table.shape[1]
    out = torch.empty(n, d, dtype=torch.float32, device=table.device)
    lib.fs2_embedding_fwd(ptr(ids), ptr(table), n, d, ptr(out), stream())
    return out


def embedding_bwd(dout, ids, dtable, padding_idx=-1):
    _dev(dout, ids, dtable)
    n = lib.fs2_embedding_bwd_ws_bytes(ids.numel(), dtable.shape[1], dtable.shape[0])
    w = ws(n, dout.device)
    lib.fs2_embedding_bwd(ptr(dout), ptr(ids), ids.numel(), dtable.shape[1], padding_idx,
                          ptr(dtable), dtable.shape[0], ptr(w), n, stream())


def length_mask(lens, max_len):
    _dev(lens)
    m = torch.empty(lens.numel(), max_len, dtype=torch.bool, device=lens.device)
    lib.fs2_length_mask(ptr(lens), lens.numel(), max_len, ptr(m), stream())
    return m


def rowvec_add(x, ids, table, batch, seq_len, copy=None):
    _dev(x, ids, table)
    out = torch.empty_like(x)
    out_t = _copy(x.shape, copy, x.device)
    lib.fs2_rowvec_add_fwd(ptr(x), ptr(ids), ptr(table), batch, seq_len, x.shape[1], ptr(out),
                           ptr(out_t), stream())
    return out, out_t


def rowvec_add_bwd(dout, ids, dtable, batch, seq_len):
    _dev(dout, ids, dtable)
    lib.fs2_rowvec_add_bwd(ptr(dout), ptr(ids), batch, seq_len, dout.shape[1], ptr(dtable), stream())


def _vals_dtype(v):
    if v.dtype == torch.float32:
        return F32
    if v.dtype == torch.float64:
        return F64
    raise RuntimeError(f"bucketize values must be float32/float64, got {v.dtype}")


def bucket_embed(x, values, bins, table, copy=None):
    _dev(x, values, bins, table)
    rows, d = x.shape
    out = torch.empty_like(x)
    out_t = _copy(x.shape, copy, x.device)
    idx = torch.empty(rows, dtype=torch.int32, device=x.device)
    lib.fs2_bucket_embed_fwd(ptr(x), ptr(values), _vals_dtype(values), ptr(bins), bins.numel(),
                             ptr(table), rows, d, ptr(out), ptr(out_t), ptr(idx), stream())
    return out, out_t, idx


def bucket_embed_bwd(dout, idx, dtable):
    _dev(dout, idx, dtable)
    n = lib.fs2_embedding_bwd_ws_bytes(idx.numel(), dout.shape[1], dtable.shape[0])
    w = ws(n, dout.device)
    lib.fs2_bucket_embed_bwd(ptr(dout), ptr(idx), idx.numel(), dout.shape[1], ptr(dtable),
                             dtable.shape[0], ptr(w), n, stream())


def bucketize(values, bins):
    _dev(values, bins)
    idx = torch.empty(values.shape, dtype=torch.int32, device=values.device)
    lib.fs2_bucketize(ptr(values), _vals_dtype(values), ptr(bins), bins.numel(), values.numel(),
                      ptr(idx), stream())
    return idx


def lr_index(durations):
    _dev(durations)
    B, Ts = durations.shape
    if durations.dtype == torch.int64:
        dt = 0
    elif durations.dtype == torch.float32:
        dt = 1
    else:
        raise RuntimeError(f"durations must be int64 or float32, got {durations.dtype}")
    cum = torch.empty(B, Ts, dtype=torch.int32, device=durations.device)
    mel_len = torch.empty(B, dtype=torch.int64, device=durations.device)
    lib.fs2_lr_index(ptr(durations), dt, B, Ts, ptr(cum), ptr(mel_len), stream())
    return cum, mel_len


def duration_round(log_d, d_control=1.0):
    """Inference durations: clamp(round(exp(log_d) - 1) * d_control, min=0) (f32)."""
    _dev(log_d)
    if log_d.dtype != torch.float32:
        raise RuntimeError(f"log durations must be float32, got {log_d.dtype}")
    x = log_d.contiguous()
    out = torch.empty_like(x)
    lib.fs2_duration_round(ptr(x), x.numel(), float(d_control), ptr(out), stream())
    return out


def lr_source(cum, out_len):
    _dev(cum)
    B, Ts = cum.shape
    src = torch.empty(B, out_len, dtype=torch.int32, device=cum.device)
    lib.fs2_lr_source(ptr(cum), B, Ts, out_len, ptr(src), stream())
    return src


def lr_expand(x, cum, out_len, posenc=None, copy=None):
    _dev(x, cum, posenc)
    B, Ts = cum.shape
    d = x.shape[-1]
    out = torch.empty(B * out_len, d, dtype=torch.float32, device=x.device)
    out_t = _copy(out.shape, copy, x.device)
    lib.fs2_lr_expand_fwd(ptr(x), ptr(cum), B, Ts, out_len, d, ptr(posenc), ptr(out), ptr(out_t),
                          stream())
    return out, out_t


def lr_expand_embed(x, cum, out_len, pitch=None, energy=None, posenc=None, pos_len=None,
                    copy=None, want_pre=False, want_mid=False, want_out=True, want_idx=True):
    """Frame-level variance adaptor in one pass (fs2_lr_expand_embed_fwd): expand ``x`` by
    ``cum`` to ``out_len`` frames, add ``pitch`` / ``energy`` = (values (B, out_len), bins,
    table) embeddings (None: skipped) and ``posenc`` on the first ``pos_len`` frames.  Returns
    (pre, mid, out, out_t, p_idx, e_idx); what was not asked for is None and is not written.
    pre / mid (the frame-level predictors' inputs) are in ``copy`` when given, else fp32."""
    _dev(x, cum, posenc)
    B, Ts = cum.shape
    d = x.shape[-1]
    rows, dev = B * out_len, x.device
    pos_len = out_len if pos_len is None else int(pos_len)
    if posenc is not None and posenc.numel() < pos_len * d:
        raise RuntimeError(f"lr_expand_embed: position table shorter than {pos_len} frames")
    args = []
    for feat in (pitch, energy):
        if feat is None:
            args += [None, F32, None, 0, None]
            continue
        values, bins, table = feat
        _dev(values, bins, table)
        if values.numel() != rows or table.shape != (bins.numel() + 1, d):
            raise RuntimeError(f"lr_expand_embed: {tuple(values.shape)} values for {B} x {out_len} "
                               f"frames / {tuple(table.shape)} table for {bins.numel()} bins")
        args += [ptr(values), _vals_dtype(values), ptr(bins), bins.numel(), ptr(table)]
    cdt = torch.float32 if copy is None else copy
    pre = torch.empty(rows, d, dtype=cdt, device=dev) if want_pre else None
    mid = torch.empty(rows, d, dtype=cdt, device=dev) if want_mid else None
    out = torch.empty(rows, d, dtype=torch.float32, device=dev) if want_out else None
    out_t = _copy((rows, d), copy, dev) if want_out else None
    p_idx = torch.empty(rows, dtype=torch.int32, device=dev) if pitch is not None and want_idx else None
    e_idx = torch.empty(rows, dtype=torch.int32, device=dev) if energy is not None and want_idx else None
    lib.fs2_lr_expand_embed_fwd(ptr(x), ptr(cum), B, Ts, out_len, d, *args, ptr(posenc), pos_len,
                                code(cdt), ptr(pre), ptr(mid), ptr(out), ptr(out_t), ptr(p_idx),
                                ptr(e_idx), stream())
    return pre, mid, out, out_t, p_idx, e_idx


def lr_expand_bwd(dout, cum, out_len, d):
    _dev(dout, cum)
    B, Ts = cum.shape
    dx = torch.empty(B * Ts, d, dtype=torch.float32, device=dout.device)
    lib.fs2_lr_expand_bwd(ptr(dout), ptr(cum), B, Ts, out_len, d, ptr(dx), stream())
    return dx


# ------------------------------------------------------------------ losses / GMM
def fs2loss_fwd(mel_out, post_out, mel_tgt, p, e, logd, p_t, e_t, d_t, src_pad, mel_pad,
                denoms=None):
    _dev(mel_out, post_out, mel_tgt, p, e, logd, p_t, e_t, d_t, src_pad, mel_pad, denoms)
    B, Tm, n_mel = mel_out.shape
    Ts = p.shape[1]
    losses = torch.empty(6, dtype=torch.float32, device=mel_out.device)
    n = lib.fs2_fs2loss_ws_bytes(B, Tm)
    w = ws(n, mel_out.device)
    lib.fs2_fs2loss_fwd(ptr(mel_out), ptr(post_out), ptr(mel_tgt), mel_tgt.shape[1], ptr(p), ptr(e),
                        ptr(logd), ptr(p_t), ptr(e_t), ptr(d_t), ptr(src_pad), ptr(mel_pad), B, Ts,
                        Tm, n_mel, ptr(denoms), ptr(losses), ptr(w), n, stream())
    return losses, w


def fs2loss_bwd(mel_out, post_out, mel_tgt, p, e, logd, p_t, e_t, d_t, src_pad, mel_pad, w, g6):
    B, Tm, n_mel = mel_out.shape
    Ts = p.shape[1]
    outs = [torch.empty_like(t) for t in (mel_out, post_out, p, e, logd)]
    lib.fs2_fs2loss_bwd(ptr(mel_out), ptr(post_out), ptr(mel_tgt), mel_tgt.shape[1], ptr(p), ptr(e),
                        ptr(logd), ptr(p_t), ptr(e_t), ptr(d_t), ptr(src_pad), ptr(mel_pad), B, Ts,
                        Tm, n_mel, ptr(w), ptr(g6), *[ptr(o) for o in outs], stream())
    return outs


def _level_shapes(p, e, logd, mel_out, levels):
    B, Tm, _ = mel_out.shape
    Ts = logd.shape[1]
    for name, t, frame in (("pitch", p, levels[0]), ("energy", e, levels[1])):
        want = (B, Tm if frame else Ts)
        if tuple(t.shape) != want:
            raise RuntimeError(f"{'frame' if frame else 'phoneme'}-level {name} predictions are "
                               f"{tuple(t.shape)}, the mask is {want}")


def fs2loss_level_fwd(mel_out, post_out, mel_tgt, p, e, logd, p_t, e_t, d_t, src_pad, mel_pad,
                      levels, denoms=None):
    """fs2loss_fwd with ``levels = (pitch is frame-level, energy is frame-level)``: such a
    term's predictions / targets are (B, mel_len) under ``mel_pad``."""
    _dev(mel_out, post_out, mel_tgt, p, e, logd, p_t, e_t, d_t, src_pad, mel_pad, denoms)
    _level_shapes(p, e, logd, mel_out, levels)
    _level_shapes(p_t, e_t, logd, mel_out, levels)
    B, Tm, n_mel = mel_out.shape
    Ts = logd.shape[1]
    losses = torch.empty(6, dtype=torch.float32, device=mel_out.device)
    n = lib.fs2_fs2loss_ws_bytes(B, Tm)
    w = ws(n, mel_out.device)
    lib.fs2_fs2loss_level_fwd(ptr(mel_out), ptr(post_out), ptr(mel_tgt), mel_tgt.shape[1], ptr(p),
                              ptr(e), ptr(logd), ptr(p_t), ptr(e_t), ptr(d_t), ptr(src_pad),
                              ptr(mel_pad), B, Ts, Tm, n_mel, int(levels[0]), int(levels[1]),
                              ptr(denoms), ptr(losses), ptr(w), n, stream())
    return losses, w


def fs2loss_level_bwd(mel_out, post_out, mel_tgt, p, e, logd, p_t, e_t, d_t, src_pad, mel_pad,
                      levels, w, g6):
    B, Tm, n_mel = mel_out.shape
    Ts = logd.shape[1]
    outs = [torch.empty_like(t) for t in (mel_out, post_out, p, e, logd)]
    lib.fs2_fs2loss_level_bwd(ptr(mel_out), ptr(post_out), ptr(mel_tgt), mel_tgt.shape[1], ptr(p),
                              ptr(e), ptr(logd), ptr(p_t), ptr(e_t), ptr(d_t), ptr(src_pad),
                              ptr(mel_pad), B, Ts, Tm, n_mel, int(levels[0]), int(levels[1]),
                              ptr(w), ptr(g6), *[ptr(o) for o in outs], stream())
    return outs


def gmm_head_fwd(meta, w_pi, b_pi, w_s, b_s, w_mu, b_mu, K, D):
    _dev(meta, w_pi, b_pi, w_s, b_s, w_mu, b_mu)
    B, in_dim = meta.shape
    dev = meta.device
    pi = torch.empty(B, K, dtype=torch.float32, device=dev)
    sigma = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    mu = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    sigma_pre = torch.empty(B, K, D, dtype=torch.float32, device=dev)
    lib.fs2_gmm_head_fwd(ptr(meta), B, in_dim, K, D, ptr(w_pi), ptr(b_pi), ptr(w_s), ptr(b_s),
                         ptr(w_mu), ptr(b_mu), ptr(pi), ptr(sigma), ptr(mu), ptr(sigma_pre), stream())
    return pi, mu, sigma, sigma_pre


def gmm_logprob(e, pi, mu, sigma, want_mean=False, denom=None):
    _dev(e, pi, mu, sigma, denom)
    B, K, D = mu.shape
    logp = torch.empty(B, dtype=torch.float32, device=e.device)
    resp = torch.empty(B, K, dtype=torch.float32, device=e.device)
    mean = torch.empty((), dtype=torch.float32, device=e.device) if want_mean else None
    lib.fs2_gmm_logprob(ptr(e), ptr(pi), ptr(mu), ptr(sigma), B, K, D, ptr(logp), ptr(resp),
                        ptr(mean), ptr(denom), stream())
    return logp, resp, mean


def dp_counts(src_lens, mel_lens, src_len, mel_len, n_mel):
    _dev(src_lens, mel_lens)
    out = torch.empty(3, dtype=torch.float32, device=src_lens.device)
    lib.fs2_dp_counts(ptr(src_lens), ptr(mel_lens), src_lens.numel(), src_len, mel_len, n_mel,
                      ptr(out), stream())
    return out


def gmm_head_bwd(meta, e, pi, mu, sigma, sigma_pre, resp, g_logp, grads):
    B, K, D = mu.shape
    lib.fs2_gmm_head_bwd(ptr(meta), ptr(e), ptr(pi), ptr(mu), ptr(sigma), ptr(sigma_pre), ptr(resp),
                         ptr(g_logp), B, meta.shape[1], K, D, *[ptr(g) for g in grads], stream())


def gmm_sample(pi, mu, sigma, seed, offset=0):
    _dev(pi, mu, sigma)
    B, K, D = mu.shape
    out = torch.empty(B, D, dtype=torch.float32, device=mu.device)
    comp = torch.empty(B, dtype=torch.int32, device=mu.device)
    lib.fs2_gmm_sample(ptr(pi), ptr(mu), ptr(sigma), B, K, D, seed, offset, ptr(out), ptr(comp),
                       stream())
    return out, comp


# ------------------------------------------------------------------ optimiser / misc
def grad_norm(g, max_norm, norm_coef):
    n = lib.fs2_grad_norm_ws_bytes(g.numel())
    w = ws(n, g.device)
    lib.fs2_grad_norm(ptr(g), g.numel(), float(max_norm), ptr(norm_coef), ptr(w), n, stream())


def adam_step(p, g, m, v, norm_coef, lr, beta1, beta2, eps, bc1, bc2_sqrt, hyper=None):
    """Adam over flat buffers; with ``hyper`` (device [lr, bc1, bc2_sqrt], see sched_step) the
    scalar lr/bc1/bc2_sqrt arguments are ignored."""
    lib.fs2_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(norm_coef), float(lr),
                      float(beta1), float(beta2), float(eps), float(bc1), float(bc2_sqrt),
                      ptr(hyper), stream())


def adam_l2_step(p, g, m, v, norm_coef, lr, beta1, beta2, eps, weight_decay, step, hyper,
                 gate=None):
    """torch.optim.Adam with coupled L2 weight decay over flat buffers (fs2_adam_l2_step):
    ``step`` device int64[1], ``hyper`` device float[3] scratch; a ``gate`` (device float) of 0
    skips the call on the device, step count included."""
    _dev(p, g, m, v, norm_coef, step, hyper, gate)
    lib.fs2_adam_l2_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(norm_coef), float(lr),
                         float(beta1), float(beta2), float(eps), float(weight_decay), ptr(step),
                         ptr(hyper), ptr(gate), stream())


def gate_lt(x, threshold):
    """Device float 1.0 where x < threshold, else 0.0 (no host sync)."""
    _dev(x)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    lib.fs2_gate_lt(ptr(x), float(threshold), ptr(out), stream())
    return out


def lstm_stack_wgrad(x, h, dgates, n_seq, steps, dw_ih0, dw_ih_up, dw_hh, db, beta=0):
    """Weight gradients of the LSTM stack from x (rows, c_in), h (L, rows, H) and dgates
    (L, rows, 4H), into the stack-layout outputs (fs2_lstm_stack_wgrad)."""
    _dev(x, h, dgates, dw_ih0, dw_ih_up, dw_hh, db)
    L, _, H = h.shape
    c_in = x.shape[-1]
    n = lib.fs2_lstm_stack_wgrad_ws_bytes(n_seq, steps, c_in, H, L)
    w = ws(n, x.device)
    lib.fs2_lstm_stack_wgrad(ptr(x), ptr(h), ptr(dgates), n_seq, steps, c_in, H, L, ptr(dw_ih0),
                             ptr(dw_ih_up), ptr(dw_hh), ptr(db), int(beta), ptr(w), n, stream())


def ge2e_softmax(emb, w, b, g=None, grads=False):
    """GE2E softmax loss of emb (N, M, D); with ``grads`` also (demb, dw, db) scaled by the
    device scalar ``g`` (fs2_ge2e_softmax)."""
    _dev(emb, g)
    N, M, D = emb.shape
    dev = emb.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    demb = torch.empty_like(emb) if grads else None
    dw = torch.empty((), dtype=torch.float32, device=dev) if grads else None
    db = torch.empty((), dtype=torch.float32, device=dev) if grads else None
    n = lib.fs2_ge2e_softmax_ws_bytes(N, M, D)
    wk = ws(n, dev)
    lib.fs2_ge2e_softmax(ptr(emb), N, M, D, ptr(w), ptr(b), ptr(g), ptr(loss), ptr(demb), ptr(dw),
                         ptr(db), ptr(wk), n, stream())
    return (loss, demb, dw, db) if grads else loss


def ge2e_contrast(emb, w, b, g=None, grads=False):
    """GE2E contrast loss of emb (N, M, D); with ``grads`` also (demb, dw, db) scaled by the
    device scalar ``g`` (fs2_ge2e_contrast).  Off the GPU there is no path: ``NotImplementedError`` (a
    ``RuntimeError``), as ``GE2ELoss(loss='contrast')`` raised there before the kernel existed."""
    if not emb.is_cuda:
        raise NotImplementedError("ge2e_contrast needs tensors on the GPU (no CPU path exists)")
    _dev(emb, g)
    N, M, D = emb.shape
    dev = emb.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    demb = torch.empty_like(emb) if grads else None
    dw = torch.empty((), dtype=torch.float32, device=dev) if grads else None
    db = torch.empty((), dtype=torch.float32, device=dev) if grads else None
    n = lib.fs2_ge2e_contrast_ws_bytes(N, M, D)
    wk = ws(n, dev)
    lib.fs2_ge2e_contrast(ptr(emb), N, M, D, ptr(w), ptr(b), ptr(g), ptr(loss), ptr(demb), ptr(dw),
                          ptr(db), ptr(wk), n, stream())
    return (loss, demb, dw, db) if grads else loss


def mel_crop_gather(store, row_off, row_stride, row_start, n_mels, length, out=None):
    """out[r, t, c] = store[row_off[r] + c * row_stride[r] + row_start[r] + t]: crop, transpose
    and stack utterances of a flat (n_mels, frames)-per-utterance corpus into (rows, length,
    n_mels) (fs2_mel_crop_gather).  Descriptors: device int64 / int32 / int32, one per row."""
    _dev(store, row_off, row_stride, row_start, out)
    n = row_off.numel()
    if (store.dtype, row_off.dtype, row_stride.dtype, row_start.dtype) != (
            torch.float32, torch.int64, torch.int32, torch.int32):
        raise RuntimeError("mel_crop_gather: store f32, row_off i64, row_stride / row_start i32")
    if row_stride.numel() != n or row_start.numel() != n:
        raise RuntimeError("mel_crop_gather: one descriptor of each kind per row")
    if out is None:
        out = torch.empty((n, int(length), int(n_mels)), dtype=torch.float32, device=store.device)
    elif out.numel() != n * int(length) * int(n_mels) or out.dtype != torch.float32:
        raise RuntimeError("mel_crop_gather: out is not f32 (rows, length, n_mels)")
    lib.fs2_mel_crop_gather(ptr(store), ptr(row_off), ptr(row_stride), ptr(row_start), n,
                            int(n_mels), int(length), ptr(out), stream())
    return out


def rows_mean_unit(x, seg_start):
    """x (rows, dim), seg_start device int64 (n_seg + 1) -> (n_seg, dim): each segment's mean
    row scaled to unit length (fs2_rows_mean_unit)."""
    _dev(x, seg_start)
    if x.dtype != torch.float32 or seg_start.dtype != torch.int64 or x.dim() != 2:
        raise RuntimeError("rows_mean_unit: x f32 (rows, dim), seg_start i64")
    n_seg = seg_start.numel() - 1
    out = torch.empty((n_seg, x.shape[1]), dtype=torch.float32, device=x.device)
    lib.fs2_rows_mean_unit(ptr(x), ptr(seg_start), n_seg, x.shape[1], ptr(out), stream())
    return out


# ------------------------------------------------------------------ exact t-SNE
def empty_f64(shape, device):
    return torch.empty(shape, dtype=torch.float64, device=device)


def _tsne_y(name, *ts):
    _dev(*ts)
    for t in ts:
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2 or t.shape != ts[0].shape:
            raise RuntimeError(f"{name}: embeddings, updates and gains are f32 (n, 2)")
    return ts[0].shape[0]


def _tsne_p(name, P, n, *f64s):
    _dev(P, *f64s)
    if P.dtype != torch.float32 or tuple(P.shape) != (n, n):
        raise RuntimeError(f"{name}: P is f32 ({n}, {n})")
    for t in f64s:
        if t.dtype != torch.float64 or t.numel() < n:
            raise RuntimeError(f"{name}: the row buffers are f64 with at least {n} elements")


def _tsne_state(name, state):
    _dev(state)
    if state.dtype != torch.float64 or state.numel() != 16:
        raise RuntimeError(f"{name}: state is f64[16] (tsne_state)")


def tsne_points(x, seg_start, cap):
    """x (rows, dim), seg_start device int64 (n + 1) -> (n, dim): the plain mean of each
    segment's first ``cap`` rows (fs2_tsne_points)."""
    _dev(x, seg_start)
    if x.dtype != torch.float32 or seg_start.dtype != torch.int64 or x.dim() != 2:
        raise RuntimeError("tsne_points: x f32 (rows, dim), seg_start i64")
    n = seg_start.numel() - 1
    out = torch.empty((n, x.shape[1]), dtype=torch.float32, device=x.device)
    lib.fs2_tsne_points(ptr(x), ptr(seg_start), n, x.shape[1], int(cap), ptr(out), stream())
    return out


def _tsne_x(name, X):
    _dev(X)
    if X.dtype != torch.float32 or X.dim() != 2:
        raise RuntimeError(f"{name}: X is f32 (n, dim)")
    return X.shape


def tsne_pca_init(X):
    """X (n, dim) -> Y0 (n, 2): the two leading principal components, the first scaled to
    standard deviation 1e-4 (fs2_tsne_pca_init)."""
    n, dim = _tsne_x("tsne_pca_init", X)
    Y0 = torch.empty((n, 2), dtype=torch.float32, device=X.device)
    nb = lib.fs2_tsne_pca_ws_bytes(n, dim)
    wk = empty_f64(max(nb // 8, 1), X.device)
    lib.fs2_tsne_pca_init(ptr(X), n, dim, ptr(Y0), ptr(wk), nb, stream())
    return Y0


def tsne_affinities(X, perplexity, want64=False):
    """X (n, dim) -> the joint probabilities P (n, n) f32 of exact t-SNE; with ``want64`` also
    beta (n) and P before its rounding, both f64 (fs2_tsne_affinities)."""
    n, dim = _tsne_x("tsne_affinities", X)
    dev = X.device
    P = torch.empty((n, n), dtype=torch.float32, device=dev)
    beta = empty_f64(n, dev) if want64 else None
    P64 = empty_f64((n, n), dev) if want64 else None
    nb = lib.fs2_tsne_affinities_ws_bytes(n)
    wk = empty_f64(max(nb // 8, 1), dev)
    lib.fs2_tsne_affinities(ptr(X), n, dim, float(perplexity), ptr(P), ptr(beta), ptr(P64),
                            ptr(wk), nb, stream())
    return (P, beta, P64) if want64 else P


def tsne_state(n, perplexity, max_iter, exploration_iter, n_iter_without_progress,
               early_exaggeration, learning_rate, min_grad_norm, device):
    """The descent's device record, f64[16] (fs2_tsne_state_init)."""
    state = empty_f64(16, device)
    lib.fs2_tsne_state_init(ptr(state), int(n), float(perplexity), int(max_iter),
                            int(exploration_iter), int(n_iter_without_progress),
                            float(early_exaggeration), float(learning_rate), float(min_grad_norm),
                            stream())
    return state


def tsne_rowsum(Y, state, rowsum):
    """Phase A of an iteration: rowsum (n) f64 = the rows' sums of w (fs2_tsne_rowsum)."""
    n = _tsne_y("tsne_rowsum", Y)
    _tsne_state("tsne_rowsum", state)
    if rowsum.dtype != torch.float64 or rowsum.numel() < n or not rowsum.is_cuda:
        raise RuntimeError(f"tsne_rowsum: rowsum is f64 with at least {n} elements")
    lib.fs2_tsne_rowsum(ptr(Y), n, ptr(state), ptr(rowsum), stream())


def tsne_update(P, Y, Y_out, update, gains, it, state, rowsum, kl_rows, gn_rows):
    """Phase B of iteration ``it``: gradient, gains, update and Y_out = Y + update; stage,
    exaggeration and momentum come from ``state`` (fs2_tsne_update)."""
    n = _tsne_y("tsne_update", Y, Y_out, update, gains)
    _tsne_p("tsne_update", P, n, rowsum, kl_rows, gn_rows)
    _tsne_state("tsne_update", state)
    lib.fs2_tsne_update(ptr(P), ptr(Y), ptr(Y_out), ptr(update), ptr(gains), n, int(it),
                        ptr(state), ptr(rowsum), ptr(kl_rows), ptr(gn_rows), stream())


def tsne_control(state, n, it, kl_rows, gn_rows):
    """The stopping and stage rules for iteration ``it`` on the record (fs2_tsne_control)."""
    _tsne_state("tsne_control", state)
    _dev(kl_rows, gn_rows)
    if min(kl_rows.numel(), gn_rows.numel()) < n or kl_rows.dtype != torch.float64 or \
            gn_rows.dtype != torch.float64:
        raise RuntimeError(f"tsne_control: the row buffers are f64 with at least {n} elements")
    lib.fs2_tsne_control(ptr(state), int(n), int(it), ptr(kl_rows), ptr(gn_rows), stream())


def tsne_step(P, Y, update, gains, exaggeration, momentum, learning_rate):
    """One iteration on explicit state: (Y', kl_rows (n) f64, gn_rows (n) f64); ``update`` and
    ``gains`` are advanced in place (fs2_tsne_step)."""
    n = _tsne_y("tsne_step", Y, update, gains)
    _tsne_p("tsne_step", P, n)
    dev = Y.device
    Y_out = torch.empty_like(Y)
    rowsum, kl_rows, gn_rows = empty_f64(n, dev), empty_f64(n, dev), empty_f64(n, dev)
    lib.fs2_tsne_step(ptr(P), ptr(Y), ptr(Y_out), ptr(update), ptr(gains), n, float(exaggeration),
                      float(momentum), float(learning_rate), ptr(rowsum), ptr(kl_rows),
                      ptr(gn_rows), stream())
    return Y_out, kl_rows, gn_rows


def tsne_kl(P, Y, exaggeration=1.0):
    """The objective of Y (n, 2) under ``exaggeration * P``: f64[1] on the device (fs2_tsne_kl)."""
    n = _tsne_y("tsne_kl", Y)
    _tsne_p("tsne_kl", P, n)
    dev = Y.device
    rowsum, kl_rows, kl = empty_f64(n, dev), empty_f64(n, dev), empty_f64(1, dev)
    lib.fs2_tsne_kl(ptr(P), ptr(Y), n, float(exaggeration), ptr(rowsum), ptr(kl_rows), ptr(kl),
                    stream())
    return kl


def tsne_finish(Y):
    """(Y - min) / (max - min) per column (fs2_tsne_finish)."""
    n = _tsne_y("tsne_finish", Y)
    out = torch.empty_like(Y)
    lib.fs2_tsne_finish(ptr(Y), n, ptr(out), stream())
    return out


def melspec(wav, lens, hop, window, twiddle, fb, n_mels, clip=False, energy=True, mag=False,
            log_mag=False, n_fft=1024, out=None):
    """The mel front end of a ragged batch (fs2_melspec): wav (B, S) f32, lens device int64 (B)
    or None -> ``(mel (B, n_mels, F), energy (B, F) or None, mag (B, 513, F) or None,
    n_frames (B) int64)``, F = 1 + S // hop, zeros at frames past ``n_frames``.  ``fb`` is the
    compressed filterbank ``(first, count, offset, weights)`` on the device (int32 x 3, f32);
    ``window`` (1024) and ``twiddle`` (1024, 2) f32.  ``out`` = preallocated
    ``(mel, energy, mag, n_frames)`` (energy / mag may be None there)."""
    first, count, off, w = fb
    _dev(wav, lens, window, twiddle, first, count, off, w)
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise RuntimeError("melspec: wav is f32 (B, S)")
    if lens is not None and (lens.dtype != torch.int64 or lens.numel() != wav.shape[0]):
        raise RuntimeError("melspec: lens is int64 (B)")
    _tables_f32("melspec", window, twiddle)
    if (first.dtype, count.dtype, off.dtype, w.dtype) != (torch.int32,) * 3 + (torch.float32,) or \
            not first.numel() == count.numel() == off.numel() == int(n_mels):
        raise RuntimeError("melspec: filterbank is (first, count, offset) int32 (n_mels) + f32 weights")
    B, S = wav.shape
    hop = int(hop)
    if not 1 <= hop <= 1024:
        raise RuntimeError(f"melspec: hop {hop} (1..1024)")
    F, dev = 1 + S // hop, wav.device
    if out is None:
        out = (torch.empty((B, int(n_mels), F), dtype=torch.float32, device=dev),
               torch.empty((B, F), dtype=torch.float32, device=dev) if energy else None,
               torch.empty((B, 513, F), dtype=torch.float32, device=dev) if mag else None,
               torch.empty(B, dtype=torch.int64, device=dev))
    mel_o, en_o, mag_o, nf_o = out
    _dev(mel_o, en_o, mag_o, nf_o)
    if mel_o.dtype != torch.float32 or mel_o.numel() != B * int(n_mels) * F or \
            (en_o is not None and (en_o.dtype != torch.float32 or en_o.numel() != B * F)) or \
            (mag_o is not None and (mag_o.dtype != torch.float32 or mag_o.numel() != B * 513 * F)) or \
            nf_o.dtype != torch.int64 or nf_o.numel() != B:
        raise RuntimeError("melspec: out is (mel (B, n_mels, F), energy (B, F), mag (B, 513, F)) "
                           "f32 and n_frames (B) int64")
    lib.fs2_melspec(ptr(wav), ptr(lens), B, S, int(n_fft), hop, ptr(window), ptr(twiddle),
                    ptr(first), ptr(count), ptr(off), ptr(w), w.numel(), int(n_mels), int(bool(clip)),
                    int(bool(log_mag)), ptr(mel_o), ptr(en_o), ptr(mag_o), ptr(nf_o), stream())
    return mel_o, en_o, mag_o, nf_o


def _spec_f32(name, bins, n_frames, *specs):
    """(B, bins, frames) f32 operands (None allowed after the first) and the live counts."""
    _dev(n_frames, *specs)
    first = specs[0]
    if first.dim() != 3 or first.shape[1] != bins:
        raise RuntimeError(f"{name}: the spectrogram is f32 (B, {bins}, frames)")
    for s in specs:
        if s is not None and (s.dtype != torch.float32 or s.shape != first.shape):
            raise RuntimeError(f"{name}: the spectrograms are f32 {tuple(first.shape)}")
    if n_frames is not None and (n_frames.dtype != torch.int64 or n_frames.numel() != first.shape[0]):
        raise RuntimeError(f"{name}: n_frames is int64 (B)")
    if first.shape[2] < 1:
        raise RuntimeError(f"{name}: no frames")
    return first.shape[0], first.shape[2]


def _tables_f32(name, window, twiddle):
    _dev(window, twiddle)
    if window.dtype != torch.float32 or window.numel() != 1024 or \
            twiddle.dtype != torch.float32 or twiddle.numel() != 2048:
        raise RuntimeError(f"{name}: window f32 (1024), twiddle f32 (1024, 2)")


def griffin_lim_ws(batch, frames, device):
    """The frame workspace of ``istft`` / ``griffin_lim_step`` (fs2_griffin_lim_ws_bytes)."""
    return ws(lib.fs2_griffin_lim_ws_bytes(int(batch), int(frames)), device)


def mel_to_linear(mel, n_frames, inv_basis, out=None):
    """``TacotronSTFT._mel_to_linear`` on LOG-mels (fs2_mel_to_linear): mel (B, n_mels, F) f32,
    n_frames device int64 (B) or None, inv_basis (513, n_mels) f32 ->
    ``max(inv_basis @ exp(mel), 1e-10)`` (B, 513, F), zeros at frames past ``n_frames``."""
    B, F = _spec_f32("mel_to_linear", mel.shape[1] if mel.dim() == 3 else -1, n_frames, mel)
    _dev(inv_basis, out)
    n_mels = mel.shape[1]
    if inv_basis.dtype != torch.float32 or tuple(inv_basis.shape) != (513, n_mels):
        raise RuntimeError(f"mel_to_linear: inv_basis is f32 (513, {n_mels})")
    if out is None:
        out = torch.empty((B, 513, F), dtype=torch.float32, device=mel.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 513, F):
        raise RuntimeError("mel_to_linear: out is f32 (B, 513, F)")
    lib.fs2_mel_to_linear(ptr(mel), ptr(n_frames), B, n_mels, F, ptr(inv_basis), ptr(out), stream())
    return out


def _wav_out(name, out, B, F, hop, dev):
    cols = max(hop, 0) * (F - 1)
    if out is None:
        return torch.empty((B, cols), dtype=torch.float32, device=dev)
    _dev(out)
    if out.dtype != torch.float32 or tuple(out.shape) != (B, cols):
        raise RuntimeError(f"{name}: the waveform is f32 (B, hop (frames - 1)) = ({B}, {cols})")
    return out


def _gl_ws(name, ws_buf, B, F, dev):
    n = lib.fs2_griffin_lim_ws_bytes(B, F)
    if ws_buf is None:
        return ws(n, dev), n
    _dev(ws_buf)
    if ws_buf.dtype != torch.float32 or ws_buf.numel() * 4 < n:
        raise RuntimeError(f"{name}: the workspace is f32 of {n} bytes (griffin_lim_ws)")
    return ws_buf, ws_buf.numel() * 4


def istft(mag, phase, n_frames, hop, window, twiddle, n_fft=1024, out=None, ws_buf=None):
    """``STFT.inverse`` of a ragged batch (fs2_istft): mag, phase (None = zero phase)
    (B, 513, F) f32, n_frames device int64 (B) or None -> wav (B, hop (F - 1)) f32, row b live
    up to ``hop (n_frames[b] - 1)`` and zeros after.  ``window`` (1024), ``twiddle`` (1024, 2)
    f32; ``ws_buf`` = a caller-owned ``griffin_lim_ws`` (else one is allocated)."""
    B, F = _spec_f32("istft", 513, n_frames, mag, phase)
    _tables_f32("istft", window, twiddle)
    hop = int(hop)
    wav = _wav_out("istft", out, B, F, hop, mag.device)
    w, n = _gl_ws("istft", ws_buf, B, F, mag.device)
    lib.fs2_istft(ptr(mag), ptr(phase), ptr(n_frames), B, F, int(n_fft), hop, ptr(window),
                  ptr(twiddle), ptr(wav), ptr(w), n, stream())
    return wav


def griffin_lim_step(wav_in, mag, n_frames, hop, window, twiddle, n_fft=1024, out=None,
                     ws_buf=None):
    """One Griffin-Lim pass (fs2_griffin_lim_step): the STFT of wav_in (B, hop (F - 1)) f32, its
    magnitudes replaced by ``mag`` (B, 513, F), inverted -> a new waveform of that shape.
    ``out`` must not be ``wav_in``."""
    B, F = _spec_f32("griffin_lim_step", 513, n_frames, mag)
    _tables_f32("griffin_lim_step", window, twiddle)
    hop = int(hop)
    if wav_in is None:
        raise RuntimeError("griffin_lim_step: wav_in is missing")
    wav_in = _wav_out("griffin_lim_step", wav_in, B, F, hop, mag.device)
    wav = _wav_out("griffin_lim_step", out, B, F, hop, mag.device)
    w, n = _gl_ws("griffin_lim_step", ws_buf, B, F, mag.device)
    lib.fs2_griffin_lim_step(ptr(wav_in), ptr(mag), ptr(n_frames), B, F, int(n_fft), hop,
                             ptr(window), ptr(twiddle), ptr(wav), ptr(w), n, stream())
    return wav


def _rows_f32(name, x, n):
    _dev(x, n)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise RuntimeError(f"{name}: values are f32 (B, cols)")
    if n is not None and (n.dtype != torch.int64 or n.numel() != x.shape[0]):
        raise RuntimeError(f"{name}: the live counts are int64 (B)")


def f0_yin(wav, lens, hop, sr, f0_floor=71.0, f0_ceil=800.0, threshold=0.15, out=None):
    """The YIN F0 contour of a ragged batch (fs2_f0_yin): wav (B, S) f32, lens device int64 (B) or
    None -> ``(f0 (B, F), dip (B, F), n_frames (B) int64)``, F = 1 + S // hop, zeros at frames
    past ``n_frames``.  ``out`` = preallocated ``(f0, dip, n_frames)``."""
    _rows_f32("f0_yin", wav, lens)
    B, S = wav.shape
    hop = int(hop)
    if not 1 <= hop <= 1024:
        raise RuntimeError(f"f0_yin: hop {hop} (1..1024)")
    F, dev = 1 + S // hop, wav.device
    if out is None:
        out = (torch.empty((B, F), dtype=torch.float32, device=dev),
               torch.empty((B, F), dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int64, device=dev))
    f0, dip, nf = out
    _dev(f0, dip, nf)
    if f0.dtype != torch.float32 or dip.dtype != torch.float32 or f0.numel() != B * F or \
            dip.numel() != B * F or nf.dtype != torch.int64 or nf.numel() != B:
        raise RuntimeError("f0_yin: out is (f0 (B, F), dip (B, F)) f32 and n_frames (B) int64")
    lib.fs2_f0_yin(ptr(wav), ptr(lens), B, S, hop, float(sr), float(f0_floor), float(f0_ceil),
                   float(threshold), ptr(f0), ptr(dip), ptr(nf), stream())
    return f0, dip, nf


def _pyin_table(name, what, t, dtype, numel, dev):
    _dev(t)
    if t.dtype != dtype or t.dim() != 1 or t.numel() != numel or t.device != dev:
        raise RuntimeError(f"{name}: {what} is {str(dtype).split('.')[-1]} ({numel}) on {dev}")


def _pyin_hop(name, hop):
    hop = int(hop)
    if not 1 <= hop <= 1024:
        raise RuntimeError(f"{name}: hop {hop} (1..1024)")
    return hop


def f0_pyin_candidates(wav, lens, hop, sr, f0_floor, f0_ceil, prior, n_bins):
    """The first stage of pYIN (fs2_f0_pyin_candidates): wav (B, S) f32, lens device int64 (B) or
    None, ``prior`` device f64 (100) -> ``(mass (B, F, n_bins) f64, cand_f0 (B, F, n_bins) f32,
    voiced (B, F) f64, unvoiced (B, F) f32, n_frames (B) int64)``, F = 1 + S // hop,
    ``n_bins`` as ``audio.pyin_tables`` counts them; zeros past ``n_frames``."""
    _rows_f32("f0_pyin_candidates", wav, lens)
    B, S = wav.shape
    hop, dev = _pyin_hop("f0_pyin_candidates", hop), wav.device
    _pyin_table("f0_pyin_candidates", "prior", prior, torch.float64, 100, dev)
    F, nb = 1 + S // hop, int(n_bins)
    if not 1 <= nb <= 1024:
        raise RuntimeError(f"f0_pyin_candidates: {nb} pitch bins (1..1024)")
    mass = torch.empty((B, F, nb), dtype=torch.float64, device=dev)
    cf0 = torch.empty((B, F, nb), dtype=torch.float32, device=dev)
    voiced = torch.empty((B, F), dtype=torch.float64, device=dev)
    unvoiced = torch.empty((B, F), dtype=torch.float32, device=dev)
    nf = torch.empty(B, dtype=torch.int64, device=dev)
    lib.fs2_f0_pyin_candidates(ptr(wav), ptr(lens), B, S, hop, float(sr), float(f0_floor),
                               float(f0_ceil), ptr(prior), nb, ptr(mass), ptr(cf0), ptr(voiced),
                               ptr(unvoiced), ptr(nf), stream())
    return mass, cf0, voiced, unvoiced, nf


def f0_pyin_viterbi(mass, voiced, n_frames, tri, cand_f0=None, centres=None):
    """The second stage of pYIN (fs2_f0_pyin_viterbi): mass (B, F, n_bins) f64, voiced (B, F) f64,
    n_frames device int64 (B) or None, ``tri`` device f64 (R + 1) -> ``path (B, F) int32`` (state
    b = voiced bin b, n_bins + b = unvoiced; -1 past ``n_frames``); with ``cand_f0`` (B, F, n_bins)
    f32 and ``centres`` (n_bins) f32 also the contour: ``(path, f0 (B, F) f32)``."""
    _dev(mass, voiced, n_frames, tri, cand_f0, centres)
    if mass.dtype != torch.float64 or mass.dim() != 3 or voiced.dtype != torch.float64 or \
            tuple(voiced.shape) != tuple(mass.shape[:2]):
        raise RuntimeError("f0_pyin_viterbi: mass (B, F, n_bins) and voiced (B, F) are f64")
    B, F, nb = mass.shape
    dev = mass.device
    if n_frames is not None:
        _lens_i64("f0_pyin_viterbi", n_frames, B)
    if tri.dtype != torch.float64 or tri.dim() != 1 or tri.numel() < 1:
        raise RuntimeError("f0_pyin_viterbi: tri is f64 (R + 1)")
    if (cand_f0 is None) != (centres is None):
        raise RuntimeError("f0_pyin_viterbi: cand_f0 and centres come as a pair or not at all")
    f0 = None
    if cand_f0 is not None:
        if cand_f0.dtype != torch.float32 or tuple(cand_f0.shape) != (B, F, nb):
            raise RuntimeError(f"f0_pyin_viterbi: cand_f0 is f32 ({B}, {F}, {nb})")
        _pyin_table("f0_pyin_viterbi", "centres", centres, torch.float32, nb, dev)
        f0 = torch.empty((B, F), dtype=torch.float32, device=dev)
    path = torch.empty((B, F), dtype=torch.int32, device=dev)
    nbytes = lib.fs2_f0_pyin_viterbi_ws_bytes(B, F, nb)
    wk = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    lib.fs2_f0_pyin_viterbi(ptr(mass), ptr(voiced), ptr(n_frames), B, F, nb, ptr(tri),
                            tri.numel() - 1, ptr(cand_f0), ptr(centres), ptr(path), ptr(f0), ptr(wk),
                            nbytes, stream())
    return path if f0 is None else (path, f0)


def f0_pyin(wav, lens, hop, sr, f0_floor, f0_ceil, prior, tri, centres, out=None, states=False):
    """The pYIN F0 contour of a ragged batch (fs2_f0_pyin): wav (B, S) f32, lens device int64 (B)
    or None; the device tables of ``audio.pyin_tables``: ``prior`` f64 (100), ``tri`` f64 (R + 1),
    ``centres`` f32 (n_bins) -> ``(f0 (B, F), unvoiced (B, F), n_frames (B) int64)``,
    F = 1 + S // hop, zeros past ``n_frames``; ``unvoiced`` = 1 - the voiced prior mass (small
    means strongly periodic).  ``out`` = preallocated ``(f0, unvoiced, n_frames)``;
    ``states=True`` appends the decoded states (B, F) int32."""
    _rows_f32("f0_pyin", wav, lens)
    B, S = wav.shape
    hop, dev = _pyin_hop("f0_pyin", hop), wav.device
    _pyin_table("f0_pyin", "prior", prior, torch.float64, 100, dev)
    _dev(tri, centres)
    if tri.dtype != torch.float64 or tri.dim() != 1 or tri.numel() < 1:
        raise RuntimeError("f0_pyin: tri is f64 (R + 1)")
    if centres.dtype != torch.float32 or centres.dim() != 1 or centres.numel() < 1:
        raise RuntimeError("f0_pyin: centres is f32 (n_bins)")
    F, nb = 1 + S // hop, centres.numel()
    if out is None:
        out = (torch.empty((B, F), dtype=torch.float32, device=dev),
               torch.empty((B, F), dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.int64, device=dev))
    f0, unv, nf = out
    _dev(f0, unv, nf)
    if f0.dtype != torch.float32 or unv.dtype != torch.float32 or f0.numel() != B * F or \
            unv.numel() != B * F or nf.dtype != torch.int64 or nf.numel() != B:
        raise RuntimeError("f0_pyin: out is (f0 (B, F), unvoiced (B, F)) f32 and n_frames (B) int64")
    st = torch.empty((B, F), dtype=torch.int32, device=dev) if states else None
    nbytes = lib.fs2_f0_pyin_ws_bytes(B, S, hop, nb)
    wk = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    lib.fs2_f0_pyin(ptr(wav), ptr(lens), B, S, hop, float(sr), float(f0_floor), float(f0_ceil),
                    ptr(prior), ptr(tri), tri.numel() - 1, ptr(centres), nb, ptr(f0), ptr(unv),
                    ptr(nf), ptr(st), ptr(wk), nbytes, stream())
    return (f0, unv, nf, st) if states else (f0, unv, nf)


def resample(wav, lens, table, up, down, half, first=None, count=None, out_samples=None, out=None):
    """Rational polyphase resampling of a ragged batch (fs2_resample): wav (B, S) f32, lens
    device int64 (B) or None, table device f32 (2 half + 1) = L h (audio.resample_filter),
    up = L, down = M -> ``(out (B, out_samples), out_lens (B) int64)``, zeros past ``out_lens``.
    ``first`` / ``count`` (device int64 (B) or None) select the window ``y[first:first + count]``
    of each row; ``out_samples`` defaults to ``ceil(S L / M)``.  ``out`` = preallocated
    ``(out, out_lens)``."""
    _rows_f32("resample", wav, lens)
    _dev(table, first, count)
    if table.dtype != torch.float32 or table.dim() != 1:
        raise RuntimeError("resample: table is f32 (2 half + 1)")
    B, S = wav.shape
    for name, v in (("first", first), ("count", count)):
        if v is not None and (v.dtype != torch.int64 or v.numel() != B):
            raise RuntimeError(f"resample: {name} is int64 (B)")
    up, down, half = int(up), int(down), int(half)
    if up < 1 or down < 1:
        raise RuntimeError(f"resample: L {up}, M {down}")
    if out is None:
        cols = -(-S * up // down) if out_samples is None else int(out_samples)
        out = (torch.empty((B, max(cols, 1)), dtype=torch.float32, device=wav.device),
               torch.empty(B, dtype=torch.int64, device=wav.device))
    y, n = out
    _dev(y, n)
    if y.dtype != torch.float32 or y.dim() != 2 or y.shape[0] != B or not y.is_contiguous() or \
            n.dtype != torch.int64 or n.numel() != B:
        raise RuntimeError("resample: out is (out (B, out_samples) f32, out_lens (B) int64)")
    lib.fs2_resample(ptr(wav), ptr(lens), B, S, ptr(table), table.numel(), up, down, half,
                     ptr(first), ptr(count), ptr(y), y.shape[1], ptr(n), stream())
    return y, n


def nonsilent_split(wav, lens, top_db, frame_length=2048, hop=512, pad_mode=0, max_intervals=None,
                    power=False, out=None):
    """``librosa.effects.split`` of a ragged batch (fs2_nonsilent_split): wav (B, S) f32, lens
    device int64 (B) or None -> ``(intervals (B, max_intervals, 2) int64, n_intervals (B) int32,
    power (B, F) f32 or None)``, F = 1 + S // hop.  ``n_intervals`` is the true count, entries
    of ``intervals`` past it are zero; ``max_intervals`` defaults to the bound ``F // 2 + 1``.
    ``pad_mode`` 0 reflects, 1 pads zeros.  ``out`` = preallocated
    ``(intervals, n_intervals, power or None)``."""
    _rows_f32("nonsilent_split", wav, lens)
    B, S = wav.shape
    frame_length, hop = int(frame_length), int(hop)
    if frame_length < 2 or frame_length > 4096 or frame_length % 2 or not 1 <= hop <= frame_length:
        raise RuntimeError(f"nonsilent_split: frame_length {frame_length} (even, 2..4096), "
                           f"hop {hop} (1..frame_length)")
    if S < 1:
        raise RuntimeError("nonsilent_split: wav has no samples")
    F, dev = 1 + S // hop, wav.device
    if out is None:
        cap = F // 2 + 1 if max_intervals is None else int(max_intervals)
        out = (torch.empty((B, cap, 2), dtype=torch.int64, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty((B, F), dtype=torch.float32, device=dev) if power else None)
    iv, n_iv, pw = out
    _dev(iv, n_iv, pw)
    if iv.dtype != torch.int64 or iv.dim() != 3 or iv.shape[0] != B or iv.shape[2] != 2 or \
            n_iv.dtype != torch.int32 or n_iv.numel() != B or \
            (pw is not None and (pw.dtype != torch.float32 or pw.numel() != B * F)):
        raise RuntimeError("nonsilent_split: out is (intervals (B, max_intervals, 2) int64, "
                           "n_intervals (B) int32, power (B, F) f32 or None)")
    nbytes = 0 if pw is not None else lib.fs2_nonsilent_split_ws_bytes(B, S, hop)
    scratch = ws(nbytes, dev) if pw is None else None
    lib.fs2_nonsilent_split(ptr(wav), ptr(lens), B, S, frame_length, hop, float(top_db),
                            int(pad_mode), ptr(iv), iv.shape[1], ptr(n_iv), ptr(pw), ptr(scratch),
                            nbytes, stream())
    return iv, n_iv, pw


def wave_segments(wav, seg_row, seg_first, seg_len, out_samples, out=None):
    """out[s, i] = wav[seg_row[s], seg_first[s] + i] for i < seg_len[s], zeros up to
    ``out_samples`` (fs2_wave_segments): wav (B, S) f32; descriptors device int32 / int64 /
    int64, one per segment; the caller guarantees ``seg_first + seg_len <= S`` and
    ``seg_len <= out_samples``."""
    _dev(wav, seg_row, seg_first, seg_len, out)
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise RuntimeError("wave_segments: wav is f32 (B, S)")
    if (seg_row.dtype, seg_first.dtype, seg_len.dtype) != (torch.int32, torch.int64, torch.int64):
        raise RuntimeError("wave_segments: seg_row i32, seg_first / seg_len i64")
    n = seg_row.numel()
    if seg_first.numel() != n or seg_len.numel() != n:
        raise RuntimeError("wave_segments: one descriptor of each kind per segment")
    out_samples = int(out_samples)
    if out_samples < 1 or wav.numel() == 0:
        raise RuntimeError(f"wave_segments: out_samples {out_samples}, wav {tuple(wav.shape)}")
    if out is None:
        out = torch.empty((n, out_samples), dtype=torch.float32, device=wav.device)
    elif out.dtype != torch.float32 or out.numel() != n * out_samples:
        raise RuntimeError("wave_segments: out is f32 (n_seg, out_samples)")
    lib.fs2_wave_segments(ptr(wav), wav.shape[0], wav.shape[1], ptr(seg_row), ptr(seg_first),
                          ptr(seg_len), n, ptr(out), out_samples, stream())
    return out


def tisv_window_count(frames, tisv):
    """Windows of ``tisv`` frames at half-window steps in ``frames`` frames
    (data_preprocess.py:63-66): ``2 frames // tisv - 1``, 0 below ``tisv``."""
    frames, tisv = int(frames), int(tisv)
    return 2 * frames // tisv - 1 if frames >= tisv else 0


def tisv_windows(mel, n_frames, win_off, n_windows, tisv, out=None):
    """The half-overlapping ``tisv``-frame windows of each row of mel (rows, n_mels, F) f32
    (fs2_tisv_windows): window j of row r is ``mel[r, :, tisv j // 2 : tisv j // 2 + tisv]``.
    n_frames device int64 (rows); win_off device int64 (rows + 1), the exclusive prefix of
    ``tisv_window_count`` per row, and ``n_windows`` its last entry (both from the host) ->
    (n_windows, n_mels, tisv)."""
    _dev(mel, n_frames, win_off, out)
    if mel.dim() != 3 or mel.dtype != torch.float32:
        raise RuntimeError("tisv_windows: mel is f32 (rows, n_mels, F)")
    rows, n_mels, F = mel.shape
    if n_frames.dtype != torch.int64 or n_frames.numel() != rows or \
            win_off.dtype != torch.int64 or win_off.numel() != rows + 1:
        raise RuntimeError("tisv_windows: n_frames int64 (rows), win_off int64 (rows + 1)")
    n_windows, tisv = int(n_windows), int(tisv)
    if out is None:
        out = torch.empty((n_windows, n_mels, tisv), dtype=torch.float32, device=mel.device)
    elif out.dtype != torch.float32 or out.numel() != n_windows * n_mels * tisv:
        raise RuntimeError("tisv_windows: out is f32 (n_windows, n_mels, tisv)")
    if n_windows:
        lib.fs2_tisv_windows(ptr(mel), ptr(n_frames), rows, n_mels, F, tisv, ptr(win_off),
                             n_windows, ptr(out), stream())
    return out


def pitch_fill_(x, n=None):
    """Interpolate over the zero frames of each row in place (fs2_pitch_fill,
    preprocessor.py:213-221): x (B, F) f32, n device int64 (B) live frames or None ->
    ``ok (B) int32``, 1 where the row has more than one non-zero frame (others are untouched)."""
    _rows_f32("pitch_fill", x, n)
    ok = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    lib.fs2_pitch_fill(ptr(x), ptr(n), x.shape[0], x.shape[1], ptr(ok), stream())
    return ok


def segment_mean_(x, durations, n=None):
    """Phoneme-level means (fs2_segment_mean, preprocessor.py:223-242): x (B, F) f32, durations
    (B, P) int64, n device int64 (B) live frames or None -> (B, P) f32.  As in the reference the
    means are also written over ``x[:, :P]`` while later phonemes still read it."""
    _rows_f32("segment_mean", x, n)
    _dev(durations)
    if durations.dim() != 2 or durations.dtype != torch.int64 or durations.shape[0] != x.shape[0]:
        raise RuntimeError("segment_mean: durations are int64 (B, P)")
    out = torch.empty(durations.shape, dtype=torch.float32, device=x.device)
    lib.fs2_segment_mean(ptr(x), ptr(n), ptr(durations), x.shape[0], x.shape[1],
                         durations.shape[1], ptr(out), stream())
    return out


def outlier_moments_(state, sorted_values, n=None):
    """state (device f64[3] = count, mean, M2) takes in, row by row, the values of
    ``sorted_values`` (B, cols) f32 (ascending, the ``n[b]`` live ones first) that survive
    ``remove_outlier`` (fs2_outlier_moments, preprocessor.py:307-315 and 94-97)."""
    _rows_f32("outlier_moments", sorted_values, n)
    _dev(state)
    if state.dtype != torch.float64 or state.numel() != 3:
        raise RuntimeError("outlier_moments: state is f64[3]")
    lib.fs2_outlier_moments(ptr(sorted_values), ptr(n), sorted_values.shape[0],
                            sorted_values.shape[1], ptr(state), stream())
    return state


def normalize_minmax_(x, mean, std, minmax, n=None):
    """x[b, :n[b]] = (x - mean) / std in place; minmax (device f64[2]) keeps the running
    extrema of the stored values (fs2_normalize_minmax, preprocessor.py:317-328)."""
    _rows_f32("normalize_minmax", x, n)
    _dev(minmax)
    if minmax.dtype != torch.float64 or minmax.numel() != 2:
        raise RuntimeError("normalize_minmax: minmax is f64[2]")
    lib.fs2_normalize_minmax(ptr(x), ptr(n), x.shape[0], x.shape[1], float(mean), float(std),
                             ptr(minmax), stream())
    return x


def ge2e_eer(enroll, verify):
    """test()'s scoring of one batch: enroll (N, M_e, D), verify (N, M_v, D) ->
    sim (N, M_v, N), table (50, 2) = FAR, FRR per threshold, result (4) = EER, threshold, FAR,
    FRR, all on the device (fs2_ge2e_eer)."""
    _dev(enroll, verify)
    N, Me, D = enroll.shape
    Nv, Mv, Dv = verify.shape
    if (Nv, Dv) != (N, D) or enroll.dtype != torch.float32 or verify.dtype != torch.float32:
        raise RuntimeError("ge2e_eer: enroll (N, M_e, D) and verify (N, M_v, D), f32")
    dev = enroll.device
    sim = torch.empty((N, Mv, N), dtype=torch.float32, device=dev)
    table = torch.empty((50, 2), dtype=torch.float32, device=dev)
    result = torch.empty(4, dtype=torch.float32, device=dev)
    n = lib.fs2_ge2e_eer_ws_bytes(N, D)
    wk = ws(n, dev)
    lib.fs2_ge2e_eer(ptr(enroll), ptr(verify), N, Me, Mv, D, ptr(sim), ptr(table), ptr(result),
                     ptr(wk), n, stream())
    return sim, table, result


def epoch_stats_add(totals, loss=None, da_loss=None, logit=None, y=None, correct=None):
    """totals (device float[4]) += [loss, da_loss, 100 * accuracy(logit, y), 1] without a host
    read; ``correct`` (device float) receives the count of right labels (fs2_epoch_stats_add)."""
    _dev(totals, loss, da_loss, logit, y, correct)
    n = logit.numel() if logit is not None else 0
    lib.fs2_epoch_stats_add(ptr(totals), ptr(loss), ptr(da_loss), ptr(logit), ptr(y), n,
                            ptr(correct), stream())


def _host_i32(a, n, what):
    import numpy as np
    if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous and
            a.size == n):
        raise RuntimeError(f"batch_gather: {what} must be a contiguous host int32[{n}] array")
    return a.ctypes.data


def batch_gather(st, idx, idx_host, max_src_len, max_mel_len, accents=True, out=None):
    """The padded training batch of the utterances ``idx`` (device int32[B]; ``idx_host`` its host
    copy, which the entry point validates against the store's host tables before it launches) of
    a device-resident corpus ``st`` (``corpus_store.CorpusStore``: flat ``text``, ``dur``,
    ``accent``, ``mel``, ``pitch``, ``energy``, ``meta`` stores, the device tables
    ``d_src_len``, ``d_mel_len``, ``d_src_off``, ``d_mel_off``, ``d_speaker`` and the host tables
    ``src_len``, ``mel_len``) in one launch (fs2_batch_gather).  Returns ``(speakers, texts,
    src_lens, mels, mel_lens, pitches, energies, durations, speaker_meta, accents or None)`` with
    ``to_device``'s dtypes; ``out``: such a tuple of the same shapes to write into."""
    B, n = idx.numel(), len(st)
    Ts, Tm, C, Md = int(max_src_len), int(max_mel_len), st.n_mels, st.meta_dim
    pf, ef = st.levels
    dev = st.mel.device
    _dev(idx, st.text, st.dur, st.accent, st.mel, st.pitch, st.energy, st.meta, st.d_src_len,
         st.d_mel_len, st.d_src_off, st.d_mel_off, st.d_speaker)
    if idx.dtype != torch.int32:
        raise RuntimeError("batch_gather: idx must be device int32")
    i64, f32 = torch.int64, torch.float32
    spec = (((B,), i64), ((B, Ts), i64), ((B,), i64), ((B, Tm, C), f32), ((B,), i64),
            ((B, Tm if pf else Ts), f32), ((B, Tm if ef else Ts), st.energy.dtype),
            ((B, Ts), i64), ((B, Md), f32), ((B, Ts), i64))
    if out is None:
        out = [torch.empty(s, dtype=d, device=dev) for s, d in spec]
        if not accents:
            out[9] = None
    else:
        out = list(out)
        if len(out) != 10 or (out[9] is None) == bool(accents):
            raise RuntimeError("batch_gather: out must be a tuple this function returned")
        for t, (s, d) in zip(out, spec):
            if t is not None and (tuple(t.shape) != s or t.dtype != d):
                raise RuntimeError(f"batch_gather: out tensor {tuple(t.shape)} {t.dtype}, "
                                   f"expected {s} {d}")
        _dev(*out)
    spk, texts, sl, mels, ml, pit, ene, dur, meta, acc = out
    lib.fs2_batch_gather(
        ptr(idx), _host_i32(idx_host, B, "idx_host"), B, n,
        _host_i32(st.src_len, n, "src_len"), _host_i32(st.mel_len, n, "mel_len"),
        ptr(st.d_src_len), ptr(st.d_mel_len), ptr(st.d_src_off), ptr(st.d_mel_off),
        ptr(st.d_speaker), ptr(st.text), ptr(st.dur), ptr(st.accent), ptr(st.mel), ptr(st.pitch),
        ptr(st.energy), ptr(st.meta), C, Md, st.energy.element_size(), int(pf), int(ef), Ts, Tm,
        ptr(texts), ptr(dur), ptr(acc), ptr(mels), ptr(pit), ptr(ene), ptr(sl), ptr(ml), ptr(spk),
        ptr(meta), stream())
    return tuple(out)


def eval_accum(sums, esum, losses, eloss, batch):
    """sums (device double[6]) += losses (device float[6]) * batch; esum (device float[1]) +=
    eloss * batch: the validation sums of evaluate.py:68-72 without a host read
    (fs2_eval_accum)."""
    _dev(sums, esum, losses, eloss)
    if (sums.dtype, esum.dtype, losses.dtype) != (torch.float64, torch.float32, torch.float32) \
            or sums.numel() != 6 or losses.numel() != 6:
        raise RuntimeError("eval_accum: sums f64[6], esum f32[1], losses f32[6]")
    lib.fs2_eval_accum(ptr(sums), ptr(esum), ptr(losses), ptr(eloss), int(batch), stream())


def sched_step(steps, hyper, init_lr, n_warmup, anneal_steps, anneal_rate, beta1, beta2,
               advance_lr=True):
    """Device-side LR schedule + Adam bias corrections for one step (fs2_sched_step)."""
    an = (ctypes.c_int64 * 3)(*[int(a) for a in anneal_steps][:3])
    lib.fs2_sched_step(ptr(steps), ptr(hyper), float(init_lr), int(n_warmup), ctypes.addressof(an),
                       len(anneal_steps), float(anneal_rate), float(beta1), float(beta2),
                       int(advance_lr), stream())


def seed_next(state):
    """state: device int64[3] {base, counter, current}; advances the per-step dropout seed."""
    lib.fs2_seed_next(ptr(state), stream())


def fill_(t, value):
    _dev(t)
    lib.fs2_fill(ptr(t), t.numel(), float(value), stream())
    return t


def zeros(shape, device):
    return fill_(torch.empty(shape, dtype=torch.float32, device=device), 0.0)


def add(a, b, out=None):
    _dev(a, b)
    out = torch.empty_like(a) if out is None else out
    lib.fs2_add(ptr(out), ptr(a), ptr(b), a.numel(), stream())
    return out


def scale_(t, value):
    """t *= value in place (f32)."""
    _dev(t)
    lib.fs2_scale(ptr(t), t.numel(), float(value), stream())
    return t


def add_i64_(t, value):
    _dev(t)
    lib.fs2_add_i64(ptr(t), t.numel(), int(value), stream())
    return t


# ------------------------------------------------------------------ mid-attribute GMMs
def gmm_w2_cost(mu_a, sd_a, mu_b, sd_b):
    """(ka, kb) float64 cost of InterpolateGMM._w2sq (distributions.py:64-77)."""
    _dev(mu_a, sd_a, mu_b, sd_b)
    ka, d = mu_a.shape
    kb = mu_b.shape[0]
    cost = torch.empty(ka, kb, dtype=torch.float64, device=mu_a.device)
    lib.fs2_gmm_w2_cost(ptr(mu_a), ptr(sd_a), ka, ptr(mu_b), ptr(sd_b), kb, d, ptr(cost), stream())
    return cost


def ot_emd(a, b, cost, max_iter=10000):
    """Exact OT plan (ot.emd): (plan float64 (ka, kb), status int32[1] = iterations or -1)."""
    _dev(a, b, cost)
    ka, kb = cost.shape
    plan = torch.empty(ka, kb, dtype=torch.float64, device=cost.device)
    status = torch.empty(1, dtype=torch.int32, device=cost.device)
    lib.fs2_ot_emd(ptr(a), ptr(b), ptr(cost), ka, kb, int(max_iter), ptr(plan), ptr(status),
                   stream())
    return plan, status


def gmm_interpolate(plan, mu_a, sd_a, mu_b, sd_b, t):
    _dev(plan, mu_a, sd_a, mu_b, sd_b)
    ka, d = mu_a.shape
    kb = mu_b.shape[0]
    n = ka * kb
    pi = torch.empty(n, dtype=torch.float32, device=mu_a.device)
    mu = torch.empty(n, d, dtype=torch.float32, device=mu_a.device)
    sd = torch.empty(n, d, dtype=torch.float32, device=mu_a.device)
    lib.fs2_gmm_interpolate(ptr(plan), ptr(mu_a), ptr(sd_a), ka, ptr(mu_b), ptr(sd_b), kb, d,
                            float(t), ptr(pi), ptr(mu), ptr(sd), stream())
    return pi, mu, sd


def gmm_barycenter(mu, sd, rate32, iters=60):
    """Barycenter mean/std of every position of product(range(k), repeat=m)."""
    _dev(mu, sd, rate32)
    m, k, d = mu.shape
    n_pos = lib.fs2_gmm_barycenter_positions(m, k)
    if n_pos <= 0:
        raise RuntimeError(f"{k}^{m} barycenter positions exceed the kernel's limit")
    bm = torch.empty(n_pos, d, dtype=torch.float32, device=mu.device)
    bs = torch.empty(n_pos, d, dtype=torch.float32, device=mu.device)
    lib.fs2_gmm_barycenter(ptr(mu), ptr(sd), m, k, d, ptr(rate32), int(iters), ptr(bm), ptr(bs),
                           stream())
    return bm, bs


def gmm_bary_mix(pi, mu, sd, rate64, bm, bs):
    """Nearest-barycenter mixture: (n_used int32[1], used, pi, mu, sd) with capacity m*k
    (rows past n_used are unwritten)."""
    _dev(pi, mu, sd, rate64, bm, bs)
    m, k, d = mu.shape
    dev = mu.device
    n_used = torch.empty(1, dtype=torch.int32, device=dev)
    used = torch.empty(m * k, dtype=torch.int32, device=dev)
    pi_o = torch.empty(m * k, dtype=torch.float32, device=dev)
    mu_o = torch.empty(m * k, d, dtype=torch.float32, device=dev)
    sd_o = torch.empty(m * k, d, dtype=torch.float32, device=dev)
    n = lib.fs2_gmm_bary_mix_ws_bytes(m, k)
    w = torch.empty(max(n // 8, 1), dtype=torch.float64, device=dev)
    lib.fs2_gmm_bary_mix(ptr(pi), ptr(mu), ptr(sd), m, k, d, ptr(rate64), ptr(bm), ptr(bs),
                         ptr(n_used), ptr(used), ptr(pi_o), ptr(mu_o), ptr(sd_o), ptr(w), n,
                         stream())
    return n_used, used, pi_o, mu_o, sd_o


# ------------------------------------------------------------------ objective synthesis metrics
METRIC_FIELDS = 8    # FS2_METRIC_FIELDS
DTW_MAX_LEN = 2048   # FS2_DTW_MAX_LEN


def _lens_i64(name, lens, batch):
    _dev(lens)
    if lens.dtype != torch.int64 or lens.numel() != batch:
        raise RuntimeError(f"{name}: lengths are device int64 ({batch})")


def mfcc(logmel, n_frames, dct, rows=False):
    """Coefficients 1..K of the orthonormal DCT-II over the mel axis (fs2_mfcc): logmel
    (B, n_mels, F) f32, or with ``rows`` the model's row layout (B, F, n_mels) / (B * F, n_mels);
    n_frames device int64 (B) (None: every frame; needed for the 2-D row layout, whose batch
    it gives); dct (n_mels, K) f32, ``metrics.dct_table`` -> (B, F, K), zeros past n_frames."""
    _dev(logmel, n_frames, dct)
    if logmel.dtype != torch.float32 or dct.dtype != torch.float32 or dct.dim() != 2:
        raise RuntimeError("mfcc: logmel and the DCT table are f32")
    n_mels, n_coef = dct.shape
    if rows:
        if logmel.dim() == 3:
            B, F = logmel.shape[:2]
        elif logmel.dim() == 2 and n_frames is not None and logmel.shape[0] % n_frames.numel() == 0:
            B = n_frames.numel()
            F = logmel.shape[0] // B
        else:
            raise RuntimeError("mfcc: the row layout is (B, F, n_mels), or (B * F, n_mels) with "
                               "n_frames (B)")
        ok = logmel.shape[-1] == n_mels
    else:
        ok = logmel.dim() == 3 and logmel.shape[1] == n_mels
        B, F = (logmel.shape[0], logmel.shape[2]) if ok else (0, 0)
    if not ok:
        raise RuntimeError(f"mfcc: logmel {tuple(logmel.shape)} does not have the table's "
                           f"{n_mels} mel channels")
    if n_frames is not None:
        _lens_i64("mfcc", n_frames, B)
    out = torch.empty((B, F, n_coef), dtype=torch.float32, device=logmel.device)
    lib.fs2_mfcc(ptr(logmel), ptr(n_frames), B, n_mels, F, int(bool(rows)), ptr(dct), n_coef,
                 ptr(out), stream())
    return out


def dtw(a, b, la, lb):
    """Batched dynamic time warping with its path (fs2_dtw): a (B, T1max, K), b (B, T2max, K) f32,
    la / lb device int64 (B) -> ``(cost (B) f64, path (B, T1max + T2max - 1, 2) int32,
    path_len (B) int32)``; entries of ``path`` past ``path_len`` are unwritten."""
    _dev(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 3 or b.dim() != 3 or \
            a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise RuntimeError("dtw: a (B, T1max, K) and b (B, T2max, K) are f32")
    B, T1, Kf = a.shape
    T2, dev = b.shape[1], a.device
    _lens_i64("dtw", la, B)
    _lens_i64("dtw", lb, B)
    cost = torch.empty(B, dtype=torch.float64, device=dev)
    path = torch.empty((B, max(T1 + T2 - 1, 0), 2), dtype=torch.int32, device=dev)
    path_len = torch.empty(B, dtype=torch.int32, device=dev)
    nb = lib.fs2_dtw_ws_bytes(B, T1, T2, Kf)
    wk = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    lib.fs2_dtw(ptr(a), ptr(b), ptr(la), ptr(lb), B, T1, T2, Kf, ptr(cost), ptr(path),
                ptr(path_len), ptr(wk), nb, stream())
    return cost, path, path_len


def path_metrics(cost, path, path_len, la, lb, t1_max, t2_max, fa=None, fb=None):
    """The per-pair records along DTW paths (fs2_path_metrics) -> (B, METRIC_FIELDS) f64:
    path_len, mcd_db, frames_a, frames_b, n_vv, f0_sq_cents, n_vuv, len_err; fa (B, T1max) and
    fb (B, T2max) f32 F0 contours (0 = unvoiced), both or neither."""
    _dev(cost, path, path_len, fa, fb)
    B, T1, T2 = cost.numel(), int(t1_max), int(t2_max)
    if cost.dtype != torch.float64 or path.dtype != torch.int32 or path_len.dtype != torch.int32 \
            or tuple(path.shape) != (B, T1 + T2 - 1, 2) or path_len.numel() != B:
        raise RuntimeError("path_metrics: cost f64 (B), path int32 (B, T1max + T2max - 1, 2), "
                           "path_len int32 (B)")
    _lens_i64("path_metrics", la, B)
    _lens_i64("path_metrics", lb, B)
    if (fa is None) != (fb is None):
        raise RuntimeError("path_metrics: the F0 contours come as a pair or not at all")
    if fa is not None and (fa.dtype != torch.float32 or fb.dtype != torch.float32 or
                           tuple(fa.shape) != (B, T1) or tuple(fb.shape) != (B, T2)):
        raise RuntimeError(f"path_metrics: F0 contours are f32 ({B}, {T1}) and ({B}, {T2})")
    rec = torch.empty((B, METRIC_FIELDS), dtype=torch.float64, device=cost.device)
    lib.fs2_path_metrics(ptr(cost), ptr(path), ptr(path_len), ptr(la), ptr(lb), B, T1, T2, ptr(fa),
                         ptr(fb), ptr(rec), stream())
    return rec


# ------------------------------------------------------------------ alignment without TextGrids
ALIGN_MAX_SRC = 1024   # FS2_ALIGN_MAX_SRC
ALIGN_MAX_MEL = 2048   # FS2_ALIGN_MAX_MEL
ALIGN_MAX_WIDTH = 128  # FS2_ALIGN_MAX_WIDTH


def _align_qk(name, q, k, src_lens, mel_lens):
    _dev(q, k)
    if q.dtype != torch.float32 or k.dtype != torch.float32 or q.dim() != 3 or k.dim() != 3 or \
            q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise RuntimeError(f"{name}: q (B, T_m, A) and k (B, T_s, A) are f32")
    B, T_m, A = q.shape
    _lens_i64(name, src_lens, B)
    _lens_i64(name, mel_lens, B)
    return B, T_m, k.shape[1], A


def _align_logp(name, logp, src_lens, mel_lens):
    _dev(logp)
    if logp.dtype != torch.float32 or logp.dim() != 3:
        raise RuntimeError(f"{name}: logp (B, T_m, T_s) is f32")
    B, T_m, T_s = logp.shape
    _lens_i64(name, src_lens, B)
    _lens_i64(name, mel_lens, B)
    return B, T_m, T_s


def _align_path_exists(name, host_lens):
    """``host_lens``: (src, mel) length lists where the caller has them on the host."""
    if host_lens is not None:
        for b, (n, m) in enumerate(zip(*host_lens)):
            if int(m) < int(n):
                raise RuntimeError(f"{name}: row {b} has {int(m)} frames for {int(n)} phonemes "
                                   "(no monotonic path)")


def align_logprob(q, k, src_lens, mel_lens, temperature, omega=0.0):
    """fs2_align_logprob: q (B, T_m, A), k (B, T_s, A) f32, device int64 lengths -> logp
    (B, T_m, T_s) = log_softmax_s(-temperature |q_t - k_s|^2) + the log beta-binomial prior
    (``omega`` <= 0: none); cells past a row's lengths are 0."""
    B, T_m, T_s, A = _align_qk("align_logprob", q, k, src_lens, mel_lens)
    logp = torch.empty((B, T_m, T_s), dtype=torch.float32, device=q.device)
    lib.fs2_align_logprob(ptr(q), ptr(k), ptr(src_lens), ptr(mel_lens), B, T_m, T_s, A,
                          float(temperature), float(omega), ptr(logp), stream())
    return logp


def align_logprob_bwd(q, k, g, src_lens, mel_lens, temperature):
    """fs2_align_logprob_bwd: g = dL/dlogp (B, T_m, T_s) -> ``(dq, dk)``; the softmax is recomputed
    and the prior has no gradient."""
    B, T_m, T_s, A = _align_qk("align_logprob_bwd", q, k, src_lens, mel_lens)
    _dev(g)
    if g.dtype != torch.float32 or tuple(g.shape) != (B, T_m, T_s):
        raise RuntimeError(f"align_logprob_bwd: g is f32 ({B}, {T_m}, {T_s})")
    dq, dk = torch.empty_like(q), torch.empty_like(k)
    nb = lib.fs2_align_logprob_bwd_ws_bytes(B, T_m, T_s, A)
    wk = ws(nb, q.device)
    lib.fs2_align_logprob_bwd(ptr(q), ptr(k), ptr(g), ptr(src_lens), ptr(mel_lens), B, T_m, T_s, A,
                              float(temperature), ptr(dq), ptr(dk), ptr(wk), nb, stream())
    return dq, dk


def _align_optional(name, optional, B, T_s, host_lens):
    """The device mask of ``forward_sum`` / ``mas``; with ``host_lens`` = (src, mel, mask), the
    mask's host copy (B, >= N), the rows are checked before any launch: two adjacent marks or no
    unmarked position is a ``ValueError``, fewer frames than unmarked positions has no path."""
    _dev(optional)
    if optional.dtype != torch.uint8 or tuple(optional.shape) != (B, T_s) or \
            not optional.is_contiguous():
        raise RuntimeError(f"{name}: optional is uint8 ({B}, {T_s}), contiguous")
    if host_lens is None:
        return
    if len(host_lens) < 3:
        raise RuntimeError(f"{name}: with a mask host_lens is (src, mel, the mask's host copy)")
    for b, (n, m, row) in enumerate(zip(*host_lens)):
        n = int(n)
        marks = [bool(v) for v in list(row)[:n]]
        if len(marks) < n:
            raise RuntimeError(f"{name}: row {b}: a host mask of {len(marks)} for {n} positions")
        if any(x and y for x, y in zip(marks, marks[1:])):
            raise ValueError(f"{name}: row {b} has two adjacent optional positions")
        need = n - sum(marks)
        if n >= 1 and need == 0:
            raise ValueError(f"{name}: row {b} has no position that is not optional")
        if int(m) < need:
            raise RuntimeError(f"{name}: row {b} has {int(m)} frames for {need} phonemes "
                               "(no monotonic path)")


def forward_sum(logp, src_lens, mel_lens, w, host_lens=None, optional=None):
    """fs2_forward_sum: the CTC forward-sum loss of the target 1..N under logp (blank score -1)
    -> ``(nll (B) f32, grad (B, T_m, T_s) = d(nll[b] w[b]) / dlogp)``.  ``host_lens`` = (src, mel)
    host lists: a row with fewer frames than phonemes raises before the launch (on the device
    such a row gives nll = +inf and a zero gradient).  ``optional`` (B, T_s) uint8 on the device:
    fs2_forward_sum_opt, marked positions may take no frame; ``host_lens`` is then (src, mel,
    the mask's host copy), see ``_align_optional``."""
    B, T_m, T_s = _align_logp("forward_sum", logp, src_lens, mel_lens)
    _dev(w)
    if w.dtype != torch.float32 or w.numel() != B:
        raise RuntimeError(f"forward_sum: w is f32 ({B})")
    if optional is not None:
        _align_optional("forward_sum", optional, B, T_s, host_lens)
    else:
        _align_path_exists("forward_sum", host_lens)
    nll = torch.empty(B, dtype=torch.float32, device=logp.device)
    grad = torch.empty_like(logp)
    nb = lib.fs2_forward_sum_ws_bytes(B, T_m, T_s)
    wk = torch.empty(max(nb // 8, 1), dtype=torch.float64, device=logp.device)
    if optional is not None:
        lib.fs2_forward_sum_opt(ptr(logp), ptr(src_lens), ptr(mel_lens), ptr(optional), ptr(w), B,
                                T_m, T_s, ptr(nll), ptr(grad), ptr(wk), nb, stream())
        return nll, grad
    lib.fs2_forward_sum(ptr(logp), ptr(src_lens), ptr(mel_lens), ptr(w), B, T_m, T_s, ptr(nll),
                        ptr(grad), ptr(wk), nb, stream())
    return nll, grad


def mas(logp, src_lens, mel_lens, host_lens=None, optional=None):
    """fs2_mas: monotonic alignment search -> durations (B, T_s) int64, frames per phoneme (>= 1
    below a row's phoneme count, 0 past it).  ``host_lens`` as in ``forward_sum``.  ``optional``
    (B, T_s) uint8 on the device: fs2_mas_opt, a marked position the path omits has 0 frames."""
    B, T_m, T_s = _align_logp("mas", logp, src_lens, mel_lens)
    if optional is not None:
        _align_optional("mas", optional, B, T_s, host_lens)
    else:
        _align_path_exists("mas", host_lens)
    durations = torch.empty((B, T_s), dtype=torch.int64, device=logp.device)
    nb = lib.fs2_mas_ws_bytes(B, T_m, T_s)
    wk = torch.empty(max(nb, 1), dtype=torch.uint8, device=logp.device)
    if optional is not None:
        lib.fs2_mas_opt(ptr(logp), ptr(src_lens), ptr(mel_lens), ptr(optional), B, T_m, T_s,
                        ptr(durations), ptr(wk), nb, stream())
        return durations
    lib.fs2_mas(ptr(logp), ptr(src_lens), ptr(mel_lens), B, T_m, T_s, ptr(durations), ptr(wk), nb,
                stream())
    return durations


# ------------------------------------------------------------------ phoneme error rate
CTC_MAX_T = 2048         # FS2_CTC_MAX_T
CTC_MAX_TARGET = 1024    # FS2_CTC_MAX_TARGET
CTC_MAX_CLASSES = 1024   # FS2_CTC_MAX_CLASSES
EDIT_MAX_LEN = 2048      # FS2_EDIT_MAX_LEN


def _ctc_logits(name, logits, frame_lens, n_classes):
    _dev(logits)
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise RuntimeError(f"{name}: logits (B, T, ld) are f32")
    B, T, ld = logits.shape
    _lens_i64(name, frame_lens, B)
    return B, T, ld, ld if n_classes is None else int(n_classes)


def ctc_loss(logits, targets, frame_lens, target_lens, w, n_classes=None, blank=0, host_lens=None):
    """fs2_ctc_loss: logits (B, T, ld) f32 whose first ``n_classes`` columns are the classes
    (default all), targets (B, L_max) int64, device int64 lengths, w (B) f32 -> ``(nll (B) f32,
    grad (B, T, ld) = d(w[b] nll[b]) / dlogits)``, the gradient 0 past a row's frames and in the
    columns past the classes.  ``host_lens`` = (target, frame) host lists: a row with fewer frames
    than labels raises before the launch (on the device a row without a valid path gives nll =
    +inf and a zero gradient)."""
    B, T, ld, C = _ctc_logits("ctc_loss", logits, frame_lens, n_classes)
    _dev(targets, w)
    if targets.dtype != torch.int64 or targets.dim() != 2 or targets.shape[0] != B:
        raise RuntimeError(f"ctc_loss: targets are int64 ({B}, L_max)")
    L_max = targets.shape[1]
    _lens_i64("ctc_loss", target_lens, B)
    if w.dtype != torch.float32 or w.numel() != B:
        raise RuntimeError(f"ctc_loss: w is f32 ({B})")
    if host_lens is not None:
        for b, (n, m) in enumerate(zip(*host_lens)):
            if int(m) < int(n):
                raise RuntimeError(f"ctc_loss: row {b} has {int(m)} frames for {int(n)} labels "
                                   "(no valid path)")
    nll = torch.empty(B, dtype=torch.float32, device=logits.device)
    grad = torch.empty_like(logits)
    nb = lib.fs2_ctc_loss_ws_bytes(B, T, L_max)
    wk = torch.empty(max(nb // 8, 1), dtype=torch.float64, device=logits.device)
    lib.fs2_ctc_loss(ptr(logits), ptr(targets), ptr(frame_lens), ptr(target_lens), ptr(w), B, T, C,
                     ld, int(blank), L_max, ptr(nll), ptr(grad), ptr(wk), nb, stream())
    return nll, grad


def ctc_greedy(logits, frame_lens, n_classes=None, blank=0, argmax=False):
    """fs2_ctc_greedy: per-frame arg-max of the raw logits (ties to the lowest class, a NaN never
    wins, an all-NaN frame is blank), repeats collapsed, blanks dropped -> ``(ids (B, T) int64, 0
    past the length, lens (B) int64)``; with ``argmax`` also the per-frame arg-max (B, T)
    int32."""
    B, T, ld, C = _ctc_logits("ctc_greedy", logits, frame_lens, n_classes)
    ids = torch.empty((B, T), dtype=torch.int64, device=logits.device)
    lens = torch.empty(B, dtype=torch.int64, device=logits.device)
    am = torch.empty((B, T), dtype=torch.int32, device=logits.device) if argmax else None
    lib.fs2_ctc_greedy(ptr(logits), ptr(frame_lens), B, T, C, ld, int(blank), ptr(ids), ptr(lens),
                       ptr(am), stream())
    return (ids, lens, am) if argmax else (ids, lens)


def edit_distance(ref, ref_lens, hyp, hyp_lens):
    """fs2_edit_distance: ref (B, R_max), hyp (B, H_max) int64 with device int64 lengths ->
    (B, 4) int64 = [distance, substitutions, deletions, insertions] of the unit-cost Levenshtein
    alignment, the diagonal preferred to a deletion to an insertion at a tie."""
    _dev(ref, hyp)
    if ref.dtype != torch.int64 or hyp.dtype != torch.int64 or ref.dim() != 2 or hyp.dim() != 2 \
            or ref.shape[0] != hyp.shape[0]:
        raise RuntimeError("edit_distance: ref (B, R_max) and hyp (B, H_max) are int64")
    (B, R), H = ref.shape, hyp.shape[1]
    _lens_i64("edit_distance", ref_lens, B)
    _lens_i64("edit_distance", hyp_lens, B)
    out = torch.empty((B, 4), dtype=torch.int64, device=ref.device)
    nb = lib.fs2_edit_distance_ws_bytes(B, R, H)
    wk = torch.empty(max(nb, 1), dtype=torch.uint8, device=ref.device)
    lib.fs2_edit_distance(ptr(ref), ptr(ref_lens), ptr(hyp), ptr(hyp_lens), B, R, H, ptr(out),
                          ptr(wk), nb, stream())
    return out


# ------------------------------------------------------------------ generated-speaker metrics
NN_MAX_DIM = 256           # FS2_NN_MAX_DIM
NN_MAX_K = 16              # FS2_NN_MAX_K
SUMMARY_MAX_N = 1 << 20    # FS2_SUMMARY_MAX_N
FRECHET_MAX_DIM = 64       # FS2_FRECHET_MAX_DIM


def cosine_nn(a, b, k=1, group_a=None, group_b=None, same=False):
    """fs2_cosine_nn: a (Na, D), b (Nb, D) f32 -> ``(dist (Na, k) f32 ascending, index (Na, k)
    int64)``, the k rows of b nearest to each row of a by cosine distance, ties to the lower
    index, slots without a candidate +inf / -1.  ``group_a`` (Na) / ``group_b`` (Nb) device
    int64, both or neither: candidates of the row's own group are skipped, or with ``same`` the
    only ones kept."""
    _dev(a, b, group_a, group_b)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or b.dim() != 2 or \
            a.shape[1] != b.shape[1]:
        raise RuntimeError("cosine_nn: a (Na, D) and b (Nb, D) are f32")
    (Na, D), Nb, k = a.shape, b.shape[0], int(k)
    if (group_a is None) != (group_b is None):
        raise RuntimeError("cosine_nn: the groups come as a pair or not at all")
    if group_a is not None and (group_a.dtype != torch.int64 or group_b.dtype != torch.int64 or
                                group_a.numel() != Na or group_b.numel() != Nb):
        raise RuntimeError(f"cosine_nn: groups are device int64 ({Na}) and ({Nb})")
    dist = torch.empty((Na, max(k, 0)), dtype=torch.float32, device=a.device)
    index = torch.empty((Na, max(k, 0)), dtype=torch.int64, device=a.device)
    nb = lib.fs2_cosine_nn_ws_bytes(Na, Nb, k)
    wk = torch.empty(max(nb, 1), dtype=torch.uint8, device=a.device)
    lib.fs2_cosine_nn(ptr(a), ptr(b), Na, Nb, D, k, ptr(group_a), ptr(group_b), int(bool(same)),
                      ptr(dist), ptr(index), ptr(wk), nb, stream())
    return dist, index


def finite_summary(x):
    """fs2_finite_summary: x f32 (any shape, at most 2^20 entries) -> f64[5] on the device =
    [count, median, mean, min, max] of the finite entries (NaN but for the count when none)."""
    _dev(x)
    if x.dtype != torch.float32:
        raise RuntimeError("finite_summary: x is f32")
    n = x.numel()
    out = torch.empty(5, dtype=torch.float64, device=x.device)
    nb = lib.fs2_finite_summary_ws_bytes(n)
    wk = torch.empty(max(nb, 1), dtype=torch.uint8, device=x.device)
    lib.fs2_finite_summary(ptr(x), n, ptr(out), ptr(wk), nb, stream())
    return out


def gauss_moments(x):
    """fs2_gauss_moments: x (n, D) f32, n >= 2 -> ``(mean (D), cov (D, D))`` f64, the unbiased
    covariance, two-pass with the rows in order."""
    _dev(x)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise RuntimeError("gauss_moments: x is f32 (n, D)")
    n, D = x.shape
    mean = torch.empty(D, dtype=torch.float64, device=x.device)
    cov = torch.empty((D, D), dtype=torch.float64, device=x.device)
    lib.fs2_gauss_moments(ptr(x), n, D, ptr(mean), ptr(cov), stream())
    return mean, cov


def frechet(mean_a, cov_a, mean_b, cov_b):
    """fs2_frechet: f64 moments (D) / (D, D), or batched (P, D) / (P, D, D) -> (P, 4) f64 =
    [distance, |dmu|^2, tr cov_a + tr cov_b, sum sqrt(eig(S cov_b S))]."""
    _dev(mean_a, cov_a, mean_b, cov_b)
    D = mean_a.shape[-1]
    P = mean_a.numel() // max(D, 1)
    for m, c in ((mean_a, cov_a), (mean_b, cov_b)):
        if m.dtype != torch.float64 or c.dtype != torch.float64 or m.numel() != P * D or \
                c.numel() != P * D * D or c.shape[-2:] != (D, D):
            raise RuntimeError(f"frechet: moments are f64 ({P}, {D}) and ({P}, {D}, {D})")
    out = torch.empty((P, 4), dtype=torch.float64, device=mean_a.device)
    lib.fs2_frechet(ptr(mean_a), ptr(cov_a), ptr(mean_b), ptr(cov_b), P, D, ptr(out), stream())
    return out
