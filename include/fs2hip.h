/* fs2hip.h — C-ABI of libfs2hip.so, the gfx950 (MI355X) kernels of the FastSpeech2 +
 * TacoSpawn-GMM training step.
 *
 * The reference (sarulab-speech/Mid-Attribute-Speaker-Generation) is pure PyTorch: it has no
 * FFI.  Each entry point below replaces a *sequence of ATen ops* of the reference's
 * `nn.Module`s; the citation on each names the reference lines it replaces
 * (paths relative to the reference root).  The Python host in
 * mid-attribute-speaker-generation_amd/ mirrors the reference module API on top of these.
 *
 * Conventions (all entry points):
 *   - plain device pointers, int64 sizes, a dtype enum where storage type varies,
 *     `stream` = hipStream_t (as void*), return 0 on success, <0 on error;
 *     `fs2_last_error()` describes the last failure of the calling thread.
 *   - no allocation, no host synchronisation: callers pass workspaces (size queries are
 *     provided), so every call can be captured into a hipGraph.
 *   - activations are (rows, channels) row-major = the reference's (B, T, C) layout;
 *     row r of a batch of sequences of length seq_len is frame r % seq_len of utterance
 *     r / seq_len.  Padding masks are given as per-utterance lengths (int64), a row being
 *     padding when (r % seq_len) >= lens[r / seq_len] (utils/tools.py:155-163).
 *   - dropout is counter-based (Philox4x32-10 keyed by seed, site, element index): the
 *     backward entry points regenerate the forward mask from the same (seed, site).  The
 *     seed is read from DEVICE memory (`const uint64_t* seed`, NULL when p == 0), so a
 *     captured HIP graph of the step draws a new seed per replay (fs2_seed_next).
 */
#ifndef FS2HIP_H
#define FS2HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { FS2_OK = 0, FS2_ERR_ARG = -1, FS2_ERR_LAUNCH = -2, FS2_ERR_DTYPE = -3 };
enum { FS2_F32 = 0, FS2_BF16 = 1 };
/* GEMM epilogue flags */
enum {
  FS2_EPI_BIAS = 1,          /* y += bias[n]                                   */
  FS2_EPI_RELU = 2,          /* y = max(y, 0)                                  */
  FS2_EPI_ADD_AUX = 4,       /* y += aux[m, n]   (residual-gradient fusion)    */
  FS2_EPI_RELU_MASK_AUX = 8, /* y *= (aux[m, n] > 0)   (ReLU backward fusion)  */
  FS2_EPI_OUT_BF16 = 16,     /* bf16 path: store y as bf16 (default fp32)       */
  FS2_EPI_AUX_BF16 = 32,     /* bf16 path: aux is bf16 (default fp32)           */
  /* fs2_conv_gemm_ex only (vocoder, hifigan/models.py), applied after BIAS / ADD_AUX:  */
  FS2_EPI_LRELU = 64,        /* y = y >= 0 ? y : alpha * y                      */
  FS2_EPI_ACC_Y = 128,       /* y = (y + y_old[m, n]) * scale  (y read, then written) */
  FS2_EPI_Y2 = 256,          /* y2[m, n] = y >= 0 ? y : alpha2 * y  (compute dtype) */
  FS2_EPI_SKIP_NOSTORE = 512 /* with lens: skipped row tiles store nothing (y, y2 keep their
                                contents there) -- for consumers that never read those rows */
};

const char* fs2_last_error(void);
int fs2_abi_version(void);

/* ---------------------------------------------------------------- convolution / linear
 * Conv1d over time as an implicit GEMM on (rows, c_in) activations:
 *   y[r, o] = sum_{j, c} wk[o, j*c_in + c] * x[r + j - pad, c]      (zero outside the utterance)
 * dtype FS2_F32: x, wk fp32 (exact f32 MFMA); FS2_BF16: x, wk bf16 (bf16 MFMA, fp32
 * accumulate), y fp32 or bf16 (FS2_EPI_OUT_BF16).
 * A Linear layer is taps=1, pad=0.  Forward uses wk = fs2_conv_weight_prep's w_fwd; the
 * data gradient is the same call on dy with w_bwd (flipped taps, transposed channels).
 * Replaces nn.Conv1d / nn.Linear forward and their input-gradient:
 *   transformer/SubLayers.py:39-41,53,85-89 ; model/modules.py:289-296 ;
 *   transformer/Layers.py:59-64 ; model/fastspeech2.py:25-28,109.
 * lens (nullable, device int64[rows / seq_len]): row r = b*seq_len + t is padding when
 * t >= lens[b].  With lens, output tiles made only of padding rows are not computed: they
 * are written as if their rows were zero and there were no bias (aux under ADD_AUX, 0
 * otherwise) -- for the FFT blocks, whose padded rows are masked (Layers.py:25,28) or carry
 * zero gradient.  fs2_conv_wgrad skips 64-row k-tiles made only of padding rows (their dy
 * rows must be zero).  The fp32 path ignores lens.                                     */
int fs2_conv_gemm(int dtype, const void* x, int64_t ldx, const void* wk, void* y, int64_t ldy,
                  int64_t rows, int64_t seq_len, int64_t c_in, int64_t c_out, int taps, int pad,
                  const int64_t* lens, const float* bias, int flags, const void* aux,
                  int64_t ld_aux, void* stream);

/* bf16 Conv1d / Linear with the FFT block's post-LayerNorm fused into the epilogue
 * (c_out = 256, the LayerNorm width; x, wk bf16 as fs2_conv_gemm):
 *   z[r, :] = dropout(conv(x)[r, :] + bias, p_in) + res[r, :]      (res nullable)
 *   out = (z - mean) * rstd * gamma + beta, out_t = bf16(out) (nullable), xhat, rstd saved;
 *   rows t >= lens[b] are written as 0 (xhat / rstd left unwritten there).
 * Bitwise equal to fs2_conv_gemm (fp32 y, FS2_EPI_BIAS) followed by fs2_ln_fwd(y, res, ...,
 * p_out = 0, no head): one kernel instead of two, and y never goes to memory.  The dropout
 * mask is fs2_ln_fwd's (seed, site_in), so fs2_ln_bwd is its backward.
 * Replaces transformer/SubLayers.py:54-55 (fc, dropout, residual, layer_norm) and :88-91
 * (w_2, dropout, residual, layer_norm).                                                  */
int fs2_conv_gemm_ln(const void* x, int64_t ldx, const void* wk, int64_t rows, int64_t seq_len,
                     int64_t c_in, int64_t c_out, int taps, int pad, const int64_t* lens,
                     const float* bias, const float* res, const float* gamma, const float* beta,
                     float* out, void* out_t, float* xhat, float* rstd, float p_in,
                     const uint64_t* seed, uint64_t site_in, void* stream);
/* The same with the residual in either of two forms: res (fp32, as above), or the LayerNorm
 * that produced it -- res_xhat (rows, 256) with res_gamma / res_beta (256,), masked by the same
 * lens: the residual of row r is res_xhat[r] * res_gamma + res_beta where t < lens[b] and 0
 * where t >= lens[b] (res_xhat is not read there: its producer left those rows unwritten).
 * The producer is a post-LN site (fs2_conv_gemm_ln, or fs2_ln_fwd with p_out = 0, no head).
 * The rebuilt value has the bits that producer wrote (or would have written) to its `out`, so
 * a stack of post-LN sites need not store the fp32 `out` at all: out may be NULL here and in
 * fs2_conv_gemm_ln (no fp32 store; out_t, xhat and rstd as usual).  Give res or the triple,
 * not both.                                                                               */
int fs2_conv_gemm_ln_nres(const void* x, int64_t ldx, const void* wk, int64_t rows,
                          int64_t seq_len, int64_t c_in, int64_t c_out, int taps, int pad,
                          const int64_t* lens, const float* bias, const float* res,
                          const float* res_xhat, const float* res_gamma, const float* res_beta,
                          const float* gamma, const float* beta, float* out, void* out_t,
                          float* xhat, float* rstd, float p_in, const uint64_t* seed,
                          uint64_t site_in, void* stream);

/* bf16 Linear / Conv1d (c_out = 256) whose output is the upstream gradient of a post-
 * LayerNorm, with that LayerNorm's backward in the epilogue:
 *   dout[r, :] = conv(x)[r, :] + aux[r, :]                (aux: fp32 residual gradient, nullable)
 *   then fs2_ln_bwd(dout, xhat, rstd, gamma, ..., p_in, site_in, dres, dres_add, dy_t = the bf16
 *   dy copy, dgamma / dbeta / dbias_in accumulated; p_out = 0, no head, no ReLU input).
 * Against fs2_conv_gemm(FS2_EPI_ADD_AUX) followed by fs2_ln_bwd (the contract its test
 * checks): dres equal to fp32 rounding (the row arithmetic is compiled in another kernel and
 * contracted differently), the bf16 dy copy within 1 bf16 ulp, and the parameter gradients
 * summed from per-32-row block partials in another in-block order.
 * ws: fs2_ln_bwd_ws_bytes(rows, 256).  In the FFT-block backward x is the attention input
 * gradient (dqkv) and the LayerNorm is the PREVIOUS block's FFN post-LN: block i's QKV data
 * gradient and block i-1's first backward op in one launch (transformer/SubLayers.py:38-40,91). */
int fs2_conv_gemm_ln_bwd(const void* x, int64_t ldx, const void* wk, int64_t rows,
                         int64_t seq_len, int64_t c_in, int64_t c_out, int taps, int pad,
                         const int64_t* lens, const float* aux, const float* xhat,
                         const float* rstd, const float* gamma, float* dgamma, float* dbeta,
                         float* dbias_in, float p_in, const uint64_t* seed, uint64_t site_in,
                         float* dres, int dres_add, void* dy_t, float* ws, int64_t ws_bytes,
                         void* stream);

/* Dilated Conv1d with the vocoder epilogue (HiFi-GAN generator, hifigan/models.py:19-178):
 *   v[r, o] = sum_{j, c} wk[o, j*c_in + c] * x[r + j*dilation - pad, c]   (zero outside the
 *   utterance of seq_len rows), then BIAS, ADD_AUX, ACC_Y, LRELU in that order; y stored
 *   (skipped when y is NULL) and, with FS2_EPI_Y2, a second output y2 = leaky_relu(v, alpha2)
 *   in the compute dtype (bf16 for FS2_BF16, fp32 for FS2_F32; ld = c_out): the input copy
 *   of the next convolution (models.py:95-97,157,167).  pad <= (taps-1)*dilation.
 *   ConvTranspose1d(k = 2s, stride s, pad s/2) runs as taps=3, pad=1 over s*c_out phase
 *   columns (see fs2_convT_weight_prep).  lens (optional, device, one per utterance): as
 *   fs2_conv_gemm -- bf16 row tiles made only of rows t >= lens[b] skip the product (their
 *   outputs are the epilogue of a zero accumulator); rows t < lens[b] are exact.  The
 *   vocoder passes its valid length plus the network's receptive radius, so the kept samples
 *   equal the padded-batch result bitwise.  fs2_conv_gemm(...) == fs2_conv_gemm_ex(...,
 *   dilation 1, lens, alpha 0, scale 1, y2 NULL, alpha2 0).                              */
int fs2_conv_gemm_ex(int dtype, const void* x, int64_t ldx, const void* wk, void* y, int64_t ldy,
                     int64_t rows, int64_t seq_len, int64_t c_in, int64_t c_out, int taps, int pad,
                     int dilation, const int64_t* lens, const float* bias, int flags,
                     const void* aux, int64_t ld_aux, float alpha, float scale, void* y2,
                     float alpha2, void* stream);

/* ConvTranspose1d(c_in -> c_out, k = 2*stride, stride, padding = stride/2) weight
 * w (c_in, c_out, k) (hifigan/models.py:127-137) as the equivalent 3-tap Conv1d weight
 * wc (stride*c_out, c_in, 3) over input frames q-1, q, q+1 producing output samples
 * stride*q + ph (column ph*c_out + o):
 *   wc[ph*c_out + o, c, d+1] = w[c, o, ph + stride/2 - stride*d]  if that tap is in [0, k)
 * (else 0), and bias_c[ph*c_out + o] = bias[o].  Feed wc to fs2_conv_weight_prep.        */
int fs2_convT_weight_prep(const float* w, const float* bias, int64_t c_in, int64_t c_out,
                          int stride, float* wc, float* bias_c, void* stream);

/* Fused HiFi-GAN ResBlock1 (hifigan/models.py:21-53) for the narrow stages: one launch runs
 * the block's three (leaky_relu 0.1, dilated conv k, leaky_relu 0.1, conv k, residual add)
 * pairs on an LDS-resident row tile (R = 256 rows at 32 channels, 128 at 64) and folds the
 * stage's running average: v = acc ? (xs + out) * scale : out * scale; xs = v when store_xs;
 * hc = bf16(leaky_relu(v, alpha2)) when hc is given.  x (rows, C) fp32; w1 / w2: HOST arrays
 * of 3 device pointers to fs2_conv_weight_prep bf16 weights (C, k*C); b1 / b2: host arrays
 * of 3 fp32 bias pointers; dil: host array of 3 dilations.  seq_len % R == 0 (tiles inside
 * one utterance; zero padding at its edges as each Conv1d).  lens (optional): tiles made
 * only of rows t >= lens[b] store nothing.  fs2_resblock1_supported() returns 1 when a shape
 * qualifies (channels 32 / 64, receptive radius <= 64 rows), else 0 (not an error code). */
int fs2_resblock1_supported(int64_t channels, int64_t seq_len, int kernel_size, const int* dil);
int fs2_resblock1_fused(const void* x, int64_t rows, int64_t seq_len, int64_t channels,
                        int kernel_size, const int* dil, const void* const* w1,
                        const void* const* w2, const float* const* b1, const float* const* b2,
                        float* xs, int acc, float scale, int store_xs, void* hc, float alpha2,
                        const int64_t* lens, void* stream);

/* HiFi-GAN output head (hifigan/models.py:167-169, utils/model.py:74-90):
 *   wav[r] = tanh(bias + sum_{j<7, c} w[0, c, j] * x[r + j - 3, c])   (zero outside the
 *   utterance), x (rows, c_in) in the compute dtype; wav fp32 and, when pcm is not NULL,
 *   pcm[r] = (int16) (wav[r] * max_wav_value) truncated toward zero as numpy's astype.
 *   lens (optional, device, samples per utterance): rows t >= lens[b] are written as 0.
 *   1 <= c_in <= 64: a 256-row block stages (256 + 6 + 7) * c_in fp32 in LDS, 68,864 B at 64. */
int fs2_vocoder_post(int dtype, const void* x, int64_t rows, int64_t seq_len, int64_t c_in,
                     const int64_t* lens, const float* w, const float* bias, float max_wav_value,
                     float* wav, int16_t* pcm, void* stream);

/* ---------------------------------------------------------------- vocoder training
 * The generator's backward (hifigan/models.py:155-171 under autograd).  The data gradient of
 * every convolution is fs2_conv_gemm_ex on dy with fs2_conv_weight_prep's w_bwd; the entry
 * points below are the rest.
 *
 * Weight (and optionally bias) gradient of a dilated Conv1d, accumulated into the fp32
 * master layout (c_out, c_in, taps):
 *   dw[o, c, j] += sum_r dy[r, o] * x[r + j*dilation - pad, c]   (x zero outside the utterance
 *                                                                 of seq_len rows)
 *   db[o]       += sum_r dy[r, o]                                (db may be NULL)
 * Any c_in, c_out >= 1, 1 <= taps <= 11, dilation >= 1, 0 <= pad <= (taps-1)*dilation;
 * rows = batch x seq_len (anything else is an argument error).  dy
 * (rows, ldy) and x (rows, ldx) are both FS2_F32 (exact f32 MFMA) or both FS2_BF16 (bf16 MFMA,
 * fp32 accumulate).  64 (o) x 64 (j*c_in + c) output tiles; the rows are cut into `splits`
 * equal ranges (a multiple of 32 rows each), one fp32 slab per range in ws, and a second
 * launch adds the slabs to dw / db in a fixed order (eight partial sums, sum g over the
 * ranges g, g + 8, ... ascending, then added for g = 0..7): no atomics, bitwise reproducible
 * for the same inputs.  splits = 1 once the tiles alone fill the device (the wide stages), else up to
 * rows / 128 (the narrow stages' long reductions); fs2_conv_wgrad_dil_ws_bytes holds the rule.
 * The phase form of a transposed conv is taps = 3, pad = 1 over s*c_out columns; fold its
 * result with fs2_convT_wgrad_fold.  Replaces the weight half of ConvolutionBackward for
 * models.py:30-46,113-137.                                                                */
int64_t fs2_conv_wgrad_dil_ws_bytes(int64_t rows, int64_t c_in, int64_t c_out, int taps);
int fs2_conv_wgrad_dil(int dtype, const void* dy, int64_t ldy, const void* x, int64_t ldx,
                       float* dw, float* db, int64_t rows, int64_t seq_len, int64_t c_in,
                       int64_t c_out, int taps, int pad, int dilation, float* ws,
                       int64_t ws_bytes, void* stream);

/* Leaky-ReLU backward: dx[i] (+)= dy[i] * (v[i] > 0 ? 1 : alpha)   (torch's convention at 0).
 * v (dtype FS2_F32 or FS2_BF16) is the saved pre-activation or its leaky-ReLU'd copy -- the
 * same sign for alpha > 0, and the forward already stores the copies as the next conv's input.
 * dy, dx fp32; accumulate != 0 adds to dx.  dx may alias dy.                               */
int fs2_lrelu_bwd(int dtype, const void* v, const float* dy, float* dx, int64_t n, float alpha,
                  int accumulate, void* stream);

/* Backward of fs2_vocoder_post (conv_post + tanh, no lens): g[r] = d_wav[r] (1 - wav[r]^2),
 *   dx[r, c]   = sum_j g[r - j + 3] w[c*7 + j]      (rows of the same utterance only)
 *   dw[c*7+j] += sum_r g[r] x[r + j - 3, c],   db[0] += sum_r g[r]
 * x (rows, c_in) in `dtype`, 1 <= c_in <= 64; wav the saved output; dx fp32 (rows, c_in),
 * nullable.  Blocks of 128 rows put their partial dw / db into ws, a second launch adds them
 * in block order (fixed summation order).                                                 */
int64_t fs2_vocoder_post_bwd_ws_bytes(int64_t rows, int64_t c_in);
int fs2_vocoder_post_bwd(int dtype, const void* x, const float* wav, const float* d_wav,
                         int64_t rows, int64_t seq_len, int64_t c_in, const float* w, float* dx,
                         float* dw, float* db, float* ws, int64_t ws_bytes, void* stream);

/* The inverse index map of fs2_convT_weight_prep: the gradient dwc (stride*c_out, c_in, 3) of
 * the 3-tap phase form goes back to the ConvTranspose1d layout,
 *   dw[c, o, k] += dwc[ph*c_out + o, c, d + 1],  k = ph + stride/2 - stride*d
 * (every k in [0, 2 stride) has exactly one (ph, d)), and
 *   db[o] += sum_ph dbc[ph*c_out + o]   in phase order (dbc, db nullable together).       */
int fs2_convT_wgrad_fold(const float* dwc, const float* dbc, int64_t c_in, int64_t c_out,
                         int stride, float* dw, float* db, void* stream);

/* ---------------------------------------------------------------- language discriminator
 * The --use_clf branch (train.py:168-197): GE2E SpeechEmbedder (speech_embedder_net.py:65-162)
 * and GE2ELoss's BCE term (165-186), fp32.
 * One LSTM layer (nn.LSTM, batch_first, gates i,f,g,o, h0 = c0 = 0) over n_seq sequences of
 * `steps` rows (row n*steps + t): gx = x W_ih^T + bias (bias = b_ih + b_hh; one GEMM), then
 * the recurrence, one launch per step issued from C.  w_ih (4H, c_in) and w_hh (4H, H)
 * natural; hidden a multiple of 256.  Saves h_all, c_all (rows, H) and the activated gates
 * act (rows, 4H).                                                                         */
int fs2_lstm_layer_fwd(const float* x, int64_t n_seq, int64_t steps, int64_t c_in, int64_t hidden,
                       const float* w_ih, const float* bias, const float* w_hh, float* gx,
                       float* h_all, float* c_all, float* act, void* stream);
/* Backward through time: dh_out (rows, H; NULL = 0) is the gradient of the layer's outputs;
 * writes dgates (rows, 4H; pre-activation gate gradients) and, when dx is given,
 * dx = dgates W_ih (rows, c_in; w_ih_t = W_ih^T (c_in, 4H)); w_hh_t = W_hh^T (H, 4H).
 * dc_ws: 2*n_seq*H floats.
 * The weight gradients are a separate entry (fs2_lstm_stack_wgrad, from dgates and h):
 * train.py never steps the discriminator, so its path does not pay for them.           */
int fs2_lstm_layer_bwd(const float* dh_out, int64_t n_seq, int64_t steps, int64_t c_in,
                       int64_t hidden, const float* w_ih_t, const float* w_hh_t, const float* act,
                       const float* c_all, float* dgates, float* dc_ws, float* dx, void* stream);
/* The whole L-layer stack (the GE2E LSTM_stack, nn.LSTM(num_layers = L)) as a wavefront:
 * launch s runs layer l at step s - l, so the stack takes steps + L - 1 launches; the inputs
 * of layers >= 1 are folded into their step kernels.  Layer-major buffers: h_all, c_all
 * (L, rows, H), act (L, rows, 4H); weights w_ih0 (4H, c_in), w_ih_up (L-1, 4H, H) = W_ih of
 * layers 1.., w_hh (L, 4H, H), bias (L, 4H) = b_ih + b_hh; gx (rows, 4H) workspace.  Same
 * results as fs2_lstm_layer_fwd layer by layer, within fp32 summation order.              */
int fs2_lstm_stack_fwd(const float* x, int64_t n_seq, int64_t steps, int64_t c_in,
                       int64_t hidden, int layers, const float* w_ih0, const float* w_ih_up,
                       const float* w_hh, const float* bias, float* gx, float* h_all,
                       float* c_all, float* act, void* stream);
/* Backward of the stack: dh_out (rows, H; NULL = 0) is the top layer's output gradient;
 * writes dgates (L, rows, 4H) and, with dx, dx = dgates_0 W_ih0 (rows, c_in).  Transposed
 * weights: w_ih0_t (c_in, 4H), w_ih_up_t (L-1, H, 4H), w_hh_t (L, H, 4H).
 * dc_ws: L * 2 * n_seq * H floats.                                                      */
int fs2_lstm_stack_bwd(const float* dh_out, int64_t n_seq, int64_t steps, int64_t c_in,
                       int64_t hidden, int layers, const float* w_ih0_t, const float* w_ih_up_t,
                       const float* w_hh_t, const float* act, const float* c_all, float* dgates,
                       float* dc_ws, float* dx, void* stream);
/* Weight gradients of the stack (train_speech_embedder.py), from what the forward and the
 * backward left: x (rows, c_in), h_all (L, rows, H), dgates (L, rows, 4H).  Per layer
 *   dW_ih (4H, c_in_l) = sum_rows dgates^T (x) in_l,   in_0 = x, in_l = h[l-1]
 *   dW_hh (4H, H)      = sum_rows dgates^T (x) h[l][row-1]  (0 at the first step of a sequence)
 *   db    (4H)         = sum_rows dgates     (the gradient of b_ih and of b_hh alike)
 * in the stack's weight layout: dw_ih0 (4H, c_in), dw_ih_up (L-1, 4H, H), dw_hh (L, 4H, H),
 * db (L, 4H).  f32 MFMA; the rows are split over blocks and the slices added in a fixed order,
 * so the result is bitwise repeatable.  beta = 0 overwrites the outputs, beta = 1 adds to them.
 * hidden a multiple of 256, c_in of 4, n_seq, steps >= 1; ws: fs2_lstm_stack_wgrad_ws_bytes. */
int64_t fs2_lstm_stack_wgrad_ws_bytes(int64_t n_seq, int64_t steps, int64_t c_in, int64_t hidden,
                                      int layers);
int fs2_lstm_stack_wgrad(const float* x, const float* h_all, const float* dgates, int64_t n_seq,
                         int64_t steps, int64_t c_in, int64_t hidden, int layers, float* dw_ih0,
                         float* dw_ih_up, float* dw_hh, float* db, int beta, float* ws,
                         int64_t ws_bytes, void* stream);
/* Embedding + domain-classifier head on the last LSTM frame (x row n at x + n*ldx, 256 wide):
 * projection 256->64, L2 norm (emb), Linear 64->64, dropout, ReLU, Linear 64->64, dropout,
 * ReLU, Linear 64->1 (logit).  w*t are the transposed weights (forward), w* the natural
 * ones (backward).  With dx: dx = d(head)/dx for the given demb / dlogit (NULL = 0), the
 * dropout masks regenerated from (seed, site).                                           */
int fs2_clf_head(const float* x, int64_t ldx, int64_t n, const float* wp, const float* wpt,
                 const float* bp, const float* w0, const float* w0t, const float* b0,
                 const float* w1, const float* w1t, const float* b1, const float* w2,
                 const float* b2, float p_drop, const uint64_t* seed, uint64_t site, float* emb,
                 float* logit, const float* demb, const float* dlogit, float* dx, int64_t lddx,
                 void* stream);
/* Weight gradients of that head for the given demb / dlogit (NULL = 0): projection dwp (64, 256),
 * dbp (64); classifier dw0, dw1 (64, 64), db0, db1 (64), dw2 (1, 64), db2 (1).  Same weight
 * operands and regenerated dropout masks as fs2_clf_head; rows added in row order; beta = 0
 * overwrites, beta = 1 adds.  ws: fs2_clf_head_wgrad_ws_bytes(n).                         */
int64_t fs2_clf_head_wgrad_ws_bytes(int64_t n);
int fs2_clf_head_wgrad(const float* x, int64_t ldx, int64_t n, const float* wp, const float* wpt,
                       const float* bp, const float* w0, const float* w0t, const float* b0,
                       const float* w1, const float* w1t, const float* b1, const float* w2,
                       const float* b2, float p_drop, const uint64_t* seed, uint64_t site,
                       const float* demb, const float* dlogit, float* dwp, float* dbp, float* dw0,
                       float* db0, float* dw1, float* db1, float* dw2, float* db2, int beta,
                       float* ws, int64_t ws_bytes, void* stream);
/* GE2E softmax loss of emb (n_spk, m_utt >= 2, dim <= 256) (utils.py:77-90, 126-135,
 * speech_embedder_net.py:173-181): S_jik = w cos(e_ji, c_k) + b, c_k the mean over m_utt, the
 * k = j entry against the exclude-self centroid; loss = sum_ji log(sum_k exp S_jik + 1e-6) -
 * S_jij.  w, b, g device scalars (g = upstream gradient, NULL = 1).  loss, and with demb also
 * demb (n_spk, m_utt, dim), dw, db (each nullable).  ws: fs2_ge2e_softmax_ws_bytes.       */
int64_t fs2_ge2e_softmax_ws_bytes(int64_t n_spk, int64_t m_utt, int64_t dim);
int fs2_ge2e_softmax(const float* emb, int64_t n_spk, int64_t m_utt, int64_t dim, const float* w,
                     const float* b, const float* g, float* loss, float* demb, float* dw,
                     float* db, float* ws, int64_t ws_bytes, void* stream);
/* GE2E contrast loss (hp.model.loss == 'contrast'; utils.py:77-90, 106-124,
 * speech_embedder_net.py:173-179) on the same operands, limits and nullability as
 * fs2_ge2e_softmax.  S_jik as there (w cos + b, each norm clamped at 1e-8, the k = j entry
 * against the exclude-self centroid (sum_i e_ji - e_ji) / (m_utt - 1)), sig = 1 / (1 + exp(-S)),
 *   loss = sum_ji (1 - sig(S_jij)) + sum_ji max_k sig~_jik,
 * sig~_jik = sig(S_jik) for k != j and sig~_jij = 0: the reference zeroes the own-speaker entry
 * in place, so it takes part in the maximum with value 0 and carries no gradient (n_spk = 1:
 * the second sum is 0).  Equal values: the lowest k wins, the index torch.max(dim=2) reports.
 * Gradients: dL/dS_jij = -sig (1 - sig), dL/dS_jik* = +sig (1 - sig) at the winning k*, nothing
 * else; dw = g sum dS cos, db = g sum dS, demb through the cosine into e_ji, the winning
 * centroid's m_utt members and the exclude-self centroid's m_utt - 1 members.  One workgroup,
 * fixed-order reductions, bitwise repeatable.  ws: fs2_ge2e_contrast_ws_bytes (0 on a bad
 * shape).                                                                                 */
int64_t fs2_ge2e_contrast_ws_bytes(int64_t n_spk, int64_t m_utt, int64_t dim);
int fs2_ge2e_contrast(const float* emb, int64_t n_spk, int64_t m_utt, int64_t dim, const float* w,
                      const float* b, const float* g, float* loss, float* demb, float* dw,
                      float* db, float* ws, int64_t ws_bytes, void* stream);
/* Speaker-encoder batches cut on the device (data_load.py:107-110, 122-129):
 *   out[r, t, c] = store[row_off[r] + c * row_stride[r] + row_start[r] + t],  t < len, c < n_mels.
 * A row's source is one utterance stored (n_mels, frames) inside the flat corpus `store`:
 * row_off its element offset (64-bit: a corpus may pass 2^31 elements), row_stride its frame
 * count, row_start the crop start; the caller guarantees row_start + len <= row_stride.  The
 * three descriptor arrays are device memory; out is (n_rows, len, n_mels).  1 <= len <= 256,
 * 1 <= n_mels <= 128, n_rows >= 0 (0: nothing is launched).                               */
int fs2_mel_crop_gather(const float* store, const int64_t* row_off, const int32_t* row_stride,
                        const int32_t* row_start, int64_t n_rows, int64_t n_mels, int64_t len,
                        float* out, void* stream);
/* out[s] = m / ||m||, m the mean of rows seg_start[s] .. seg_start[s + 1] - 1 of x (rows, dim):
 * the d-vector of generate_dvector (train_speech_embedder.py:75-78), one segment per
 * utterance.  seg_start: device int64[n_seg + 1], non-decreasing; rows are added in row order
 * (bitwise repeatable); an empty segment gives NaN, as torch's mean does.  dim <= 1024.    */
int fs2_rows_mean_unit(const float* x, const int64_t* seg_start, int64_t n_seg, int64_t dim,
                       float* out, void* stream);
/* The scoring of test() (train_speech_embedder.py:425-450) for one batch, no host sync.
 * enroll (n_spk, m_enr, dim), verify (n_spk, m_ver, dim), n_spk >= 2, m_ver >= 2, dim <= 256.
 * sim (n_spk, m_ver, n_spk) = get_cossim(verify, get_centroids(enroll)) (utils.py:169-236):
 * the cosine of verification utterance (j, i) with enrolment centroid k, but for k = j with the
 * verification utterances' own exclude-self centroid; every entry + 1e-6.  table (50, 2) = FAR,
 * FRR at thresholds float(0.01 i + 0.5), acceptance is sim > threshold:
 *   FAR = (accepted - accepted same-speaker) / (n_spk - 1) / m_ver / n_spk,
 *   FRR = (n_spk m_ver - accepted same-speaker) / m_ver / n_spk,
 * from integer counts by fp32 divisions in that order.  result[4] = EER = (FAR + FRR) / 2,
 * threshold, FAR, FRR at the first threshold with the strictly smallest |FAR - FRR| below 1;
 * all zeros if none is.  ws: fs2_ge2e_eer_ws_bytes.                                       */
int64_t fs2_ge2e_eer_ws_bytes(int64_t n_spk, int64_t dim);
int fs2_ge2e_eer(const float* enroll, const float* verify, int64_t n_spk, int64_t m_enr,
                 int64_t m_ver, int64_t dim, float* sim, float* table, float* result, float* ws,
                 int64_t ws_bytes, void* stream);
/* Epoch statistics kept on the device (train_speech_embedder.py:193-195, 278-279):
 * totals (float[4]) += [loss[0], da_loss[0], 100 correct / n, 1] with correct =
 * #{round(sigmoid(logit_i)) == y_i} (utils.py:238-247, round half to even).  loss, da_loss and
 * logit are each nullable (their total then stays); correct (nullable) receives the count.   */
int fs2_epoch_stats_add(float* totals, const float* loss, const float* da_loss, const float* logit,
                        const float* y, int64_t n, float* correct, void* stream);
/* The FastSpeech2 training batch cut on the device from a device-resident corpus: what
 * Dataset.reprocess + to_device build on the host (dataset.py:112-172, utils/tools.py:18-125).
 * The corpus is one flat store per field, utterance after utterance: text, dur, accent (int64,
 * src_len[u] entries at element src_off[u]), mel (fp32, mel_len[u] * n_mels entries at element
 * mel_off[u], a multiple of n_mels), pitch (fp32) and energy (energy_bytes = 4: fp32, 8: fp64),
 * each at src_off[u] with src_len[u] entries, or -- *_frame != 0 -- at frame mel_off[u] / n_mels
 * with mel_len[u] entries; meta (n_utt, meta_dim) fp32 and speaker (n_utt) int64.
 * idx: device int32[batch], the utterances of the batch in row order.  Outputs, row b from
 * utterance idx[b], zero past the utterance's length (pad_1D / pad_2D): o_text, o_dur, o_accent
 * (batch, max_src_len) int64; o_mel (batch, max_mel_len, n_mels); o_pitch / o_energy (batch,
 * max_src_len), or (batch, max_mel_len) when frame-level, in their store type; o_src_len,
 * o_mel_len, o_speaker (batch) int64; o_meta (batch, meta_dim).  accent and o_accent are
 * nullable (a 13-tuple batch has no accents).  One launch; every output element is written.
 * Host-side validation before anything is launched or touched (FS2_ERR_ARG): the caller passes
 * HOST copies of the indices (idx_host) and of the two length tables (src_len_host,
 * mel_len_host, int32[n_utt]); batch >= 1, every index in 0..n_utt-1, max_src_len / max_mel_len
 * >= the lengths of every utterance of the batch (larger is allowed: data-parallel shards pad to
 * the ranks' maxima), non-null pointers, n_mels a multiple of 4 and the mel store / output
 * 16-byte aligned (the mel rows move as 16-byte words).  The device tables must hold what the
 * host copies hold.                                                                          */
int fs2_batch_gather(const int32_t* idx, const int32_t* idx_host, int64_t batch, int64_t n_utt,
                     const int32_t* src_len_host, const int32_t* mel_len_host,
                     const int32_t* src_len, const int32_t* mel_len, const int64_t* src_off,
                     const int64_t* mel_off, const int64_t* speaker, const int64_t* text,
                     const int64_t* dur, const int64_t* accent, const float* mel,
                     const float* pitch, const void* energy, const float* meta, int64_t n_mels,
                     int64_t meta_dim, int64_t energy_bytes, int64_t pitch_frame,
                     int64_t energy_frame, int64_t max_src_len, int64_t max_mel_len,
                     int64_t* o_text, int64_t* o_dur, int64_t* o_accent, float* o_mel,
                     float* o_pitch, void* o_energy, int64_t* o_src_len, int64_t* o_mel_len,
                     int64_t* o_speaker, float* o_meta, void* stream);
/* Validation sums kept on the device (evaluate.py:68-72), one call per batch:
 * sums[i] (double[6]) += (double)losses[i] * batch, esum[0] (float) += eloss[0] * batch (the
 * product rounded to fp32 first, as the reference's tensor expression); eloss nullable.      */
int fs2_eval_accum(double* sums, float* esum, const float* losses, const float* eloss,
                   int64_t batch, void* stream);
/* ---- Exact t-SNE of speaker embeddings (train_speech_embedder.py:311-385; the semantics of
 * scikit-learn's TSNE(2, init='pca', method='exact'), Euclidean metric).  fp32 storage; limits
 * for every entry: n <= 4096 points, dim <= 1024, 2 output components.  n = 0 launches nothing.
 * Every accumulation runs in a fixed order (no atomics): results are bitwise repeatable.
 *
 * fs2_tsne_points: out[s] (n, dim) = the plain mean of the first min(count_s, cap) rows of
 * segment s of x (rows, dim), rows seg_start[s] .. seg_start[s + 1] - 1 (device int64[n + 1],
 * non-decreasing), added in row order; no renormalisation (embs[indices, :cap].mean(1)).  An
 * empty segment gives NaN.  cap >= 1.                                                       */
int fs2_tsne_points(const float* x, const int64_t* seg_start, int64_t n, int64_t dim, int64_t cap,
                    float* out, void* stream);
/* Y0 (n, 2) = the PCA initialisation: X centred, the dim x dim covariance and its two leading
 * eigenvectors in fp64 (subspace iteration with a Rayleigh-Ritz rotation, at most 1000 rounds,
 * so it ends on a degenerate spectrum too), each component's sign such that its
 * largest-magnitude loading is positive (svd_flip, V-based), Y0 = Xc V scaled by
 * 1e-4 / std(Y0[:, 0]) (population std).  ws: fs2_tsne_pca_ws_bytes.                          */
int64_t fs2_tsne_pca_ws_bytes(int64_t n, int64_t dim);
int fs2_tsne_pca_init(const float* X, int64_t n, int64_t dim, float* Y0, void* ws,
                      int64_t ws_bytes, void* stream);
/* P (n, n) fp32 = the joint probabilities of _joint_probabilities: squared distances from the
 * direct (x_i - x_j)^2 form (fp64 sums rounded to fp32); per row the binary search of
 * _binary_search_perplexity in fp64 (beta from 1, at most 100 steps, |H - log(perplexity)| <=
 * float(1e-5), doubling / halving while the far bound is infinite, a zero row sum becomes
 * float(1e-8), the diagonal excluded); P = max((C + C^T) / max(sum, eps), eps) with eps the
 * fp64 machine epsilon, zero diagonal.  0 < perplexity < n.  beta (fp64[n]) and P64 (fp64
 * (n, n), P before its rounding) are optional.  ws: fs2_tsne_affinities_ws_bytes.            */
int64_t fs2_tsne_affinities_ws_bytes(int64_t n);
int fs2_tsne_affinities(const float* X, int64_t n, int64_t dim, double perplexity, float* P,
                        double* beta, double* P64, void* ws, int64_t ws_bytes, void* stream);
/* The descent's device record, double[16]: {iteration, stage (1, 2), best error, best
 * iteration, done, n_iter, last evaluated error, first iteration of the stage, gradient norm at
 * the last check, max_iter, exploration_iter, n_iter_without_progress, early_exaggeration,
 * learning_rate, min_grad_norm, 0}.  exploration_iter, max_iter >= 1, 0 < perplexity < n.    */
int fs2_tsne_state_init(double* state, int64_t n, double perplexity, int64_t max_iter,
                        int64_t exploration_iter, int64_t n_iter_without_progress,
                        double early_exaggeration, double learning_rate, double min_grad_norm,
                        void* stream);
/* Phase A of iteration: rowsum[i] (fp64[n]) = sum_{j != i} w_ij, w = 1 / (1 + |y_i - y_j|^2)
 * in fp32, summed in fp64.  state (nullable): returns at once when the record says done.    */
int fs2_tsne_rowsum(const float* Y, int64_t n, const double* state, double* rowsum, void* stream);
/* Phase B of iteration `iter`: Z = sum of rowsum (every block in the same order), q = max(w / Z,
 * eps), grad_i = 4 sum_j (e p_ij - q_ij) w_ij (y_i - y_j); gains += 0.2 where update * grad < 0,
 * else *= 0.8, floor 0.01; grad *= gains; update = momentum update - lr grad; Y_out = Y + update
 * (Y_out != Y: other rows still read Y).  Exaggeration e, momentum (0.5 / 0.8) and lr come from
 * the record's stage; at the first iteration of stage 2 update is read as 0 and gains as 1.
 * gn_rows[i] = the row's share of |gains grad|^2.  On an evaluating iteration ((iter + 1) % 50
 * == 0 or the last iteration of the stage) kl_rows[i] = sum_j e p_ij log(max(e p_ij, eps) /
 * q_ij) of Y (fp64 from the fp32 pair terms; this phase knows Z, so phase A leaves the error
 * to it).  Returns at once when the record says done.                                       */
int fs2_tsne_update(const float* P, const float* Y, float* Y_out, float* update, float* gains,
                    int64_t n, int64_t iter, const double* state, const double* rowsum,
                    double* kl_rows, double* gn_rows, void* stream);
/* One launch per check iteration, per last iteration of a stage: the rules of
 * _gradient_descent on the record with error = sum kl_rows, grad_norm = sqrt(sum gn_rows).  At
 * (iter + 1) % 50 == 0: error < best records a new best, otherwise iter - best_iter > window
 * ends the stage (window: exploration_iter in stage 1, n_iter_without_progress in stage 2);
 * then grad_norm <= min_grad_norm ends it.  The last iteration of a stage (exploration_iter - 1,
 * max_iter - 1) ends it too.  After stage 1, stage 2 starts at iter + 1 with best reset (stage 1
 * runs to exploration_iter whatever max_iter is, as sklearn's; if it ends at or past
 * max_iter - 1 there is no stage 2); after the last stage, done = 1 and n_iter = iter.      */
int fs2_tsne_control(double* state, int64_t n, int64_t iter, const double* kl_rows,
                     const double* gn_rows, void* stream);
/* Phases A and B once on explicit scalars, no record (tests, single steps): always evaluates
 * kl_rows.  fs2_tsne_kl: kl[0] = the error of Y under exaggeration * P, nothing updated.     */
int fs2_tsne_step(const float* P, const float* Y, float* Y_out, float* update, float* gains,
                  int64_t n, double exaggeration, double momentum, double learning_rate,
                  double* rowsum, double* kl_rows, double* gn_rows, void* stream);
int fs2_tsne_kl(const float* P, const float* Y, int64_t n, double exaggeration, double* rowsum,
                double* kl_rows, double* kl, void* stream);
/* out (n, 2) = (Y - min) / (max - min) per column (visualize_embeddings:366); a constant
 * column gives NaN, as numpy does.                                                          */
int fs2_tsne_finish(const float* Y, int64_t n, float* out, void* stream);
/* The mel front end (preprocessor/preprocessor.py:330-336; common/layers.py:101-123 over
 * common/stft.py) of a ragged batch in one launch: wav (batch, samples) fp32, lens (device
 * int64, nullable = samples for every row; read clamped into [1, samples]).  Per row, frames
 * f < n_frames = 1 + len / hop of the centred STFT (n_fft = win_length = 1024, reflect padding
 * of 512 resolved against the row's own len: index -k is k, len - 1 + k is len - 1 - k, every
 * index clamped into [0, len - 1]); F_max = 1 + samples / hop:
 *   mag    (batch, 513, F_max)  |STFT| (nullable)
 *   energy (batch, F_max)       ||mag[:, f]||_2 (nullable)
 *   mel    (batch, n_mels, F_max)  log(max(filterbank . mag, 1e-5))
 * and zeros at f >= n_frames.  window (1024) fp32; twiddle (1024, 2) fp32 = cos, -sin of
 * 2 pi k / 1024 rounded from fp64; the filterbank in compressed form: filter c weighs bins
 * fb_first[c] .. fb_first[c] + fb_count[c] - 1 with fb_w[fb_off[c] ..] (device int32 x 3,
 * n_weights floats; ranges are clamped to the 513 bins and the n_weights floats).  clip != 0
 * clamps the samples to [-1, 1] on load; log_mag != 0 stores log(max(mag, 1e-5)) in mag
 * (linear_spectrogram, layers.py:120-123).  1 <= hop <= 1024, n_mels <= 128; any other n_fft is
 * an argument error.  A frame's result does not depend on its place in the batch.         */
int fs2_melspec(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                int64_t n_fft, int64_t hop, const float* window, const float* twiddle,
                const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                const float* fb_w, int64_t n_weights, int64_t n_mels, int clip, int log_mag,
                float* mel, float* energy, float* mag, int64_t* n_frames, void* stream);
/* The exact adjoint of fs2_melspec's mel output (clip = 0, log_mag = 0) for the vocoder's mel
 * loss: wav, lens and the tables as fs2_melspec takes them, d_mel (batch, n_mels, F_max) the
 * cotangent of mel (entries at f >= n_frames are not read), d_wav (batch, samples) its pull-back
 * (zeros at t >= len).  Each live frame's spectrum is recomputed as fs2_melspec computes it;
 * then the log clamp (zero where filterbank . mag <= 1e-5, else 1 / it), the filterbank (bin
 * k sums its filters in ascending order), the modulus (dX = dmag X / |X|, 0 where |X| = 0),
 * the adjoint of the one-sided transform (d frame[n] = Re sum_{k=0}^{512} dX[k] e^{+2 pi i k n
 * / 1024}: bins 0 and 512 are real and count once, which is not irfft's weighting) and the
 * window.  The windowed frames go to ws (batch, F_max, 1024); a second launch sums, per
 * sample t, every (frame, offset) that fs2_melspec's index rule maps to t -- the position
 * itself, its reflections about 0 and len - 1 and, at t = 0, everything the final clamp sends
 * there -- frames ascending.  No atomics: a row's result is bitwise batch invariant.
 * 128 <= hop <= 512 (the LDS plan of the Griffin-Lim step), n_mels <= 128.                 */
int64_t fs2_melspec_bwd_ws_bytes(int64_t batch, int64_t samples, int64_t hop);
int fs2_melspec_bwd(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                    int64_t n_fft, int64_t hop, const float* window, const float* twiddle,
                    const int32_t* fb_first, const int32_t* fb_count, const int32_t* fb_off,
                    const float* fb_w, int64_t n_weights, int64_t n_mels, const float* d_mel,
                    float* d_wav, float* ws, int64_t ws_bytes, void* stream);
/* loss[0] = mean_i |a[i] - b[i]| as a device scalar and, when d_a is given,
 * d_a[i] = sign(a[i] - b[i]) / n (0 at equality).  Fixed order: with P = min(1024, ceil(n /
 * 256)) blocks, thread t of block p sums elements i = 256 p + t + 256 P m (m ascending), the
 * block reduces them as a binary tree into its partial in ws; a second launch adds the P
 * partials in order and divides.  All sums in fp64: the loss is the correctly rounded mean.
 * ws: fs2_mel_l1_ws_bytes() bytes.                                                        */
int64_t fs2_mel_l1_ws_bytes(void);
int fs2_mel_l1(const float* a, const float* b, int64_t n, float* loss, float* d_a, float* ws,
               int64_t ws_bytes, void* stream);
/* Griffin-Lim (common/audio_processing.py:86-102 over STFT.inverse, common/stft.py:107-137, and
 * TacotronSTFT._mel_to_linear, common/layers.py:125-131): the inverse half of fs2_melspec's
 * transform pair.  Built for n_fft = win_length = 1024 (513 bins) and 128 <= hop <= 512; anything
 * else is an argument error.  Ragged convention: n_frames (batch) device int64, nullable =
 * frames, read clamped into [0, frames]; row b has F_b live frames and L_b = hop (F_b - 1)
 * samples (0 for F_b <= 1); waveforms are (batch, hop (frames - 1)) fp32 and everything past L_b
 * is written as exact zeros.  A row's result depends on that row's data only and is bitwise
 * batch invariant (no atomics, fixed summation orders).  Nothing allocates or synchronises.
 *
 * fs2_mel_to_linear: mel (batch, n_mels, frames) holds LOG-mels,
 *   mag[b, k, f] = max(sum_m inv_basis[k, m] exp(mel[b, m, f]), 1e-10),
 * one fp32 accumulator, m ascending; inv_basis (513, n_mels) fp32 (audio.inverse_mel_basis);
 * mag (batch, 513, frames), zeros at f >= F_b.  n_mels <= 128.
 *
 * fs2_istft: mag and phase (nullable = zero phase) are (batch, 513, frames); window (1024) and
 * twiddle (1024, 2) as fs2_melspec takes them.  With p the position before the trim,
 *   y[p]   = sum_f w[p - f hop] irfft_1024(mag[:, f] e^(i phase[:, f]))[p - f hop]
 *            / sum_f w^2[p - f hop],
 * both sums over the frames f < F_b that cover p, f ascending, and wav[t] = y[t + 512] for
 * t < L_b.  The irfft uses only the real parts of bins 0 and 512.  The reference's inverse basis
 * pinv(scale fourier_basis) is this irfft times hop / n_fft and its later factor n_fft / hop
 * cancels that; both are dropped.  Its `window_sum > tiny` exception is not made: for
 * 128 <= hop <= 512 every kept position is covered by a frame at an offset with w^2 > 0 (the
 * periodic Hann window vanishes at offset 0 only), so the divisor is positive throughout.
 *
 * fs2_griffin_lim_step: one pass of the loop body (audio_processing.py:100-101).  Per live frame
 * the span of wav_in is taken by fs2_melspec's index rule (reflection against L_b), windowed and
 * transformed to X[k]; X'[k] = mag[k] X[k] / |X[k]|, and (mag[k], 0) where |X[k]| = 0 (the
 * reference's atan2(0, 0) = 0); then the inverse transform, the window and the overlap-add of
 * fs2_istft.  wav_out must not overlap wav_in.
 *
 * ws (fs2_griffin_lim_ws_bytes: (batch, frames, 1024) fp32) is the caller's and receives the
 * windowed inverse frames; a second launch sums them per sample.  batch = 0 launches nothing. */
int fs2_mel_to_linear(const float* mel, const int64_t* n_frames, int64_t batch, int64_t n_mels,
                      int64_t frames, const float* inv_basis, float* mag, void* stream);
int64_t fs2_griffin_lim_ws_bytes(int64_t batch, int64_t frames);
int fs2_istft(const float* mag, const float* phase, const int64_t* n_frames, int64_t batch,
              int64_t frames, int64_t n_fft, int64_t hop, const float* window,
              const float* twiddle, float* wav, float* ws, int64_t ws_bytes, void* stream);
int fs2_griffin_lim_step(const float* wav_in, const float* mag, const int64_t* n_frames,
                         int64_t batch, int64_t frames, int64_t n_fft, int64_t hop,
                         const float* window, const float* twiddle, float* wav_out, float* ws,
                         int64_t ws_bytes, void* stream);
/* The F0 contour of a ragged batch by YIN (de Cheveigne & Kawahara 2002), the estimator that
 * stands where preprocessor/preprocessor.py:196-201 calls pyworld (no parity with DIO is
 * claimed).  wav (batch, samples) fp32, lens (device int64, nullable = samples; read clamped
 * into [0, samples]).  Per row, frames k < n_frames = 1 + len / hop centred at k hop (the
 * frames of fs2_melspec); F_max = 1 + samples / hop; W = 512 (compiled in),
 * tau_max = floor(sr / f0_floor) <= 512, tau_min = ceil(sr / f0_ceil) >= 1, L = W + tau_max:
 *   s[j]     = wav[k hop - L / 2 + j], 0 <= j < L, zero outside [0, len)
 *   d(tau)   = sum_{j < W} (s[j] - s[j + tau])^2, fp32, j ascending, no fused multiply-add
 *   d'(0)    = 1, d'(tau) = d(tau) tau / sum_{1 <= j <= tau} d(j) (1 where that sum is 0)
 *   tau      = the first in [tau_min, tau_max] with d'(tau) < threshold, advanced while
 *              d'(tau + 1) < d'(tau); none: f0 = 0, dip = min d' over the range
 *   dip      = d'(tau); for 1 <= tau < tau_max a parabola through d'(tau - 1 .. tau + 1) moves
 *              tau by 0.5 (a - c) / (a - 2 b + c), clamped to +-1, 0 unless the curvature is
 *              positive; f0 = sr / (tau + offset), 0 when outside [f0_floor, f0_ceil]
 * f0, dip (batch, F_max) fp32, zeros at k >= n_frames; n_frames (batch) int64.  A frame's
 * result depends on its samples only, never on its place in the batch.                     */
int fs2_f0_yin(const float* wav, const int64_t* lens, int64_t batch, int64_t samples, int64_t hop,
               double sr, double f0_floor, double f0_ceil, double threshold, float* f0, float* dip,
               int64_t* n_frames, void* stream);
/* The F0 contour by pYIN (Mauch & Dixon, ICASSP 2014): every threshold of a prior distribution
 * votes for the pick fs2_f0_yin would make at it, and a Viterbi pass over (pitch bin, voiced /
 * unvoiced) states picks the track.  Opt-in beside fs2_f0_yin; nothing is compared with librosa's
 * or the authors' code.  wav, lens, the frames, s[j], d(tau), d'(tau), tau_min, tau_max, W = 512,
 * the descent, the parabola and the [f0_floor, f0_ceil] test are exactly those of fs2_f0_yin
 * (the same fp32 operations in the same order, no fused multiply-add).
 *
 * Candidates (fs2_f0_pyin_candidates).  Thresholds theta_i = float32(i / 100), i = 1..100, with
 * prior (100) fp64 holding w_i = I(theta_i) - I(theta_(i-1)), I the Beta(2, 18) CDF
 * 1 - (1 - x)^19 - 19 x (1 - x)^18 (audio.pyin_tables).  Threshold i picks the first tau in
 * [tau_min, tau_max] with d'(tau) < theta_i, advanced while d'(tau + 1) < d'(tau), with mass w_i;
 * if no tau qualifies, the first argmin of d' over the range with mass w_i * 0.01 (one fp64
 * product) -- and no mass at all unless d' there is below 1: where a frame has no energy d' is 1
 * by convention, and such a frame votes for nothing.  The pick is refined by the parabola; an f0 outside [f0_floor, f0_ceil] drops its
 * mass (it counts as unvoiced), otherwise its bin is
 *   b = clamp(rint(60 log2((double)f0 / (double)(float)f0_floor)), 0, n_bins - 1)   (fp64),
 * 60 = 12 semitones of 5 bins; the caller passes n_bins = floor(60 log2(f0_ceil / f0_floor)) + 1
 * (210 for 71..800 Hz), 1 <= n_bins <= 1024.  Per live frame:
 *   mass[b]    = the fp64 sum of the masses of the thresholds picking bin b, i ascending
 *   cand_f0[b] = the f0 of the lowest such i (fp32), 0 for a bin nobody picked
 *   voiced     = min(sum_b mass[b], 1), one fp64 accumulator, b ascending
 *   unvoiced   = (float)(1 - voiced) (nullable): small means strongly periodic, as dip
 * mass (batch, F_max, n_bins) fp64, cand_f0 (batch, F_max, n_bins) fp32, voiced (batch, F_max)
 * fp64, unvoiced (batch, F_max) fp32, all zeros at k >= n_frames; n_frames (batch) int64.
 *
 * Viterbi (fs2_f0_pyin_viterbi) over the states s = b (voiced) and n_bins + b (unvoiced), in
 * the probability domain with no logarithms.  mass (batch, frames, n_bins) and voiced (batch,
 * frames) fp64 as above; n_frames (batch) device int64, nullable = frames, read clamped into
 * [0, frames]; tri (reach + 1) fp64 with tri(d) = (R + 1 - d) / (R + 1)^2 for the reach
 * R = round(35.92 * 60 * hop / sr) (25 at hop 256 and 22 050 Hz), 0 <= R <= 1023.
 *   obs_k(b)          = mass_k[b] + 1e-9;  obs_k(n_bins + b) = (1 - voiced_k) / n_bins + 1e-9
 *   P((b', v')|(b, v)) = tri(|b' - b|) * (0.99 if v' = v else 0.01) for |b' - b| <= R, else 0;
 *                       what leaves the bin range at the edges is not redistributed
 *   delta_0           = obs_0 / (2 n_bins), then divided by its maximum
 *   delta_k(s')       = (max_s delta_(k-1)(s) * P(s'|s)) * obs_k(s'), then the frame is divided
 *                       by its maximum
 * every operation one IEEE fp64 multiply, divide or compare (no fused multiply-add), so numpy
 * gives the same bits.  Ties go to the lowest predecessor and the lowest final state (numpy's
 * argmax); the path is traced back from frame n_frames - 1.  path (batch, frames) int32
 * receives the states, -1 at k >= n_frames.  With f0 (batch, frames) fp32 (nullable; it needs
 * cand_f0 and centres (n_bins) fp32 = float32(f0_floor 2^(b / 60))): 0 for an unvoiced state,
 * cand_f0_k[b] for a voiced one where that is non-zero, else centres[b]; 0 at k >= n_frames.
 * ws (fs2_f0_pyin_viterbi_ws_bytes) holds int16 back-pointers (batch, frames, 2 n_bins).
 *
 * fs2_f0_pyin runs both stages on the stream: f0 and unvoiced (batch, F_max) fp32, n_frames
 * (batch) int64, states (batch, F_max) int32 (nullable), ws of fs2_f0_pyin_ws_bytes.  A row's
 * result never depends on its place in the batch.  batch = 0 launches nothing; bad arguments are
 * FS2_ERR_ARG before any launch; lens is never read back.                                    */
int fs2_f0_pyin_candidates(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                           int64_t hop, double sr, double f0_floor, double f0_ceil,
                           const double* prior, int64_t n_bins, double* mass, float* cand_f0,
                           double* voiced, float* unvoiced, int64_t* n_frames, void* stream);
int64_t fs2_f0_pyin_viterbi_ws_bytes(int64_t batch, int64_t frames, int64_t n_bins);
int fs2_f0_pyin_viterbi(const double* mass, const double* voiced, const int64_t* n_frames,
                        int64_t batch, int64_t frames, int64_t n_bins, const double* tri,
                        int64_t reach, const float* cand_f0, const float* centres, int* path,
                        float* f0, void* ws, int64_t ws_bytes, void* stream);
int64_t fs2_f0_pyin_ws_bytes(int64_t batch, int64_t samples, int64_t hop, int64_t n_bins);
int fs2_f0_pyin(const float* wav, const int64_t* lens, int64_t batch, int64_t samples, int64_t hop,
                double sr, double f0_floor, double f0_ceil, const double* prior, const double* tri,
                int64_t reach, const float* centres, int64_t n_bins, float* f0, float* unvoiced,
                int64_t* n_frames, int* states, void* ws, int64_t ws_bytes, void* stream);
/* Rational polyphase FIR resampling of a ragged batch, where preprocessor/preprocessor.py:186
 * calls librosa.load(sr=22050) (no parity with resampy's interpolated filter table is claimed).
 * wav (batch, samples) fp32, lens (device int64, nullable = samples; read clamped into
 * [0, samples]); up = L and down = M coprime (sr_out / gcd, sr_in / gcd); table (2 half + 1)
 * fp32 = L h[i], h the low-pass filter centred at i = half (audio.resample_filter).  Per row,
 * n_out = ceil(len L / M) and
 *   y[n] = sum_j table[n M + half - j L] x[j],  0 <= n < n_out,
 * over the j in [0, len) whose table index lies in [0, 2 half], j ascending, one fp32
 * accumulator, every product rounded before it is added (no fused multiply-add).  Nothing past
 * len is read.  out_first, out_count (device int64, nullable = 0 and everything after
 * out_first; read clamped into [0, n_out] and [0, min(n_out - first, out_samples)]) select a
 * window: out (batch, out_samples) fp32 receives y[first + n] for n < count and zeros after,
 * out_lens (batch) int64 the count.  A sample's value depends on its row's samples only: not
 * on the batch, the window or the call.  samples < 2^30; batch * ceil(out_samples / 256) <
 * 2^31 suffices (a tile is 256 outputs or more); the sample span of 256 outputs
 * (255 M / L + 2 half / L + 3) at most 12 288.                                             */
int fs2_resample(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                 const float* table, int64_t table_len, int64_t up, int64_t down, int64_t half,
                 const int64_t* out_first, const int64_t* out_count, float* out,
                 int64_t out_samples, int64_t* out_lens, void* stream);
/* librosa.effects.split of a ragged batch (Multilingual-Speaker-Encoder-with-Domain-Adaptation/
 * data_preprocess.py:46; the rule is librosa 0.7.2's, read from its source, nothing was compared
 * with it).  wav (batch, samples) fp32, lens (device int64, nullable = samples; read clamped
 * into [0, samples]); frame_length even in 2..4096, 1 <= hop <= frame_length.  Per row, frames
 * f < n_f = 1 + len / hop (0 for len = 0); frame f covers the padded samples
 * f hop - frame_length / 2 .. + frame_length - 1.  pad_mode 0 is reflect padding (librosa
 * 0.7.2's rms) by the index rule of fs2_melspec: index -k is k, len - 1 + k is len - 1 - k, every
 * index clamped into [0, len - 1] -- numpy's reflect for len > frame_length / 2, a stated
 * deviation for shorter rows; pad_mode 1 is zero padding (librosa >= 0.10).
 *   p_f   = (sum of the frame's squares) / frame_length: fp32, each square rounded once (no
 *           fused multiply-add), 64 interleaved partial sums (sample i in partial i mod 64,
 *           ascending) joined by a fixed butterfly, so p_f depends on the frame's samples only
 *   p_max = max_f p_f
 *   frame f is non-silent iff max(1e-10, p_f) > max(1e-10, p_max) 10^(-top_db / 10), in fp64:
 *           10 log10(max(1e-10, p_f)) - 10 log10(max(1e-10, p_max)) > -top_db
 * The maximal runs [f0, f1) of non-silent frames, in order, are the intervals
 * [min(f0 hop, len), min(f1 hop, len)].  n_intervals (batch) int32 receives the true count;
 * intervals (batch, max_intervals, 2) int64 the first max_intervals of them and ZEROS after the
 * count.  power (batch, F_max = 1 + samples / hop) fp32, nullable, receives p_f and zeros at
 * f >= n_f; without it ws (fs2_nonsilent_split_ws_bytes) holds the powers, with it ws may be
 * NULL.  At top_db = 100 every row with |x| < 1 is the single interval [0, len].  samples <
 * 2^30.  A row's result does not depend on its place in the batch.                          */
int64_t fs2_nonsilent_split_ws_bytes(int64_t batch, int64_t samples, int64_t hop);
int fs2_nonsilent_split(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                        int64_t frame_length, int64_t hop, double top_db, int pad_mode,
                        int64_t* intervals, int64_t max_intervals, int32_t* n_intervals,
                        float* power, float* ws, int64_t ws_bytes, void* stream);
/* Intervals as rows for fs2_melspec (data_preprocess.py:56):
 *   out[s, i] = wav[seg_row[s], seg_first[s] + i], i < seg_len[s], and 0 up to out_samples.
 * wav (batch, samples) fp32; the descriptors are device int32 / int64 / int64, one per segment;
 * the caller guarantees seg_first + seg_len <= samples and seg_len <= out_samples (they are
 * read clamped to that, so a broken descriptor reads nothing outside wav).  out (n_seg,
 * out_samples) fp32.  n_seg = 0 launches nothing.                                          */
int fs2_wave_segments(const float* wav, int64_t batch, int64_t samples, const int32_t* seg_row,
                      const int64_t* seg_first, const int64_t* seg_len, int64_t n_seg, float* out,
                      int64_t out_samples, void* stream);
/* The half-overlapping windows of data_preprocess.py:63-66.  mel (rows, n_mels, frames) fp32 as
 * fs2_melspec writes it, n_frames (rows) device int64 (read clamped into [0, frames]).  Row r
 * with F = n_frames[r] yields the windows j = 0, 1, ... while 2 F >= tisv (j + 2):
 * mel[r, :, s_j : s_j + tisv], s_j = floor(tisv j / 2) -- the reference's float loop
 * `i += 0.5; int(tisv * i)` in integers, floor(2 F / tisv) - 1 windows for F >= tisv, else none.
 * win_off (rows + 1) device int64: the exclusive prefix of those counts, from the host (which
 * knows every F); n_windows = win_off[rows].  out (n_windows, n_mels, tisv) fp32; a window the
 * offsets promise and the row lacks is written as zeros.  tisv <= 256, n_mels <= 128;
 * n_windows = 0 launches nothing.                                                          */
int fs2_tisv_windows(const float* mel, const int64_t* n_frames, int64_t rows, int64_t n_mels,
                     int64_t frames, int64_t tisv, const int64_t* win_off, int64_t n_windows,
                     float* out, void* stream);
/* preprocessor.py:213-221 in place: per row of x (batch, frames) fp32 with n[b] live frames
 * (device int64, nullable = frames; clamped into [0, frames]), every zero frame becomes the
 * line between its non-zero neighbours (fp64, rounded once), the first non-zero value before
 * it and the last after it; ok[b] (int32) = count_nonzero > 1, and a row with ok = 0 is left
 * as it was (the reference returns None there, line 204).  frames <= 15360.                */
int fs2_pitch_fill(float* x, const int64_t* n, int64_t batch, int64_t frames, int32_t* ok,
                   void* stream);
/* preprocessor.py:223-242: out[b, i] = mean(x[b, pos : pos + d[b, i]]) (fp64 sum, rounded once)
 * or 0 where d = 0, pos the running sum of d; durations (batch, phones) int64, n as above.
 * The reference's in-place order is kept: x[b, i] is overwritten with the mean as it goes (for
 * i < frames), so a phoneme whose pos fell behind i after zero durations averages values already
 * written.  The slice is cut at n[b] as numpy cuts it; an empty slice of a non-zero duration
 * gives NaN as np.mean does.  frames <= 15360.                                             */
int fs2_segment_mean(float* x, const int64_t* n, const int64_t* durations, int64_t batch,
                     int64_t frames, int64_t phones, float* out, void* stream);
/* remove_outlier (preprocessor.py:307-315) then StandardScaler.partial_fit (94-97) per row, rows
 * in order: sorted (batch, cols) fp32 ascending with n[b] live values first; the 25th and 75th
 * percentiles by numpy's linear rule in fp64, survivors lower < v < upper, their count, mean and
 * M2 in fp64, merged into state (device double[3] = n, mean, M2) by Chan's formula.  A row with
 * no survivor contributes nothing.                                                        */
int fs2_outlier_moments(const float* sorted, const int64_t* n, int64_t batch, int64_t cols,
                        double* state, void* stream);
/* normalize (preprocessor.py:317-328): x[b, i] = (x[b, i] - mean) / std (fp64, rounded once) over
 * i < n[b], and minmax (device double[2]) = min, max of itself and the stored values.      */
int fs2_normalize_minmax(float* x, const int64_t* n, int64_t batch, int64_t cols, double mean,
                         double std, double* minmax, void* stream);
/* BCEWithLogits per row (loss_rows, nullable) and dlogit = g[0] * scale * (sigmoid - y)
 * (g nullable = 1).                                                                      */
int fs2_bce_logits(const float* logit, const float* y, int64_t n, float* loss_rows,
                   const float* g, float scale, float* dlogit, void* stream);
/* (batch, t_src, c) rows -> (batch, t_dst, c): copy the first min(t_src, t_dst) frames,
 * zero the rest (the 150-frame chunking of train.py:178-183 and its gradient).          */
int fs2_rows_repad(const float* src, int64_t batch, int64_t t_src, int64_t t_dst, int64_t c,
                   float* dst, void* stream);
/* y[b*rep + k] = meta[b*ld + col] (per-chunk language labels, train.py:184).             */
int fs2_repeat_col(const float* meta, int64_t batch, int64_t ld, int col, int rep, float* y,
                   void* stream);

/* Weight re-layout (and cast for bf16) of a (c_out, c_in, taps) fp32 master weight:
 *   w_fwd[o, j*c_in + c]        = w[o, c, j]
 *   w_bwd[c, j*c_out + o]       = w[o, c, taps-1-j]      (either output may be NULL)     */
int fs2_conv_weight_prep(int dtype, const float* w, int64_t c_out, int64_t c_in, int taps,
                         void* w_fwd, void* w_bwd, void* stream);
/* The same for every layer of the model in one launch: jobs (device, int64) holds
 * n_jobs rows {w, c_out, c_in, taps, w_fwd, w_bwd, first, end}: the job's tiles
 * [first, end) of ceil(c_out/64) * ceil(c_in/CT) tiles, numbered consecutively over the
 * jobs, CT = fs2_weight_prep_tile_channels(dtype); n_tiles = end of the last job; taps <= 9. */
int fs2_weight_prep_tile_channels(int dtype);
int fs2_weight_prep_batch(int dtype, const int64_t* jobs, int n_jobs, int64_t n_tiles,
                          void* stream);

/* Kernel-selection knobs for benchmarking (0 = automatic choice, the default).  Variants that
 * measured slower or neutral were removed in round 4 (their A/B records stay in profiles/).
 * The conv / GEMM knobs are read in one place, the planner (csrc/conv_plan.hpp), which maps a
 * shape and these knobs to a kernel; fs2_debug_conv_plan prints its answer.
 *   FS2_TUNE_GEMM_STAGES   fwd/dX LDS stages (1..4) of the tap-major kernel
 *   FS2_TUNE_WGRAD_STAGES  weight-gradient LDS stages (1..4) of the tap-major wgrad kernel
 *   FS2_TUNE_WGRAD_TILE    weight-gradient tile width (64 or 128) of the tap-major wgrad kernel
 *   FS2_TUNE_WGRAD_SPLITS  weight-gradient row splits (1..64) of the split-K wgrad kernels
 *   FS2_TUNE_RESERVED_4    (was FS2_TUNE_LEGACY_GEMM: the register-staged bf16 kernels of round
 *                          1, removed; setting it to a non-zero value is FS2_ERR_ARG)
 *   FS2_TUNE_NT_GROUP      fwd/dX n-tiles per L2 tile group
 *   FS2_TUNE_NT_HALO       fwd/dX Conv1d (taps > 1) halo kernel: 0 = automatic (8-wave 256 x 128
 *                          tiles for the wide c_in <= 256 forward shapes, else 4-wave tiles by
 *                          grid size), 1 = 4-wave tiles only, 2 = force 128-wide 4-wave tiles,
 *                          -1 = off (tap-major kernel)
 *   FS2_TUNE_WGRAD_HALO    weight gradient of Conv1d taps 3/5/9: 0 = the slab-free band kernel
 *                          where its 32 x 32 output tiles fill the chip, else the split-K halo
 *                          kernel (default), 1 = the split-K halo kernel, -1 = tap-major kernel
 *   FS2_TUNE_HALO_SPLITK   64x64 halo fwd/dX on an under-filled grid (long-K encoder data
 *                          gradient): 0 = automatic channel-block split (128x64 tiles when
 *                          T % 128 == 0), -1 = off, -2 = 64x64 tiles only, n = n splits
 *   FS2_TUNE_ATTN          bf16 attention: 0 = two 16-row groups per wave in the forward
 *                          and dQ (delta fused) kernels at T >= 256, one 16-key group per wave
 *                          at two workgroups per CU in dK/dV (automatic), -1 = one group
 *                          everywhere, 1 = as 0 with the one-workgroup-per-CU dK/dV build,
 *                          2 = two groups in dK/dV too, 3 = dK/dV at three workgroups per CU
 *   FS2_TUNE_NT_TILE       tap-major fwd/dX kernel (k = 1 projections, odd shapes): 0 = tile
 *                          by grid size, 1 / 2 / 3 = force 128x128 / 128x64 / 64x64
 *   FS2_TUNE_LN_TILE       fs2_conv_gemm_ln(_bwd) row tile: 0 = 64 x 256 (default), 1 = 128 x 256
 *   FS2_TUNE_WGRAD_K1      k = 1 weight gradient: 0 = the grouped split-K kernel of
 *                          fs2_conv_wgrad_k1_multi with one job (default), -1 = the tap-major kernel
 *   FS2_TUNE_NT_K1         k = 1 projections on the tap-major kernel: 0 = buffer-descriptor
 *                          staging build (default), -1 = the general tap-walking build (A/B)
 *   FS2_TUNE_ATTN_DMA      bf16 attention at T >= 256: 0 = K / V (Q / dO) tiles by LDS-DMA into
 *                          a 2-slot ring, exp2-folded softmax (default), 1 = 3-slot forward ring
 *                          at one workgroup per CU, -1 = the register-staged kernels (A/B)
 *   FS2_TUNE_TAPREG        fwd/dX Conv1d taps 5 / 9 (C_in % 64 == 0, T and rows % 128 == 0):
 *                          0 = the tap-register halo kernel where its grid fills the chip
 *                          (default: 4-wave 128 x 64 tiles at 3 blocks per CU, 128 x 128 at 2 for
 *                          c_out <= 256), -1 = off (the halo kernels above), 1 = force the
 *                          128 x 64 tiles, 3 = force 128 x 128
 *   FS2_TUNE_WGRAD_BAND    band weight gradient (taps 9, and taps 3 / 5 whose channels are not
 *                          64-multiples): 0 = default, 3 = only on grids of >= 128 tiles,
 *                          4 = the band kernel for taps 3 / 5 with 64-multiple channels too
 *   FS2_TUNE_ATTN_XCD      LDS-DMA attention kernels: 0 = the blocks of one (utterance, head) on
 *                          one XCD (K / V reuse in its L2; default), -1 = the launch grid's order
 *   FS2_TUNE_WGRAD_K1M_STAGES  grouped k = 1 weight gradient LDS ring: 0 = 4 slots, 2 / 3 slots
 *   FS2_TUNE_WGRAD_WIDE    weight gradient of Conv1d taps 3/5/9 (T % 64 == 0) on the wide-tile
 *                          kernel (64 x 64 x taps tiles, row splits to ~256 blocks): 0 = where a
 *                          channel count is not a 64-multiple (default), 1 = wherever eligible,
 *                          -1 = off (band / split-K halo kernels), n > 1 = everywhere, n splits
 * Process-wide; query workspace sizes after setting.                                 */
enum { FS2_TUNE_GEMM_STAGES = 0, FS2_TUNE_WGRAD_STAGES = 1, FS2_TUNE_WGRAD_TILE = 2,
       FS2_TUNE_WGRAD_SPLITS = 3, FS2_TUNE_RESERVED_4 = 4, FS2_TUNE_NT_GROUP = 5,
       FS2_TUNE_NT_HALO = 6, FS2_TUNE_WGRAD_HALO = 7, FS2_TUNE_HALO_SPLITK = 8,
       FS2_TUNE_ATTN = 9, FS2_TUNE_NT_TILE = 10, FS2_TUNE_LN_TILE = 11, FS2_TUNE_WGRAD_K1 = 12,
       FS2_TUNE_NT_K1 = 13, FS2_TUNE_ATTN_DMA = 14, FS2_TUNE_TAPREG = 15,
       FS2_TUNE_WGRAD_BAND = 16, FS2_TUNE_ATTN_XCD = 17, FS2_TUNE_WGRAD_K1M_STAGES = 18,
       FS2_TUNE_WGRAD_WIDE = 19, FS2_TUNE_COUNT = 20 };
int fs2_set_tuning(int knob, int value);

/* Which kernel a bf16 conv / GEMM call of this shape runs under the current knobs (debug; host
 * only: nothing is launched and no GPU is needed).  op: FS2_PLAN_GEMM (fs2_conv_gemm / _ex),
 * FS2_PLAN_GEMM_LN, FS2_PLAN_GEMM_LN_BWD, FS2_PLAN_WGRAD (fs2_conv_wgrad) or
 * FS2_PLAN_WGRAD_K1_MULTI (jobs / n_jobs as in fs2_conv_wgrad_k1_multi: only db != 0, c_in and
 * c_out of each row are read; NULL for the other ops).  facts: FS2_PLAN_* bits for what the
 * dispatch reads off the pointers -- VEC (8-wide epilogue legal: c_out, ldy, ld_aux multiples
 * of 8; y, bias, aux, y2 16-B aligned), HAS_Y, HAS_LENS, HAS_DB, DW16 (dw 16-B aligned), WS16
 * (ws given and 16-B aligned).  cu_count: the device's compute units (256 on MI355X).
 * Writes "<kernel> grid=G group=g kz=k reduce=<kernel or -> reduce_grid=R" to out (cap bytes):
 * the kernel in the profiler's demangled form without "void fs2::" and the argument list,
 * e.g. conv_gemm_tapreg<128, 64, 2, 2, 4, 9, 2, 3>; grid in workgroups (split factor
 * included); kz = the split count (channel-block splits of the halo kernel, row splits of the
 * weight gradients; 0 or 1 = none). */
enum { FS2_PLAN_GEMM = 0, FS2_PLAN_GEMM_LN = 1, FS2_PLAN_GEMM_LN_BWD = 2, FS2_PLAN_WGRAD = 3,
       FS2_PLAN_WGRAD_K1_MULTI = 4 };
enum { FS2_PLAN_VEC = 1, FS2_PLAN_HAS_Y = 2, FS2_PLAN_HAS_LENS = 4, FS2_PLAN_HAS_DB = 8,
       FS2_PLAN_DW16 = 16, FS2_PLAN_WS16 = 32 };
int fs2_debug_conv_plan(int op, int64_t rows, int64_t seq_len, int64_t c_in, int64_t c_out,
                        int taps, int pad, int dilation, int flags, int facts,
                        const int64_t* jobs, int n_jobs, int cu_count, char* out, int cap);

/* ---------------------------------------------------------------- one FFT block per call
 * transformer/Layers.py:21-30 (FFTBlock.forward: MultiHeadAttention SubLayers.py:29-57, then
 * PositionwiseFeedForward SubLayers.py:85-93, post-LN, padded rows masked) and its backward,
 * bf16, issued from C: the same entry points in the same order as the per-kernel host path
 * (model.FFTBlock.fwd / bwd), so the results are bitwise those.  `blk` is a host int64 table of
 * FS2_FB_WORDS words (pointers as integers): geometry, the bf16 compute-layout weights
 * (fs2_conv_weight_prep: QKV fused as one (3 h d_k, d) Linear), the fp32 biases / LayerNorm
 * affines, and the fp32 gradient buffers they accumulate into.                               */
enum { FS2_FB_D = 0, FS2_FB_HEADS, FS2_FB_DK, FS2_FB_DINNER, FS2_FB_TAPS, FS2_FB_PAD, FS2_FB_SITE,
       FS2_FB_WQKV_F, FS2_FB_WQKV_B, FS2_FB_BQKV, FS2_FB_WFC_F, FS2_FB_WFC_B, FS2_FB_BFC,
       FS2_FB_W1_F, FS2_FB_W1_B, FS2_FB_B1, FS2_FB_W2_F, FS2_FB_W2_B, FS2_FB_B2,
       FS2_FB_LN1_G, FS2_FB_LN1_B, FS2_FB_LN2_G, FS2_FB_LN2_B,
       FS2_FB_GQKV_W, FS2_FB_GQKV_B, FS2_FB_GFC_W, FS2_FB_GFC_B, FS2_FB_G1_W, FS2_FB_G1_B,
       FS2_FB_G2_W, FS2_FB_G2_B, FS2_FB_GLN1_G, FS2_FB_GLN1_B, FS2_FB_GLN2_G, FS2_FB_GLN2_B,
       FS2_FB_WORDS };
enum { FS2_FA_X2 = 0, FS2_FA_X2_T = 1 };
/* Forward: x (rows, d) fp32 residual stream and its bf16 copy x_t -> the activation region
 * `act` (fs2_fft_block_act_bytes; saved for the backward) whose FS2_FA_X2 / FS2_FA_X2_T
 * tensors (byte offsets: fs2_fft_block_act_offset) are the block output and its copy.
 * fuse_ln: the post-LNs in the fc / w_2 GEMM epilogues (fs2_conv_gemm_ln).  p: dropout rate
 * (0 = off), seed device int64[1].                                                          */
int64_t fs2_fft_block_act_bytes(const int64_t* blk, int64_t rows, int64_t batch, int64_t seq_len,
                                int fuse_ln);
int64_t fs2_fft_block_act_offset(const int64_t* blk, int64_t rows, int64_t batch,
                                 int64_t seq_len, int fuse_ln, int which);
int fs2_fft_block_fwd(const int64_t* blk, const float* x, const void* x_t, void* act, int64_t rows,
                      int64_t batch, int64_t seq_len, const int64_t* lens, float p,
                      const uint64_t* seed, int fuse_ln, void* stream);
/* A block inside a stack.  The fp32 residual stream between post-LN sites is not stored: the
 * w_2 site rebuilds LN1's output from the saved xhat, and with prev_blk / prev_act (the block
 * before this one and its act region, same rows / lens; x NULL) the fc site rebuilds the block
 * input from that block's LN2 the same way (fs2_conv_gemm_ln_nres: bitwise the stored value).
 * The first block of a stack passes x (prev_blk NULL).  store_x2: also write the fp32 block
 * output -- for a reader outside the stack (the encoder's last block; a single block).  Without
 * it the region has no FS2_FA_X2 tensor (fs2_fft_block_act_offset_x2 returns -1 for it) and is
 * rows * d * 4 bytes smaller; every other offset is the same either way, and the backward
 * reads neither.  fs2_fft_block_fwd / _act_bytes / _act_offset are the store_x2 = 1, prev_blk =
 * NULL forms.                                                                               */
int64_t fs2_fft_block_act_bytes_x2(const int64_t* blk, int64_t rows, int64_t batch,
                                   int64_t seq_len, int fuse_ln, int store_x2);
int64_t fs2_fft_block_act_offset_x2(const int64_t* blk, int64_t rows, int64_t batch,
                                    int64_t seq_len, int fuse_ln, int store_x2, int which);
int fs2_fft_block_fwd_nres(const int64_t* blk, const float* x, const void* x_t,
                           const int64_t* prev_blk, const void* prev_act, int prev_fuse_ln,
                           int store_x2, void* act, int64_t rows, int64_t batch, int64_t seq_len,
                           const int64_t* lens, float p, const uint64_t* seed, int fuse_ln,
                           void* stream);
/* Backward from dx2 (the output gradient) or from (carry_dy2_t, carry_dx1), the block's LN2
 * backward already done by the following block.  dx (rows, d) fp32: the input gradient, or,
 * with prev_blk (the block before this one, its act region), that block's LN2 backward runs in
 * this block's QKV data-gradient epilogue (fs2_conv_gemm_ln_bwd) and writes prev_dy2_t (bf16)
 * / prev_dx1 (fp32) -- its carry -- instead (dx is then scratch).  tmp: fs2_fft_block_tmp_bytes.
 * The weight gradients run on side_stream (NULL: stream) with side_ws
 * (>= fs2_fft_block_side_ws_bytes); act, tmp and the carry buffers are read there after the
 * call returns: keep them until that stream is joined.                                      */
int64_t fs2_fft_block_tmp_bytes(const int64_t* blk, int64_t rows, int64_t batch, int64_t seq_len);
int64_t fs2_fft_block_side_ws_bytes(const int64_t* blk, int64_t rows);
int fs2_fft_block_bwd(const int64_t* blk, void* act, const void* x_t, int fuse_ln, float p,
                      const float* dx2, const void* carry_dy2_t, float* carry_dx1,
                      const int64_t* prev_blk, void* prev_act, int prev_fuse_ln, float prev_p,
                      void* tmp, float* dx, void* prev_dy2_t, float* prev_dx1, int64_t rows,
                      int64_t batch, int64_t seq_len, const int64_t* lens, const uint64_t* seed,
                      float* side_ws, int64_t side_ws_bytes, void* stream, void* side_stream);

/* ---------------------------------------------------------------- mel head per call
 * model/fastspeech2.py:91-93 (mel_linear, then postnet(output) + output; PostNet
 * transformer/Layers.py:67-137: Conv1d(k) + BatchNorm1d (batch statistics, running update,
 * num_batches_tracked), tanh on all but the last, dropout) and its backward, bf16, issued from C
 * in the order of model.MelHeadFn / PostNet (bitwise those).  `mh` is a host int64 table of
 * FS2_MH_WORDS words: geometry, mel_linear's bf16 compute-layout weights, fp32 bias and
 * gradient buffers, then FS2_MHL_WORDS words per PostNet layer.                             */
enum { FS2_MH_NMEL = 0, FS2_MH_DIN, FS2_MH_DIM, FS2_MH_TAPS, FS2_MH_PAD, FS2_MH_LAYERS, FS2_MH_SITE,
       FS2_MH_LIN_WF, FS2_MH_LIN_WB, FS2_MH_LIN_B, FS2_MH_GLIN_W, FS2_MH_GLIN_B, FS2_MH_LAYER0 };
enum { FS2_MHL_W_F = 0, FS2_MHL_W_B, FS2_MHL_B, FS2_MHL_BN_G, FS2_MHL_BN_B, FS2_MHL_BN_RM,
       FS2_MHL_BN_RV, FS2_MHL_BN_NBT, FS2_MHL_GW, FS2_MHL_GB, FS2_MHL_GBN_G, FS2_MHL_GBN_B,
       FS2_MHL_WORDS };
enum { FS2_MH_MAX_LAYERS = 8, FS2_MH_WORDS = FS2_MH_LAYER0 + FS2_MH_MAX_LAYERS * FS2_MHL_WORDS };
enum { FS2_MHA_OUT = 0, FS2_MHA_POST = 1 };
/* Forward: x_t (rows, d_in) bf16 decoder output -> act (fs2_mel_head_act_bytes) holding the
 * mel_linear output (FS2_MHA_OUT) and postnet(out) + out (FS2_MHA_POST), fp32 (rows, n_mel),
 * byte offsets from fs2_mel_head_act_offset.  Backward from d_out and / or d_post (either may be
 * NULL, not both): dx (rows, d_in) fp32 is written; tmp: fs2_mel_head_tmp_bytes; weight
 * gradients on side_stream with side_ws (>= fs2_mel_head_side_ws_bytes), reading act / tmp /
 * x_t after the call returns: keep them until that stream is joined.                       */
int64_t fs2_mel_head_act_bytes(const int64_t* mh, int64_t rows);
int64_t fs2_mel_head_act_offset(const int64_t* mh, int64_t rows, int which);
int64_t fs2_mel_head_tmp_bytes(const int64_t* mh, int64_t rows);
int64_t fs2_mel_head_side_ws_bytes(const int64_t* mh, int64_t rows);
int fs2_mel_head_fwd(const int64_t* mh, const void* x_t, void* act, int64_t rows, int64_t seq_len,
                     float p, const uint64_t* seed, void* stream);
int fs2_mel_head_bwd(const int64_t* mh, void* act, const void* x_t, const float* d_out,
                     const float* d_post, void* tmp, float* dx, int64_t rows, int64_t seq_len,
                     float p, const uint64_t* seed, float* side_ws, int64_t side_ws_bytes,
                     void* stream, void* side_stream);

/* ---------------------------------------------------------------- variance predictor per call
 * model/modules.py:197-250 (2 x (Conv1d(k) -> ReLU -> LayerNorm -> dropout) -> Linear(., 1),
 * padded rows masked to 0) and its backward, bf16, in the order of model.VariancePredictor.fwd
 * / .bwd (bitwise those).  `vp`: host int64 table of FS2_VP_WORDS words.  Forward: x_t (rows,
 * d) bf16 -> act (fs2_variance_predictor_act_bytes) whose FS2_VPA_PRED tensor is the (rows,)
 * fp32 prediction.  Backward from dpred (rows,) fp32: the input gradient is ADDED into dx_acc
 * (rows, d) fp32; tmp / side_ws / side_stream as the mel head.                              */
enum { FS2_VP_D = 0, FS2_VP_FILTER, FS2_VP_TAPS, FS2_VP_PAD1, FS2_VP_PAD2, FS2_VP_SITE,
       FS2_VP_W1_F, FS2_VP_W1_B, FS2_VP_B1, FS2_VP_LN1_G, FS2_VP_LN1_B,
       FS2_VP_W2_F, FS2_VP_W2_B, FS2_VP_B2, FS2_VP_LN2_G, FS2_VP_LN2_B, FS2_VP_LIN_W, FS2_VP_LIN_B,
       FS2_VP_G1_W, FS2_VP_G1_B, FS2_VP_GLN1_G, FS2_VP_GLN1_B, FS2_VP_G2_W, FS2_VP_G2_B,
       FS2_VP_GLN2_G, FS2_VP_GLN2_B, FS2_VP_GLIN_W, FS2_VP_GLIN_B, FS2_VP_WORDS };
enum { FS2_VPA_PRED = 0 };
int64_t fs2_variance_predictor_act_bytes(const int64_t* vp, int64_t rows);
int64_t fs2_variance_predictor_act_offset(const int64_t* vp, int64_t rows, int which);
int64_t fs2_variance_predictor_tmp_bytes(const int64_t* vp, int64_t rows);
int64_t fs2_variance_predictor_side_ws_bytes(const int64_t* vp, int64_t rows);
int fs2_variance_predictor_fwd(const int64_t* vp, const void* x_t, void* act, int64_t rows,
                               int64_t seq_len, const int64_t* lens, float p, const uint64_t* seed,
                               void* stream);
int fs2_variance_predictor_bwd(const int64_t* vp, void* act, const void* x_t, const float* dpred,
                               void* tmp, float* dx_acc, int64_t rows, int64_t seq_len,
                               const int64_t* lens, float p, const uint64_t* seed, float* side_ws,
                               int64_t side_ws_bytes, void* stream, void* side_stream);

/* Stand-in for one gradient all-reduce of the data-parallel step, for pricing the collective
 * schedule at N ranks on one GPU (train.CollectiveModel; not on the training path):
 * `blocks` workgroups read and write back `bytes` of buf[0..n) (values unchanged), paced to
 * last duration_ns -- a ring all-reduce's CU occupancy, HBM traffic and duration without the
 * interconnect.  Replaces no reference code (the reference's only collective is
 * nn.DataParallel, train.py:67-68). */
int fs2_collective_standin(float* buf, int64_t n, int64_t bytes, int blocks, int64_t duration_ns,
                           void* stream);

/* Weight (and optionally bias) gradient, accumulated into the fp32 master-gradient layout:
 *   dw[o, c, j] += sum_r dy[r, o] * x[r + j - pad, c]
 *   db[o]       += sum_r dy[r, o]                          (db may be NULL)
 * bf16, taps 3 / 5 / 9, T % 64 == 0: 64 x 64 x taps output tiles shared by 8 waves, the rows
 * split into ~256 / tiles ranges whose fp32 slabs in `ws` are summed in split order; other
 * shapes: split-K slabs with an in-order reduction.  Bitwise reproducible for the same inputs
 * AND the same lens: with lens, 64-row bands / k-tiles made only of rows past each length
 * are skipped, which changes which split sums which rows (results then agree to fp32
 * rounding with the lens-free call on zero padding rows, not bitwise).
 * `ws_bytes` >= fs2_conv_wgrad_ws_bytes(...).
 * Replaces the weight/bias half of ConvolutionBackward / AddmmBackward.                */
int64_t fs2_conv_wgrad_ws_bytes(int64_t rows, int64_t c_in, int64_t c_out, int taps);
int fs2_conv_wgrad(int dtype, const void* dy, int64_t ldy, const void* x, int64_t ldx, float* dw,
                   float* db, int64_t rows, int64_t seq_len, int64_t c_in, int64_t c_out, int taps,
                   int pad, const int64_t* lens, float* ws, int64_t ws_bytes, void* stream);

/* Several k = 1 weight gradients over the same rows in one launch (+ one split reduce):
 * for each job j of `jobs` (HOST memory, n_jobs <= 4 rows of 8 int64:
 * {dy, ldy, x, ldx, dw, db, c_in, c_out}, pointers as integers, db may be 0)
 *   dw_j[o, c] += sum_r dy_j[r, o] * x_j[r, c],   db_j[o] += sum_r dy_j[r, o].
 * The FFT block's QKV, fc and w_2 weight gradients (SubLayers.py:39-55,88) run as one grid;
 * lens (optional): 64-row k-tiles made only of padding rows are skipped.  Fixed reduction
 * order (bitwise reproducible).  ws_bytes >= fs2_conv_wgrad_k1_multi_ws_bytes(...).           */
int64_t fs2_conv_wgrad_k1_multi_ws_bytes(const int64_t* jobs, int n_jobs, int64_t rows);
int fs2_conv_wgrad_k1_multi(int dtype, const int64_t* jobs, int n_jobs, int64_t rows,
                            int64_t seq_len, const int64_t* lens, float* ws, int64_t ws_bytes,
                            void* stream);

/* Column sums (bias / LayerNorm-affine / BatchNorm gradients):
 *   out[c] (+)= sum_r x[r, c]   in a fixed order (partials in ws, then in-order sum).   */
int64_t fs2_colsum_ws_bytes(int64_t rows, int64_t cols);
int fs2_colsum(int dtype, const void* x, int64_t ldx, int64_t rows, int64_t cols, float* out,
               int accumulate, float* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- attention
 * Fused key-padding-masked softmax attention over the packed projection buffer
 * qkv (rows, 3*heads*d_head) = [Q | K | V], head h at column block h (SubLayers.py:39-52,
 * Modules.py:14-25: scores / temperature -> masked_fill(-inf) -> softmax -> @V).
 * o (rows, heads*d_head) in the reference's (B, T, h*d_v) order; lse (batch*heads, seq_len)
 * is saved for the backward.  scale = 1/temperature.  Only d_head = 128 is supported.   */
int fs2_attn_fwd(int dtype, const void* qkv, void* o, float* lse, const int64_t* lens,
                 int64_t batch, int64_t seq_len, int heads, int d_head, float scale, void* stream);
/* d_qkv (rows, 3*heads*d_head) = gradient of the packed projections.
 * ws_bytes >= fs2_attn_bwd_ws_bytes(batch, seq_len, heads).                            */
int64_t fs2_attn_bwd_ws_bytes(int64_t batch, int64_t seq_len, int heads);
int fs2_attn_bwd(int dtype, const void* qkv, const void* o, const void* d_o, const float* lse,
                 void* d_qkv, const int64_t* lens, int64_t batch, int64_t seq_len, int heads,
                 int d_head, float scale, float* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- LayerNorm family
 * Row LayerNorm (d = 256) with the fusions of the reference's call sites:
 *   z   = dropout(y; p_in, site_in) + res          (res may be NULL)
 *   u   = LN(z) * gamma + beta                      (eps 1e-5)
 *   out = padded(row) ? 0 : dropout(u; p_out, site_out)
 * and optionally a per-row dot with a Linear(256 -> 1): dot_out[r] = padded ? 0 : out.w + b.
 *   SubLayers.py:54-55,91-93 + Layers.py:25,28   (p_in = dropout, res = residual, masked)
 *   model/modules.py:209-250                      (p_out = dropout, dot = linear_layer)
 * xhat/rstd are saved for the backward (not written for masked rows outside dot mode,
 * whose backward is zero).  out_t: optional extra copy in `dtype`.                    */
int fs2_ln_fwd(int dtype, const float* y, const float* res, const float* gamma, const float* beta,
               float* out, void* out_t, float* xhat, float* rstd, const int64_t* lens,
               int64_t seq_len, int64_t rows, int d, float p_in, float p_out,
               const uint64_t* seed, uint64_t site_in, uint64_t site_out, const float* dot_w,
               const float* dot_b,
               float* dot_out, void* stream);
/* fs2_ln_fwd with the residual as res (fp32) or as the LayerNorm that produced it (res_xhat,
 * res_gamma, res_beta; masked by the same lens and never read on masked rows): see
 * fs2_conv_gemm_ln_nres.  out may be NULL here and in fs2_ln_fwd: no fp32 store.          */
int fs2_ln_fwd_nres(int dtype, const float* y, const float* res, const float* res_xhat,
                    const float* res_gamma, const float* res_beta, const float* gamma,
                    const float* beta, float* out, void* out_t, float* xhat, float* rstd,
                    const int64_t* lens, int64_t seq_len, int64_t rows, int d, float p_in,
                    float p_out, const uint64_t* seed, uint64_t site_in, uint64_t site_out,
                    const float* dot_w, const float* dot_b, float* dot_out, void* stream);
/* Backward of fs2_ln_fwd.  Upstream gradient is dout (per element) or, in dot mode,
 * ddot (per row).  Produces dy (gradient w.r.t. y before dropout, times (relu_y > 0) when
 * relu_y != NULL), optionally adds dz into dres (dres_add 1: +=, 0: =), and accumulates dgamma, dbeta and
 * (dot mode) dw_dot/db_dot into fp32 gradients; dbias_in (nullable) += sum over rows of
 * dy — the bias gradient of the layer that produced y, fused here instead of a separate
 * column sum.  dy may be NULL when the dtype copy dy_t is requested.
 * ws >= fs2_ln_bwd_ws_bytes(rows, d).                                                 */
int64_t fs2_ln_bwd_ws_bytes(int64_t rows, int d);
int fs2_ln_bwd(int dtype, const float* dout, const float* ddot, const float* dot_w,
               const float* xhat, const float* rstd, const float* gamma, const float* beta,
               const int64_t* lens, int64_t seq_len, int64_t rows, int d, float p_in, float p_out,
               const uint64_t* seed, uint64_t site_in, uint64_t site_out, const float* relu_y,
               float* dy,
               void* dy_t, float* dres, int dres_add, float* dgamma, float* dbeta, float* dw_dot,
               float* db_dot, float* dbias_in, float* ws, int64_t ws_bytes, void* stream);
/* The parameter-gradient half of fs2_ln_bwd on its own: fs2_ln_bwd called with dgamma, dbeta,
 * dw_dot, db_dot and dbias_in all NULL leaves its per-block partial sums in ws; this sums
 * them into the given gradients (+=, fixed order) -- e.g. on another stream, off the data-
 * gradient chain.  has_ddot: fs2_ln_bwd was called with ddot (the dw_dot / db_dot partials
 * exist).  ws must hold fs2_ln_bwd's partials of the same rows.                          */
int fs2_ln_bwd_final(int64_t rows, int d, const float* ws, int has_ddot, float* dgamma,
                     float* dbeta, float* dw_dot, float* db_dot, float* dbias_in, void* stream);

/* ---------------------------------------------------------------- BatchNorm (PostNet)
 * Training-mode BatchNorm1d over all rows (padded frames included) + optional tanh +
 * dropout (transformer/Layers.py:129-137).  Stats in one pass: per 64-row block its column
 * sum and centred second moment, combined exactly (M2 = sum_b [M2_b + n_b (mean_b - mean)^2])
 * in a fixed order; running stats updated with momentum, unbiased variance.  c % 8 == 0;
 * fs2_bn_bwd also c <= 4096.  ws: fs2_bn_ws_bytes(rows, c) bytes, for either call.
 * out / dz may be NULL when the bf16 copy (out_t / dz_t) is requested.               */
int64_t fs2_bn_ws_bytes(int64_t rows, int64_t c);
int fs2_bn_fwd(int dtype, const float* z, int64_t rows, int64_t c, const float* gamma,
               const float* beta, float eps, float momentum, float* running_mean,
               float* running_var, float* mean, float* rstd, int act_tanh, float p,
               const uint64_t* seed, uint64_t site, const float* res, float* out, void* out_t,
               float* ws,
               int64_t ws_bytes, int64_t* num_batches_tracked, void* stream);
/* (num_batches_tracked: nullable device int64, incremented with the running statistics --
 *  BatchNorm1d's counter update, Layers.py:129-137, without a launch of its own.)        */
/* Eval-mode BatchNorm1d (transformer/Layers.py:129-137 under model.eval()): normalise with
 * the running statistics, no dropout, no statistics update; mean / rstd (c floats each)
 * receive running_mean and 1/sqrt(running_var + eps).                                 */
int fs2_bn_eval_fwd(int dtype, const float* z, int64_t rows, int64_t c, const float* gamma,
                    const float* beta, float eps, const float* running_mean,
                    const float* running_var, float* mean, float* rstd, int act_tanh,
                    const float* res, float* out, void* out_t, void* stream);
int fs2_bn_bwd(int dtype, const float* dout, const float* z, const float* mean, const float* rstd,
               const float* gamma, const float* beta, int64_t rows, int64_t c, int act_tanh,
               float p, const uint64_t* seed, uint64_t site, float* dz, void* dz_t,
               float* dgamma,
               float* dbeta, float* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- ResCNN speaker encoder
 * The 'rescnn' architecture of speech_embedder_net.py:19-63 (ConvNorm2D / ResBlock,
 * module.py:59-117), fp32.  Activations are channels-last with time as the OUTER spatial axis:
 * (n, w, h, c), w = time, h = mel -- the encoder's input (N, T, 80) is that layout with c = 1.
 * A torch weight (c_out, c_in, kh, kw) has kh over h and kw over w.  Square odd kernels
 * k <= 7, stride 1 or 2; output extents (w + 2 pad - k) / stride + 1.  c_out a multiple of 16;
 * c_in = 1 (direct VALU kernels) or a multiple of 16 (implicit GEMM on the f32 MFMA).
 *
 * fs2_conv2d_weight_prep: the kernel layouts of w -- w_fwd for fs2_conv2d_fwd, w_bwd for
 * fs2_conv2d_dgrad (either nullable), c_out * c_in * k * k floats each.
 * fs2_conv2d_fwd: y = act(conv(x) + bias) with, in this order, bias (nullable), the folded
 * eval-mode BatchNorm y * scale[c] + shift[c] (both or neither), + res (n, wo, ho, c_out)
 * (nullable), ReLU (relu != 0).  One launch.
 * fs2_conv2d_dgrad: dx (n, w, h, c_in) = the gradient of the input for dy (n, wo, ho, c_out),
 * + add (same shape as dx, nullable): for stride 2 a gather over the output positions of
 * matching parity.
 * fs2_conv2d_wgrad: dw (c_out, c_in, k, k) in torch's layout and db (c_out, nullable); the
 * output positions are split into slices whose partial results land in ws and are added in
 * slice order.  beta = 0 overwrites, beta = 1 adds.                                       */
int fs2_conv2d_weight_prep(const float* w, int64_t c_out, int64_t c_in, int k, float* w_fwd,
                           float* w_bwd, void* stream);
int fs2_conv2d_fwd(const float* x, int64_t n, int64_t w, int64_t h, int64_t c_in,
                   const float* w_fwd, const float* bias, int64_t c_out, int k, int stride, int pad,
                   const float* scale, const float* shift, const float* res, int relu, float* y,
                   void* stream);
int fs2_conv2d_dgrad(const float* dy, int64_t n, int64_t w, int64_t h, int64_t c_in,
                     const float* w_bwd, int64_t c_out, int k, int stride, int pad,
                     const float* add, float* dx, void* stream);
int64_t fs2_conv2d_wgrad_ws_bytes(int64_t n, int64_t w, int64_t h, int64_t c_in, int64_t c_out,
                                  int k, int stride, int pad);
int fs2_conv2d_wgrad(const float* x, const float* dy, int64_t n, int64_t w, int64_t h,
                     int64_t c_in, int64_t c_out, int k, int stride, int pad, float* dw, float* db,
                     int beta, float* ws, int64_t ws_bytes, void* stream);
/* Training-mode BatchNorm2d over (rows = n w h, c) + residual + ReLU (module.py:77-78,
 * 111-117): out = relu(BN(z) + res) (res nullable, relu a flag).  Statistics as fs2_bn_fwd:
 * per 256-row block the column sum and centred second moment, combined exactly in block
 * order; biased variance normalises, the unbiased one goes into running_var with `momentum`;
 * num_batches_tracked (nullable device int64) is incremented.  mean, rstd (c each) are kept
 * for the backward.  c in 8, 16, 32, ... 1024.  ws: fs2_bn2d_ws_bytes(rows, c), either call.
 * fs2_bn2d_bwd: g = dout * (out > 0) (rows, c) is written out -- it is also the gradient of
 * res -- then dz; dgamma, dbeta (nullable) are overwritten.
 * fs2_bn2d_fold: the eval-mode scale = gamma / sqrt(running_var + eps) and
 * shift = beta - running_mean * scale that fs2_conv2d_fwd applies.                        */
int64_t fs2_bn2d_ws_bytes(int64_t rows, int64_t c);
int fs2_bn2d_fwd(const float* z, int64_t rows, int64_t c, const float* gamma, const float* beta,
                 float eps, float momentum, float* running_mean, float* running_var,
                 int64_t* num_batches_tracked, float* mean, float* rstd, const float* res, int relu,
                 float* out, float* ws, int64_t ws_bytes, void* stream);
int fs2_bn2d_fold(const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, float eps, int64_t c, float* scale, float* shift,
                  void* stream);
int fs2_bn2d_bwd(const float* dout, const float* out, const float* z, const float* mean,
                 const float* rstd, const float* gamma, int64_t rows, int64_t c, int relu, float* g,
                 float* dz, float* dgamma, float* dbeta, float* ws, int64_t ws_bytes, void* stream);
/* AdaptiveAvgPool2d((None, 1)) + Dropout + view(N, -1) (speech_embedder_net.py:60-62):
 *   out[n, c * h_ext + h] = mean_w x[n, w, h, c] * keep,  keep = 0 or 1 / (1 - p)
 * drawn for element n * c_ext * h_ext + c * h_ext + h of `site`; the backward regenerates it. */
int fs2_pool_drop_fwd(const float* x, int64_t n, int64_t w, int64_t h, int64_t c, float p,
                      const uint64_t* seed, uint64_t site, float* out, void* stream);
int fs2_pool_drop_bwd(const float* dout, int64_t n, int64_t w, int64_t h, int64_t c, float p,
                      const uint64_t* seed, uint64_t site, float* dx, void* stream);
/* fs2_clf_head / fs2_clf_head_wgrad with the projection's input width d as an argument
 * (a multiple of 64, <= 1024; 640 for the ResCNN): wp (64, d), wpt (d, 64), dwp (64, d).   */
int fs2_clf_head_w(const float* x, int64_t ldx, int64_t n, int64_t d, const float* wp,
                   const float* wpt, const float* bp, const float* w0, const float* w0t,
                   const float* b0, const float* w1, const float* w1t, const float* b1,
                   const float* w2, const float* b2, float p_drop, const uint64_t* seed,
                   uint64_t site, float* emb, float* logit, const float* demb, const float* dlogit,
                   float* dx, int64_t lddx, void* stream);
int64_t fs2_clf_head_w_wgrad_ws_bytes(int64_t n);
int fs2_clf_head_w_wgrad(const float* x, int64_t ldx, int64_t n, int64_t d, const float* wp,
                         const float* wpt, const float* bp, const float* w0, const float* w0t,
                         const float* b0, const float* w1, const float* w1t, const float* b1,
                         const float* w2, const float* b2, float p_drop, const uint64_t* seed,
                         uint64_t site, const float* demb, const float* dlogit, float* dwp,
                         float* dbp, float* dw0, float* db0, float* dw1, float* db1, float* dw2,
                         float* db2, int beta, float* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- embeddings, adaptor
 * Encoder input: word_emb[text] + accent_emb[accent] + posenc[t] (transformer/Models.py:101-103). */
int fs2_encoder_embed_fwd(const int64_t* texts, const int64_t* accents, const float* word_emb,
                          const float* accent_emb, const float* posenc, int64_t batch,
                          int64_t seq_len, int d, float* out, void* out_t, void* stream);
/* out[i] = table[ids[i]]  (nn.Embedding lookup, e.g. speaker_emb, fastspeech2.py:81).  */
int fs2_embedding_fwd(const int64_t* ids, const float* table, int64_t n, int d, float* out,
                      void* stream);
/* mask[b, t] = t >= lens[b]  (get_mask_from_lengths, utils/tools.py:155-163), 1 byte.   */
int fs2_length_mask(const int64_t* lens, int64_t batch, int64_t max_len, uint8_t* mask,
                    void* stream);
/* dtable[ids[i]] += dout[i]  for ids[i] != padding_idx (padding_idx < 0: none); dtable
 * has n_table rows.  Fixed summation order (chunk partials in ws, no atomics).
 * ws_bytes >= fs2_embedding_bwd_ws_bytes(n, d, n_table) (also for fs2_bucket_embed_bwd). */
int64_t fs2_embedding_bwd_ws_bytes(int64_t n, int d, int64_t n_table);
int fs2_embedding_bwd(const float* dout, const int64_t* ids, int64_t n, int d, int padding_idx,
                      float* dtable, int64_t n_table, float* ws, int64_t ws_bytes, void* stream);
/* out[b, t] = x[b, t] + table[ids[b]] over all t (model/fastspeech2.py:81-84).        */
int fs2_rowvec_add_fwd(const float* x, const int64_t* ids, const float* table, int64_t batch,
                       int64_t seq_len, int d, float* out, void* out_t, void* stream);
int fs2_rowvec_add_bwd(const float* dout, const int64_t* ids, int64_t batch, int64_t seq_len,
                       int d, float* dtable, void* stream);
/* out = x + table[bucketize(values, bins)] (model/modules.py:80-100, torch.bucketize
 * right=False: #bins < v).  values_dtype: FS2_F32 or 2 = f64.  idx (int32) saved.     */
int fs2_bucket_embed_fwd(const float* x, const void* values, int values_dtype, const float* bins,
                         int n_bins, const float* table, int64_t rows, int d, float* out,
                         void* out_t, int32_t* idx, void* stream);
int fs2_bucket_embed_bwd(const float* dout, const int32_t* idx, int64_t rows, int d,
                         float* dtable, int64_t n_table, float* ws, int64_t ws_bytes, void* stream);
int fs2_bucketize(const void* values, int values_dtype, const float* bins, int n_bins,
                  int64_t n, int32_t* idx, void* stream);

/* LengthRegulator (model/modules.py:161-194, utils/tools.py:363-381).
 * fs2_lr_index: cum[b, i] = inclusive scan of max(trunc(d), 0); mel_len[b] = cum[b, Ts-1]
 * (uncropped).  dur_dtype: 0 = int64, 1 = f32.                                       */
int fs2_lr_index(const void* durations, int dur_dtype, int64_t batch, int64_t src_len,
                 int32_t* cum, int64_t* mel_len, void* stream);
/* Inference durations (model/modules.py:132-135):
 * out = clamp(round_half_even(exp(log_d) - 1) * d_control, min = 0), f32 (NaN propagates). */
int fs2_duration_round(const float* log_d, int64_t n, float d_control, float* out, void* stream);
/* src[b, t] = i with cum[i-1] <= t < cum[i], or -1 past mel_len (bit-exact index map). */
int fs2_lr_source(const int32_t* cum, int64_t batch, int64_t src_len, int64_t out_len,
                  int32_t* src, void* stream);
/* out[b, t] = x[b, src[b, t]] (+ posenc[t] for every t < out_len when posenc != NULL) */
int fs2_lr_expand_fwd(const float* x, const int32_t* cum, int64_t batch, int64_t src_len,
                      int64_t out_len, int d, const float* posenc, float* out, void* out_t,
                      void* stream);
/* dx[b, i] = sum of dout[b, t] over the frames phoneme i was copied to (segmented, in order). */
int fs2_lr_expand_bwd(const float* dout, const int32_t* cum, int64_t batch, int64_t src_len,
                      int64_t out_len, int d, float* dx, void* stream);
/* LengthRegulator + frame-level pitch / energy embeddings + decoder position encoding in one
 * pass over the (batch, out_len, d) frames (model/modules.py:128-148 with a feature at
 * "frame_level", transformer/Models.py:166-168):
 *   v    = x[b, src[b, t]], zero past mel_len[b]          -> pre  (nullable)
 *   v   += p_table[bucketize(p_values[b, t], p_bins)]      -> mid  (nullable), p_idx (nullable)
 *   v   += e_table[bucketize(e_values[b, t], e_bins)]         e_idx (nullable)
 *   v   += posenc[t] for t < pos_len                       -> out fp32 / out_t bf16 (nullable)
 * Plain fp32 adds in that order: bitwise fs2_lr_expand_fwd (no posenc) -> fs2_bucket_embed_fwd
 * -> fs2_bucket_embed_fwd -> + posenc.  A NULL table skips its embedding (that feature is
 * phoneme-level, or this call is an inference stage before its prediction exists).  The
 * embeddings are added on padded frames too: pad_1D pads the targets with 0.0 and the masked
 * predictions are 0.0, so a padded frame carries table[bucketize(0)] as in the reference.
 * values: (batch, out_len), values_dtype FS2_F32 or 2 = f64.  pre / mid are the frame-level
 * predictors' inputs in the compute dtype copy_dtype (FS2_F32 or FS2_BF16).              */
int fs2_lr_expand_embed_fwd(const float* x, const int32_t* cum, int64_t batch, int64_t src_len,
                            int64_t out_len, int d, const void* p_values, int p_values_dtype,
                            const float* p_bins, int p_n_bins, const float* p_table,
                            const void* e_values, int e_values_dtype, const float* e_bins,
                            int e_n_bins, const float* e_table, const float* posenc,
                            int64_t pos_len, int copy_dtype, void* pre, void* mid, float* out,
                            void* out_t, int32_t* p_idx, int32_t* e_idx, void* stream);

/* ---------------------------------------------------------------- losses, GMM
 * FastSpeech2Loss (model/loss.py:19-92): masked L1 (mel, postnet), masked MSE (pitch,
 * energy, log-duration vs log(d+1)) with device-side valid counts (no masked_select
 * sync).  Masks are the reference's bool tensors (1 byte, true = padding): src_pad
 * (batch, src_len), mel_pad (batch, mel_len); mel_tgt is cropped to mel_len frames.
 * losses[6] = total, mel, postnet, pitch, energy, duration.  denoms (nullable, device):
 * [mel elements, phonemes] overriding the local counts (data-parallel normalisation).
 * The backward reads the denominators the forward left in ws; g_losses[6] (device) are the
 * upstream gradients of the six outputs.                                               */
int64_t fs2_fs2loss_ws_bytes(int64_t batch, int64_t mel_len);
int fs2_fs2loss_fwd(const float* mel_out, const float* post_out, const float* mel_tgt,
                    int64_t tgt_len, const float* p_pred, const float* e_pred,
                    const float* logd_pred, const float* p_tgt, const float* e_tgt,
                    const int64_t* d_tgt, const uint8_t* src_pad, const uint8_t* mel_pad,
                    int64_t batch, int64_t src_len, int64_t mel_len, int n_mel,
                    const float* denoms, float* losses, float* ws, int64_t ws_bytes, void* stream);
int fs2_fs2loss_bwd(const float* mel_out, const float* post_out, const float* mel_tgt,
                    int64_t tgt_len, const float* p_pred, const float* e_pred,
                    const float* logd_pred, const float* p_tgt, const float* e_tgt,
                    const int64_t* d_tgt, const uint8_t* src_pad, const uint8_t* mel_pad,
                    int64_t batch, int64_t src_len, int64_t mel_len, int n_mel, const float* ws,
                    const float* g_losses, float* d_mel_out, float* d_post_out, float* d_p,
                    float* d_e, float* d_logd, void* stream);
/* The same losses with a level per variance term (model/loss.py:51-63): p_frame / e_frame
 * != 0 marks pitch / energy as "frame_level".  Such a term's predictions and targets are
 * (batch, mel_len), selected by mel_pad, and its mean runs over the valid frames: the count
 * the forward leaves in ws, or denoms[0] / n_mel when denoms is given (the phoneme count is
 * not used for it).  A phoneme-level term is (batch, src_len) under src_pad as above; with
 * both flags 0 these are fs2_fs2loss_fwd / _bwd.  Same workspace, same single launch plus
 * finaliser, no host sync.                                                               */
int fs2_fs2loss_level_fwd(const float* mel_out, const float* post_out, const float* mel_tgt,
                          int64_t tgt_len, const float* p_pred, const float* e_pred,
                          const float* logd_pred, const float* p_tgt, const float* e_tgt,
                          const int64_t* d_tgt, const uint8_t* src_pad, const uint8_t* mel_pad,
                          int64_t batch, int64_t src_len, int64_t mel_len, int n_mel,
                          int p_frame, int e_frame, const float* denoms, float* losses,
                          float* ws, int64_t ws_bytes, void* stream);
int fs2_fs2loss_level_bwd(const float* mel_out, const float* post_out, const float* mel_tgt,
                          int64_t tgt_len, const float* p_pred, const float* e_pred,
                          const float* logd_pred, const float* p_tgt, const float* e_tgt,
                          const int64_t* d_tgt, const uint8_t* src_pad, const uint8_t* mel_pad,
                          int64_t batch, int64_t src_len, int64_t mel_len, int n_mel,
                          int p_frame, int e_frame, const float* ws, const float* g_losses,
                          float* d_mel_out, float* d_post_out, float* d_p, float* d_e,
                          float* d_logd, void* stream);

/* SpeakerMetaEncoder (model/fastspeech2.py:306-341): pi = softmax(W m + b),
 * sigma = softplus(W m + b), mu = W m + b.  sigma_pre saved for the backward.          */
int fs2_gmm_head_fwd(const float* meta, int64_t batch, int in_dim, int k, int d,
                     const float* w_pi, const float* b_pi, const float* w_sigma,
                     const float* b_sigma, const float* w_mu, const float* b_mu, float* pi,
                     float* sigma, float* mu, float* sigma_pre, void* stream);
/* log p(e_b) of MixtureSameFamily(Categorical(pi), Independent(Normal(mu, sigma), 1))
 * (torch.distributions semantics incl. the probs clamp); resp (batch, k) saved;
 * mean_out (nullable) = sum_b logp_b / batch  = SpeakerMetaEncLoss (model/loss.py:102-104);
 * denom (nullable, device) replaces batch by the global batch (data parallel).       */
int fs2_gmm_logprob(const float* e, const float* pi, const float* mu, const float* sigma,
                    int64_t batch, int k, int d, float* logp, float* resp, float* mean_out,
                    const float* denom, void* stream);
/* out[3] = [sum_b min(mel_lens, mel_len) * n_mel, sum_b min(src_lens, src_len), batch]:
 * this rank's loss denominators, all-reduced into the global ones (data parallel).  */
int fs2_dp_counts(const int64_t* src_lens, const int64_t* mel_lens, int64_t batch,
                  int64_t src_len, int64_t mel_len, int n_mel, float* out, void* stream);
/* Backward of  L = sum_b g_b * logp_b  through the GMM head into fp32 weight grads (+=). */
int fs2_gmm_head_bwd(const float* meta, const float* e, const float* pi, const float* mu,
                     const float* sigma, const float* sigma_pre, const float* resp,
                     const float* g_logp, int64_t batch, int in_dim, int k, int d,
                     float* dw_pi, float* db_pi, float* dw_sigma, float* db_sigma, float* dw_mu,
                     float* db_mu, void* stream);
/* Draw one embedding per row: component ~ Categorical(pi), e = mu + sigma * N(0,1)
 * (model/fastspeech2.py:176-180 speaker_gen; Philox + Box-Muller).                    */
int fs2_gmm_sample(const float* pi, const float* mu, const float* sigma, int64_t batch, int k,
                   int d, uint64_t seed, uint64_t offset, float* out, int32_t* comp, void* stream);

/* ---------------------------------------------------------------- mid-attribute GMMs
 * model/distributions.py (off the training step).
 * Mixtures are (k, d) rows of mu / sd (Normal scale) plus k weights.
 *
 * InterpolateGMM (12-77).  fs2_gmm_w2_cost: cost[i*kb+j] = the reference's _w2sq (64-77)
 * incl. its elementwise-diagonal quirk, ||mu_a-mu_b||^2 + sum(va + vb - 2 sa^3 sb), double.
 * fs2_ot_emd: exact transport plan (replaces ot.emd, 22: the f32 weights taken as float64,
 * b rescaled to a's mass), one-thread
 * transportation simplex; status[0] = iterations or -1 at max_iter.  k <= 16.
 * fs2_gmm_interpolate (23-62): pi[n] = plan.flat[n] / sum (n = i*kb + j), component
 * n = j*ka + i: mu = (1-t) mu_a[i] + t mu_b[j], sd = ((1-t) sd_a[i] + t sd_b[j])^2.      */
int fs2_gmm_w2_cost(const float* mu_a, const float* sd_a, int ka, const float* mu_b,
                    const float* sd_b, int kb, int d, double* cost, void* stream);
int fs2_ot_emd(const float* a, const float* b, const double* cost, int ka, int kb,
               int max_iter, double* plan, int* status, void* stream);
int fs2_gmm_interpolate(const double* plan, const float* mu_a, const float* sd_a, int ka,
                        const float* mu_b, const float* sd_b, int kb, int d, double t, float* pi,
                        float* mu, float* sd, void* stream);
/* BarycenterGMM (79-192).  m mixtures of k components (one per metadata combination).
 * fs2_gmm_barycenter_positions: k^m (<= 4096) or -1.  fs2_gmm_barycenter (136-163): mean and
 * 60-step fixed-point std of every position of product(range(k), repeat=m), fp32 in the
 * reference's operation order (rate: m floats).  fs2_gmm_bary_mix (165-184): nearest
 * barycenter of each of the m*k original components, weights rate_i * pi_ij (rate: m
 * doubles) summed per barycenter in first-use order, normalised; n_used[0] = number of
 * components written to used / pi_out / mu_out / sd_out (capacity m*k).  m*k <= 64.      */
int64_t fs2_gmm_barycenter_positions(int m, int k);
int fs2_gmm_barycenter(const float* mu, const float* sd, int m, int k, int d, const float* rate,
                       int iters, float* bmean, float* bstd, void* stream);
int64_t fs2_gmm_bary_mix_ws_bytes(int m, int k);
int fs2_gmm_bary_mix(const float* pi, const float* mu, const float* sd, int m, int k, int d,
                     const double* rate, const float* bmean, const float* bstd, int* n_used,
                     int* used, float* pi_out, float* mu_out, float* sd_out, double* ws,
                     int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- optimiser
 * clip_grad_norm_ + Adam over one flat fp32 parameter buffer (train.py:202,
 * model/optimizer.py:10-51).  fs2_grad_norm writes norm_coef[0] = ||g||_2 and
 * norm_coef[1] = min(1, max_norm / (norm + 1e-6)); fs2_adam_step multiplies g by
 * norm_coef[1] on the fly (no extra pass over the gradients).                         */
int64_t fs2_grad_norm_ws_bytes(int64_t n);
int fs2_grad_norm(const float* g, int64_t n, float max_norm, float* norm_coef, float* ws,
                  int64_t ws_bytes, void* stream);
int fs2_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* norm_coef,
                  float lr, float beta1, float beta2, float eps, float bias_corr1,
                  float bias_corr2_sqrt, const float* hyper, void* stream);
/* torch.optim.Adam with coupled L2 weight decay (train_speech_embedder.py:104-113):
 * g <- norm_coef[1] g + weight_decay p (clip first), then Adam.  step (device int64[1]) is the
 * optimiser's step count, hyper (device float[3]) scratch.  gate (device float, nullable):
 * with gate[0] == 0 nothing changes, step included -- torch's "no parameter has a gradient".
 * The betas are doubles, as torch's: 1 - beta is formed in double and then rounded (1.f -
 * 0.999f is 1.3e-5 off 0.001f, which went straight into v).                            */
int fs2_adam_l2_step(float* p, const float* g, float* m, float* v, int64_t n,
                     const float* norm_coef, float lr, double beta1, double beta2, float eps,
                     float weight_decay, int64_t* step, float* hyper, const float* gate,
                     void* stream);
/* out[0] = x[0] < threshold ? 1 : 0 (a device-side condition for the gates above)      */
int fs2_gate_lt(const float* x, float threshold, float* out, void* stream);
/* Device-side ScheduledOptim.step_and_update_lr (model/optimizer.py:33-51): steps (device,
 * int64[2] = [current_step, adam t]) are incremented (current_step only when advance_lr;
 * step() without the LR update passes 0) and hyper (device, float[3]) set to
 * [lr, 1 - beta1^t, sqrt(1 - beta2^t)], lr = init_lr * min(s^-0.5, warmup^-1.5 * s) *
 * rate^#{anneal < s}; fs2_adam_step reads hyper when it is non-NULL.  anneal_steps_host is
 * a host array (<= 3 entries, copied into the launch).  Together with fs2_seed_next
 * (state = device uint64[3] {base, counter, current seed}; current = splitmix64 of the
 * incremented counter) the whole step is a fixed launch sequence: graph-capturable.     */
int fs2_sched_step(int64_t* steps, float* hyper, double init_lr, int64_t n_warmup,
                   const int64_t* anneal_steps_host, int n_anneal, double anneal_rate, double beta1,
                   double beta2, int advance_lr, void* stream);
int fs2_seed_next(uint64_t* state, void* stream);
/* Stream ordering: work queued on `waiter` after this call starts only after everything
 * queued on `signaler` so far (event record + stream wait; host-side, not a launch).  */
int fs2_stream_wait(void* waiter, void* signaler);
int fs2_fill(float* x, int64_t n, float value, void* stream);
/* y = bf16(x), round to nearest even (compute copies for the bf16 path)              */
int fs2_cast_bf16(const float* x, void* y, int64_t n, void* stream);
int fs2_add_i64(int64_t* x, int64_t n, int64_t value, void* stream); /* BN num_batches_tracked */
int fs2_scale(float* x, int64_t n, float value, void* stream);
/* x[i] = src[0] * scale / (den ? den[0] : 1)  (device scalar broadcast, no host sync) */
int fs2_fill_from(float* x, int64_t n, const float* src, float scale, const float* den,
                  void* stream);
int fs2_add(float* out, const float* a, const float* b, int64_t n, void* stream); /* out = a + b */

/* ---------------------------------------------------------------- debug: stale-read poisoning
 * Not part of the reference's surface: a harness for the bitwise-determinism tests
 * (tests/test_stale_reads.py).  fs2_debug_poison(byte), byte in [0, 255] (or the FS2_POISON
 * environment variable, read once): every workspace an entry point receives and the library's
 * reused split-K partials are filled with that byte before each use; -1 turns it off (the
 * default).  fs2_debug_alloc / fs2_debug_free have the signatures of
 * torch.cuda.memory.CUDAPluggableAllocator: no caching and no device synchronisation; a block
 * is filled with the poison byte (0xff when off) at allocation (done before the call returns)
 * and again on its stream at its free, and freed blocks are quarantined (not reused) until 6 GB of them pile up.  With both, a
 * kernel that reads memory nothing wrote this step, or memory freed before it ran, reads the
 * poison, so its results depend on the byte instead of on what ran earlier in the process.
 * With poisoning on, every fs2_stream_wait also fills the LDS of every CU with the byte on the
 * waiting stream (one 160 KiB block per CU), so a kernel reading LDS it did not write reads it.
 * fs2_debug_race(delay_us, main_stream, mode): mode 0 -- every stream other than main_stream
 * is held back delay_us after each fs2_stream_wait it receives (a one-lane sleep kernel), so
 * side-stream work trails the main stream and a buffer freed or overwritten on the main stream
 * before a side-stream reader ran is poisoned by then; mode 1 -- the main stream is held back
 * after each event a side stream waits on, so a side-stream read of a main-stream result that
 * was not waited for reads stale data.  Either way a missing ordering or lifetime guard fails
 * deterministically.  Mode 2 -- a seeded random schedule: at each wait the waiter and the
 * signaler are each held back with probability 1/2 by a random 0..delay_us (an LCG from seed),
 * so one seed replays one interleaving.  delay_us 0: off.  fs2_debug_lds_dma_oob(src, out, stream): one wave
 * LDS-DMAs 16 B per lane from src (64 x 16 B) into LDS pre-filled with 0xAB bytes, lanes 32-63
 * at an out-of-range offset, and copies the 1 KiB image to out (the padding-row contract of
 * every LDS-DMA kernel: out-of-range lanes land zeros).  fs2_debug_snap(buf, cap): the variance
 * predictor backward appends copies of its intermediates (dh2, the LN2 partials, du1, dh1, the
 * LN1 partials), in stream order, to buf; fs2_debug_snap_used() is the byte count so far
 * (cap + 1 after an overflow); buf NULL turns it off.  fs2_debug_coherence(x, n, rounds,
 * blocks, bad, stream): per round, `blocks` blocks read the n uint32 of x, one block writes
 * x[i] = tag + i, and `blocks` blocks read x again, adding to bad[block] the elements that
 * are not tag + i (bad: blocks + 1 uint32, zeroed by the caller) -- a stale line in some
 * XCD's L2 after a kernel boundary on one stream shows up as a nonzero count.             */
int fs2_debug_poison(int byte);
void* fs2_debug_alloc(int64_t size, int device, void* stream);
void fs2_debug_free(void* ptr, int64_t size, int device, void* stream);
int fs2_debug_race(int delay_us, void* main_stream, int mode, int seed);
int fs2_debug_lds_dma_oob(const float* src, void* out, void* stream);
int fs2_debug_snap(void* buf, int64_t cap);
int fs2_debug_coherence(void* x, int64_t n, int rounds, int blocks, void* bad, void* stream);
int64_t fs2_debug_snap_used(void);

/* ---------------------------------------------------------------- objective synthesis metrics
 * Not in the reference (it judges synthesis by ear, through TensorBoard samples): MFCCs of this
 * project's natural-log mels, dynamic time warping with its path, and per-pair records along
 * the path (csrc/metrics.hip).
 *
 * fs2_mfcc: coefficients 1..n_coef of the orthonormal DCT-II over the mel axis (c0 dropped).
 * logmel is (B, n_mels, F) (rows = 0, MelFrontEnd's layout) or (B * F, n_mels) (rows = 1, the
 * model's row layout); n_frames (device int64[B], nullable = F everywhere) is not read back;
 * dct is the host-built table (n_mels, n_coef), dct[m * n_coef + k - 1] =
 * sqrt(2 / n_mels) cos(pi (2 m + 1) k / (2 n_mels)) formed in fp64 and rounded once;
 * out (B, F, n_coef), rows at and past n_frames zero.  1 <= n_coef < n_mels <= 128.
 *
 * fs2_dtw: per pair p, a[p] (T1max, K) and b[p] (T2max, K) fp32 with device lengths la[p] in
 * 1..T1max, lb[p] in 1..T2max (int64; a length outside its range is clamped into it, rows at
 * and past a length are never read).  fp64: c(i, j) = sqrt(sum_k (a_ik - b_jk)^2),
 * D(0, 0) = c(0, 0), D(i, j) = c(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)) with the first
 * minimum in that order taken and a predecessor outside the matrix +inf: one add per cell.
 * cost[p] = D(la-1, lb-1); path (B, T1max + T2max - 1, 2) int32 runs from (0, 0) to
 * (la-1, lb-1), path_len[p] entries (the rest is left as it was).  One workgroup per pair sweeps
 * the anti-diagonals with the last three in LDS; the workspace holds one step byte per cell,
 * the reversed path and a feature-major copy of the pair's live rows, never the matrix
 * (fs2_dtw_ws_bytes); the path is traced in the same launch.  T1max, T2max <= 2048, K >= 1.
 *
 * fs2_path_metrics: rec (B, FS2_METRIC_FIELDS) fp64 per pair = [path_len, mcd_db =
 * (10 / ln 10) sqrt(2) cost / path_len, frames_a, frames_b, n_vv, f0_sq_cents, n_vuv,
 * len_err = (frames_a - frames_b) / frames_b].  With fa (B, T1max) and fb (B, T2max) fp32
 * contours (0 = unvoiced; both or neither): n_vv = path pairs voiced in both, f0_sq_cents =
 * sum over them of (1200 log2(fa / fb))^2, n_vuv = path pairs whose voicing differs; without
 * them the three fields are 0.  Sums in fp64 in a fixed order.                            */
#define FS2_METRIC_FIELDS 8
#define FS2_DTW_MAX_LEN 2048
#define FS2_MFCC_MAX_MELS 128
int fs2_mfcc(const float* logmel, const int64_t* n_frames, int64_t batch, int64_t n_mels,
             int64_t frames, int rows, const float* dct, int64_t n_coef, float* out, void* stream);
int64_t fs2_dtw_ws_bytes(int64_t batch, int64_t t1_max, int64_t t2_max, int64_t k);
int fs2_dtw(const float* a, const float* b, const int64_t* la, const int64_t* lb, int64_t batch,
            int64_t t1_max, int64_t t2_max, int64_t k, double* cost, int* path, int* path_len,
            void* ws, int64_t ws_bytes, void* stream);
int fs2_path_metrics(const double* cost, const int* path, const int* path_len, const int64_t* la,
                     const int64_t* lb, int64_t batch, int64_t t1_max, int64_t t2_max,
                     const float* fa, const float* fb, double* rec, void* stream);

/* ---------------------------------------------------------------- alignment without TextGrids
 * Not in the reference (its corpora come aligned by the Montreal Forced Aligner; its jdit branch,
 * model/jdit.py, is not ported): the hot path of the alignment learning framework (Badlani et
 * al. 2021) -- csrc/align.hip; DESIGN.md §7.  All tensors fp32; src_lens / mel_lens are device
 * int64[B], never read back, N = src_lens[b] clamped into 1..T_s and M = mel_lens[b] into
 * 1..T_m.  A row's result does not depend on its place in the batch; no atomics, every
 * reduction in a fixed order.  batch = 0 launches nothing.  T_s <= FS2_ALIGN_MAX_SRC, T_m <=
 * FS2_ALIGN_MAX_MEL, attention width A <= FS2_ALIGN_MAX_WIDTH with A % 8 == 0.
 *
 * fs2_align_logprob: q (B, T_m, A), k (B, T_s, A) -> logp (B, T_m, T_s); for t < M, s < N
 *   logp[t, s] = log_softmax_{s < N}(-temperature |q_t - k_s|^2) + prior(t, s),
 * prior = 0 when omega <= 0, else the log beta-binomial pmf of s with n = N - 1,
 * a = omega (t + 1), b = omega (M - t), formed with fp64 lgamma, rounded once and added to the
 * fp32 log-softmax (never stored on its own).  Cells with t >= M or s >= N are written as 0.
 *
 * fs2_align_logprob_bwd: g = dL/dlogp (B, T_m, T_s), cells with t >= M or s >= N not read ->
 * dq (B, T_m, A), dk (B, T_s, A), zero in dead rows.  The softmax is recomputed from q and k.
 * dk is summed over frames in a fixed order: partials of 256 frames, each in frame order, then
 * the partials in order.  The workspace holds dL/dscore and the partials.
 *
 * fs2_forward_sum: one workgroup per utterance.  For each frame t < M the N + 1 scores
 * [blank = -1, logp[t, 0..N-1]] are log-softmaxed and the CTC recursion runs over the 2N + 1
 * states of the target 1, 2, .., N (distinct labels: the skip transition is always open), alpha
 * and beta in fp64 in the log domain.  nll[b] = -log p(target); grad (B, T_m, T_s) =
 * d(nll[b] w[b]) / dlogp with caller-supplied weights w (B), dead cells 0.  The workspace holds
 * the label states' alpha; beta is combined with it on the fly.  M < N has no valid path:
 * nll[b] = +inf and grad = 0 for that row.
 *
 * fs2_mas: monotonic alignment search, one workgroup per utterance.  fp32, one add per cell:
 *   V[0, 0] = logp[0, 0], V[0, s > 0] = -inf, V[t, s] = logp[t, s] + max(V[t-1, s-1], V[t-1, s])
 * with the diagonal s - 1 taken on a tie (V[t-1, -1] = -inf); the path ends at (M-1, N-1) and is
 * traced back in the same launch from one step byte per cell in the workspace.  durations
 * (B, T_s) int64 = frames per phoneme, >= 1 for s < N, 0 for s >= N.  A row with M < N has no
 * such path: its durations are all 0 (callers that know the lengths reject it beforehand).
 *
 * Optional positions (fs2_forward_sum_opt, fs2_mas_opt): optional (B, T_s) uint8, read at s < N
 * only and staged once per row into LDS; a marked position may take no frame (an optional
 * silence).  A valid labelling keeps every unmarked position, may omit marked ones, never two
 * neighbours and never all.  Both are defined by the formulas below and memory-safe for any mask
 * content; callers reject rows with two adjacent marks or no unmarked position.  Workspaces,
 * limits and argument checks are those of fs2_forward_sum / fs2_mas, plus optional != NULL; with
 * an all-zero mask the results are theirs bit for bit (the extra terms are summed last, and an
 * exp of -inf adds an exact 0).
 *
 * fs2_forward_sum_opt: the states are the pairs bl[s] (the blank before label s, s = 0..N) and
 * la[s]; omitting a marked label u omits the pair (la[u], bl[u+1]), so a labelling keeps exactly
 * one state path.  Beside the edges of fs2_forward_sum: into la[s] when optional[s-1] from
 * bl[s-1] and, for s >= 2, from la[s-2]; when optional[0] and N >= 2, la[1] is an initial state
 * too; when optional[N-1] and N >= 2, la[N-2] and bl[N-1] are final states too; beta the mirror
 * image.  grad[t, s] = w[b] (softmax_t(s) - occupancy_t(la[s])).  Whether a path exists is found
 * after the alpha pass: ll = -inf gives nll[b] = +inf and a gradient that is exactly 0.
 *
 * fs2_mas_opt: V[0, 0] = logp[0, 0]; V[0, 1] = logp[0, 1] when optional[0] and N >= 2; the rest
 * of row 0 is -inf.  Among V[t-1, s-1] and V[t-1, s] the diagonal wins a tie; V[t-1, s-2] is a
 * candidate only when optional[s-1] and s >= 2, and is taken only when strictly greater than
 * that winner.  The path ends at (M-1, N-1), or at (M-1, N-2) when optional[N-1], N >= 2 and
 * V[M-1, N-2] is strictly greater.  Step byte per cell: 0 stay, 1 diagonal, 2 skip; the
 * trace-back does s -= step.  durations >= 1 for kept positions, 0 for omitted ones, their sum M;
 * a row without a path (its end cell is -inf) gets all zeros.   */
#define FS2_ALIGN_MAX_SRC 1024
#define FS2_ALIGN_MAX_MEL 2048
#define FS2_ALIGN_MAX_WIDTH 128
int fs2_align_logprob(const float* q, const float* k, const int64_t* src_lens,
                      const int64_t* mel_lens, int64_t batch, int64_t t_m, int64_t t_s, int64_t a,
                      float temperature, float omega, float* logp, void* stream);
int64_t fs2_align_logprob_bwd_ws_bytes(int64_t batch, int64_t t_m, int64_t t_s, int64_t a);
int fs2_align_logprob_bwd(const float* q, const float* k, const float* g, const int64_t* src_lens,
                          const int64_t* mel_lens, int64_t batch, int64_t t_m, int64_t t_s,
                          int64_t a, float temperature, float* dq, float* dk, void* ws,
                          int64_t ws_bytes, void* stream);
int64_t fs2_forward_sum_ws_bytes(int64_t batch, int64_t t_m, int64_t t_s);
int fs2_forward_sum(const float* logp, const int64_t* src_lens, const int64_t* mel_lens,
                    const float* w, int64_t batch, int64_t t_m, int64_t t_s, float* nll,
                    float* grad, void* ws, int64_t ws_bytes, void* stream);
int64_t fs2_mas_ws_bytes(int64_t batch, int64_t t_m, int64_t t_s);
int fs2_mas(const float* logp, const int64_t* src_lens, const int64_t* mel_lens, int64_t batch,
            int64_t t_m, int64_t t_s, int64_t* durations, void* ws, int64_t ws_bytes,
            void* stream);
int fs2_forward_sum_opt(const float* logp, const int64_t* src_lens, const int64_t* mel_lens,
                        const unsigned char* optional, const float* w, int64_t batch, int64_t t_m,
                        int64_t t_s, float* nll, float* grad, void* ws, int64_t ws_bytes,
                        void* stream);
int fs2_mas_opt(const float* logp, const int64_t* src_lens, const int64_t* mel_lens,
                const unsigned char* optional, int64_t batch, int64_t t_m, int64_t t_s,
                int64_t* durations, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- phoneme error rate
 * Not in the reference (it judges synthesis by ear): a general CTC loss, the greedy CTC decoder
 * and a batched edit distance -- csrc/ctc.hip; DESIGN.md §7.  One workgroup per utterance or
 * pair; lengths are device int64[B], never read back; no atomics, every reduction in a fixed
 * order: a row's result has the same bits wherever it sits in a batch and from run to run.
 * batch = 0 launches nothing and returns 0; every argument is checked before any launch.
 * T <= FS2_CTC_MAX_T, L_max <= FS2_CTC_MAX_TARGET, C <= FS2_CTC_MAX_CLASSES, C <= ld <= 65535,
 * R_max, H_max <= FS2_EDIT_MAX_LEN, B <= 65535.
 *
 * fs2_ctc_loss: logits (B, T, ld) fp32 with C <= ld classes (columns C..ld-1 are never read),
 * blank in [0, C), targets (B, L_max) int64, M = frame_lens[b] clamped into 1..T, L =
 * target_lens[b] clamped into 0..L_max (L = 0: the all-blank path), w (B) fp32.  For each frame
 * t < M the C logits are log-softmaxed (max in fp32, the sum of exp and the log in fp64) and the
 * CTC recursion runs over the 2L + 1 states z of the blank-interleaved target (z_2k = blank,
 * z_2k+1 = target[k]), alpha and beta in fp64 in the log domain:
 *   alpha_0(j) = y_0(z_j) for j < 2, else -inf;
 *   alpha_t(j) = y_t(z_j) + lse(alpha_t-1(j), alpha_t-1(j-1), [skip] alpha_t-1(j-2)),
 * the skip open for odd j >= 3 with target[k] != target[k-1] (k = (j-1)/2), beta the mirror
 * image from beta_M-1(j) = y_M-1(z_j) for j >= 2L - 1; ll = lse(alpha_M-1(2L), alpha_M-1(2L-1)).
 * nll[b] = -ll (fp32).  grad (B, T, ld) fp32 = d(w[b] nll[b]) / dlogits
 *   = w[b] (softmax[t, c] - gamma_t(c)),  gamma_t(c) = sum over states j with z_j = c of
 *     exp(alpha_t(j) + beta_t(j) - y_t(z_j) - ll),
 * summed in ascending state order in fp64 (the blank column: its L + 1 states in order), a state
 * whose alpha or beta is -inf at t (a -inf logit masks its class there) counting 0;
 * exactly 0 for t >= M and in columns C..ld-1.  A row without a valid path -- M < L + the number
 * of adjacent repeats, a label outside [0, C), a label equal to blank, or scores that give
 * ll = -inf -- has nll = +inf and grad = 0; nothing out of range is read for it and the other
 * rows stand.  The workspace (fs2_ctc_loss_ws_bytes = B T (2 L_max + 1) 8) holds every state's
 * alpha, replaced by its occupancy in the beta sweep.
 *
 * fs2_ctc_greedy: the same logits, C, ld, blank and frame_lens.  Per frame t < M the arg-max of
 * the raw fp32 logits over the C classes: a NaN never wins, ties go to the lowest class, a frame
 * of nothing but NaN is blank.  Repeats are collapsed, blanks dropped and the labels compacted
 * in order by a block scan: ids (B, T) int64, 0 at and past lens[b]; lens (B) int64; argmax
 * (B, T) int32 (nullable), blank at t >= M.
 *
 * fs2_edit_distance: ref (B, R_max), hyp (B, H_max) int64, lengths clamped into 0..max (0 is
 * legal on either side or both).  One Levenshtein table with unit costs, D(i, 0) = i,
 * D(0, j) = j, D(i, j) = min(D(i-1, j-1) + [ref_i != hyp_j], D(i-1, j) + 1, D(i, j-1) + 1), the
 * first minimum taken in that order: the diagonal (a match or a substitution), then a deletion
 * (a reference symbol without a partner), then an insertion.  The path is traced back from
 * (R, H) in the same launch: out (B, 4) int64 = [distance, substitutions, deletions,
 * insertions], distance = S + D + I.  Anti-diagonals with the last two in LDS; the workspace
 * holds one step byte per cell (fs2_edit_distance_ws_bytes = B (R_max + H_max + 1) (R_max + 1)).
 * All integers: exact.                                                                        */
#define FS2_CTC_MAX_T 2048
#define FS2_CTC_MAX_TARGET 1024
#define FS2_CTC_MAX_CLASSES 1024
#define FS2_EDIT_MAX_LEN 2048
int64_t fs2_ctc_loss_ws_bytes(int64_t batch, int64_t t, int64_t l_max);
int fs2_ctc_loss(const float* logits, const int64_t* targets, const int64_t* frame_lens,
                 const int64_t* target_lens, const float* w, int64_t batch, int64_t t,
                 int64_t n_classes, int64_t ld, int64_t blank, int64_t l_max, float* nll,
                 float* grad, void* ws, int64_t ws_bytes, void* stream);
int fs2_ctc_greedy(const float* logits, const int64_t* frame_lens, int64_t batch, int64_t t,
                   int64_t n_classes, int64_t ld, int64_t blank, int64_t* ids, int64_t* lens,
                   int* argmax, void* stream);
int64_t fs2_edit_distance_ws_bytes(int64_t batch, int64_t r_max, int64_t h_max);
int fs2_edit_distance(const int64_t* ref, const int64_t* ref_lens, const int64_t* hyp,
                      const int64_t* hyp_lens, int64_t batch, int64_t r_max, int64_t h_max,
                      int64_t* out, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- generated-speaker metrics
 * Not in the reference: set-to-set statistics in speaker-encoder space for speakers that have
 * no recording to be scored against (csrc/speaker_eval.hip).  No atomics, every
 * reduction in a fixed order, results independent of the grid; a size of 0 launches nothing.
 *
 * fs2_cosine_nn: for every row of a (Na, D) the k nearest rows of b (Nb, D) by cosine distance,
 * fp32 inputs of any length, 1 <= D <= FS2_NN_MAX_DIM, 1 <= k <= FS2_NN_MAX_K; the Na x Nb
 * matrix is never stored.  Per pair three fp64 sums dot, |a|^2, |b|^2, each over d = 0 .. D-1 in
 * that order (a product of two fp32 values is exact in fp64);
 *   den = sqrt(|a|^2) * sqrt(|b|^2), c = den > 0 ? dot / den : 0, dist = (float)(1.0 - c).
 * Candidates rank by that fp32 dist, ties to the lower index of b; a NaN distance is never a
 * candidate.  dist (Na, k) fp32 ascending, index (Na, k) int64; slots without a candidate hold
 * +inf and -1.  group_a (Na) / group_b (Nb): device int64, both or neither; mode 0 skips
 * candidate j when group_a[i] == group_b[j], mode 1 keeps only those.  A block owns 16 rows of
 * a in LDS and sweeps b; past 1024 rows b is cut into ranges of 1024, one block column each,
 * whose lists are merged in range order (fs2_cosine_nn_ws_bytes holds them) -- the same list,
 * bit for bit, as one sweep gives.  Nb = 0 writes the empty lists.
 *
 * fs2_finite_summary: x (n) fp32, n <= FS2_SUMMARY_MAX_N -> out[5] fp64 = [count of finite
 * entries, their median as numpy.median has it (the mean of the two middle values for an even
 * count), their mean summed in fp64 in index order, min, max]; count = 0 gives NaN for the
 * other four.  The selection is exact: a binary search over the bits of an order-preserving
 * 32-bit key, one counting pass per bit (ws: fs2_finite_summary_ws_bytes, the keys).
 *
 * fs2_gauss_moments: x (n, D) fp32, n >= 2, D <= FS2_FRECHET_MAX_DIM -> mean (D) and the
 * unbiased covariance cov (D, D), fp64, two passes: the mean (rows in order), then the centred
 * products (rows in order) / (n - 1).
 *
 * fs2_frechet: per pair p of Gaussians, from fp64 moments mean_a / mean_b (P, D) and cov_a /
 * cov_b (P, D, D), D <= FS2_FRECHET_MAX_DIM, one workgroup with the matrices in LDS:
 * Sigma_a = V L V^T by cyclic Jacobi (fp64, round-robin pair order, at most 30 sweeps, ended in
 * the kernel by the first sweep without a rotation), S = V max(L, 0)^(1/2) V^T, mu = the
 * eigenvalues of sym(S Sigma_b S) by the same solver;
 *   out[p] = [|dmu|^2 + tr Sigma_a + tr Sigma_b - 2 sum sqrt(max(mu, 0)), |dmu|^2,
 *             tr Sigma_a + tr Sigma_b, sum sqrt(max(mu, 0))].                                */
#define FS2_NN_MAX_DIM 256
#define FS2_NN_MAX_K 16
#define FS2_SUMMARY_MAX_N 1048576
#define FS2_FRECHET_MAX_DIM 64
int64_t fs2_cosine_nn_ws_bytes(int64_t na, int64_t nb, int64_t k);
int fs2_cosine_nn(const float* a, const float* b, int64_t na, int64_t nb, int64_t dim, int64_t k,
                  const int64_t* group_a, const int64_t* group_b, int mode, float* dist,
                  int64_t* index, void* ws, int64_t ws_bytes, void* stream);
int64_t fs2_finite_summary_ws_bytes(int64_t n);
int fs2_finite_summary(const float* x, int64_t n, double* out, void* ws, int64_t ws_bytes,
                       void* stream);
int fs2_gauss_moments(const float* x, int64_t n, int64_t dim, double* mean, double* cov,
                      void* stream);
int fs2_frechet(const double* mean_a, const double* cov_a, const double* mean_b,
                const double* cov_b, int64_t pairs, int64_t dim, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FS2HIP_H */
