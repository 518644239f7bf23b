// bf16 Conv1d / Linear dispatch (host code only): check the arguments, ask conv_plan.hpp which
// kernel the shape runs, fill the kernel arguments, hand the plan to its family's launcher.  No
// choice is made here or in the launchers.
#include "conv_nt.hpp"
#include "conv_plan.hpp"

namespace fs2 {

int no_instance(const char* family) {
  set_error("%s: no kernel instance is built for the planned parameters", family);
  return FS2_ERR_LAUNCH;
}

static int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      n = v;
    else
      n = 256;
  }
  return n;
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int launch_conv(const ConvPlan& p, GldsArgs& a, hipStream_t st) {
  a.tiles_m = p.tiles_m;
  a.tiles_n = p.tiles_n;
  a.group = p.group;
  switch (p.kernel) {
    case CONV_TAPREG: return launch_conv_tapreg(p, a, st);
    case CONV_HALO: return launch_conv_halo(p, a, st);
    default: return launch_conv_nt(p, a, st);
  }
}

int conv_gemm_bf16_launch(const void* x, int64_t ldx, const void* wk, void* y, int64_t ldy,
                          int64_t rows, int64_t seq_len, int64_t c_in, int64_t c_out, int taps,
                          int pad, const int64_t* lens, const float* bias, int flags,
                          const void* aux, int64_t ld_aux, const VocEpi& ve, hipStream_t st) {
  FS2_CHECK_ARG(c_in % 8 == 0 && ldx % 8 == 0 && al16(x) && al16(wk),
                "fs2_conv_gemm(bf16): c_in/ldx must be multiples of 8 and operands 16-B aligned");
  const bool uses_aux = flags & (FS2_EPI_ADD_AUX | FS2_EPI_RELU_MASK_AUX);
  const bool vec = c_out % 8 == 0 && ldy % 8 == 0 && al16(y) &&
                   (!(flags & FS2_EPI_BIAS) || al16(bias)) &&
                   (!uses_aux || (ld_aux % 8 == 0 && al16(aux))) &&
                   (!(flags & FS2_EPI_Y2) || al16(ve.y2));
  const ConvShape s{rows, seq_len, c_in, c_out, taps, pad, ve.dil, flags, lens != nullptr,
                    y != nullptr, vec};
  const ConvPlan p = plan_conv_gemm(s, g_tune, cu_count());
  GldsArgs a{(const u16*)x, ldx, (const u16*)wk, y, ldy, rows, seq_len, (int)c_in, (int)c_out,
             taps, pad, (int)(taps * c_in), bias, flags, aux, ld_aux, 0, 0, vec, 1, lens,
             ve.dil, ve.alpha, ve.scale, (u16*)ve.y2, ve.alpha2};
  if (int rc = launch_conv(p, a, st)) return rc;
  return launch_status("fs2_conv_gemm(bf16)");
}

// fs2_conv_gemm_ln: the tap-major kernel on whole 256-wide rows with the LayerNorm epilogue
int conv_gemm_ln_glds_launch(const void* x, int64_t ldx, const void* wk, int64_t rows,
                             int64_t seq_len, int64_t c_in, int taps, int pad, const int64_t* lens,
                             const float* bias, const float* res, const float* res_xhat,
                             const float* res_gamma, const float* res_beta, const float* gamma,
                             const float* beta, float* out, void* out_t, float* xhat, float* rstd,
                             float p_in, const uint64_t* seed, uint64_t site_in, hipStream_t st) {
  FS2_CHECK_ARG(c_in % 8 == 0 && ldx % 8 == 0 && al16(x) && al16(wk),
                "fs2_conv_gemm_ln: c_in/ldx must be multiples of 8 and operands 16-B aligned");
  FS2_CHECK_ARG(al16(out) && al16(xhat) && al16(gamma) && al16(beta) && al16(res) && al16(bias) &&
                    al16(out_t) && al16(res_xhat) && al16(res_gamma) && al16(res_beta),
                "fs2_conv_gemm_ln: LayerNorm tensors must be 16-B aligned");
  GldsArgs a{(const u16*)x, ldx, (const u16*)wk, nullptr, 256, rows, seq_len, (int)c_in, 256,
             taps, pad, (int)(taps * c_in), bias, bias ? FS2_EPI_BIAS : 0, nullptr, 0, 0, 0, 1, 1,
             lens, 1, 0.f, 1.f, nullptr, 0.f};
  a.ln_res = res;
  a.ln_res_xhat = res_xhat;
  a.ln_res_gamma = res_gamma;
  a.ln_res_beta = res_beta;
  a.ln_gamma = gamma;
  a.ln_beta = beta;
  a.ln_out = out;
  a.ln_out_t = (u16*)out_t;
  a.ln_xhat = xhat;
  a.ln_rstd = rstd;
  a.ln_seed = p_in > 0.f ? seed : nullptr;
  a.ln_site = site_in;
  a.ln_p = p_in;
  const ConvShape s{rows, seq_len, c_in, 256, taps, pad, 1, a.flags, lens != nullptr, false, true};
  if (int rc = launch_conv(plan_conv_gemm_ln(s, g_tune, false), a, st)) return rc;
  return launch_status("fs2_conv_gemm_ln");
}

// fs2_conv_gemm_ln_bwd: 64 x 256 tiles with the LayerNorm-backward epilogue (ws = fs2_ln_bwd's
// partial layout; the caller runs fs2_ln_bwd_final)
int conv_gemm_lnbwd_glds_launch(const void* x, int64_t ldx, const void* wk, int64_t rows,
                                int64_t seq_len, int64_t c_in, int taps, int pad,
                                const int64_t* lens, const float* aux, const float* xhat,
                                const float* rstd, const float* gamma, float p_in,
                                const uint64_t* seed, uint64_t site_in, float* dres, int dres_add,
                                void* dy_t, float* ws, hipStream_t st) {
  FS2_CHECK_ARG(c_in % 8 == 0 && ldx % 8 == 0 && al16(x) && al16(wk),
                "fs2_conv_gemm_ln_bwd: c_in/ldx must be multiples of 8 and operands 16-B aligned");
  FS2_CHECK_ARG(al16(aux) && al16(xhat) && al16(gamma) && al16(dres) && al16(dy_t) && al16(ws),
                "fs2_conv_gemm_ln_bwd: LayerNorm tensors must be 16-B aligned");
  GldsArgs a{(const u16*)x, ldx, (const u16*)wk, nullptr, 256, rows, seq_len, (int)c_in, 256,
             taps, pad, (int)(taps * c_in), nullptr, aux ? FS2_EPI_ADD_AUX : 0, aux, 256, 0, 0, 1,
             1, lens, 1, 0.f, 1.f, nullptr, 0.f};
  a.ln_gamma = gamma;
  a.ln_out = dres;
  a.ln_out_t = (u16*)dy_t;
  a.ln_xhat = const_cast<float*>(xhat);
  a.ln_rstd = const_cast<float*>(rstd);
  a.ln_seed = p_in > 0.f ? seed : nullptr;
  a.ln_site = site_in;
  a.ln_p = p_in;
  a.ln_mode = 1;
  a.ln_dres_add = dres_add;
  a.ln_part = ws;
  a.ln_nblk = (rows + 31) / 32;
  const ConvShape s{rows, seq_len, c_in, 256, taps, pad, 1, a.flags, lens != nullptr, false, true};
  if (int rc = launch_conv(plan_conv_gemm_ln(s, g_tune, true), a, st)) return rc;
  return launch_status("fs2_conv_gemm_ln_bwd");
}

int wgrad_k1_multi_bf16_launch(const int64_t* jobs, int n, int64_t rows, int64_t seq_len,
                               const int64_t* lens, float* ws, hipStream_t st) {
  const WgradPlan p = plan_wgrad_k1_multi(jobs, n, rows, g_tune);
  if (int rc = launch_wgrad_k1_multi(p, jobs, n, rows, seq_len, lens, ws, st)) return rc;
  return launch_status("fs2_conv_wgrad_k1_multi");
}

int conv_wgrad_bf16_launch(const WgradCall& c, hipStream_t st) {
  const WgradShape s{c.rows, c.seq_len, c.c_in, c.c_out, c.taps, c.pad, c.lens != nullptr,
                     c.db != nullptr, al16(c.dw), c.ws != nullptr && al16(c.ws)};
  const bool ops8 = c.c_in % 8 == 0 && c.c_out % 8 == 0 && c.ldx % 8 == 0 && c.ldy % 8 == 0 &&
                    al16(c.dy) && al16(c.x);
  if (c.taps == 1 && g_tune[FS2_TUNE_WGRAD_K1] == 0) {
    const int64_t job[8] = {(int64_t)c.dy, c.ldy, (int64_t)c.x, c.ldx, (int64_t)c.dw, (int64_t)c.db,
                            c.c_in, c.c_out};
    FS2_CHECK_ARG(ops8 && al16(c.dw),
                  "fs2_conv_wgrad(bf16, k = 1): channel counts / strides must be multiples of 8, "
                  "operands and dw 16-B aligned");
    // the kernel reads lens[row / seq_len] to skip all-padding k-tiles
    FS2_CHECK_ARG(c.lens == nullptr || (c.seq_len > 0 && c.rows % c.seq_len == 0),
                  "fs2_conv_wgrad(bf16, k = 1): with lens, rows must be batch x seq_len");
    return wgrad_k1_multi_bf16_launch(job, 1, c.rows, c.seq_len, c.lens, c.ws, st);
  }
  FS2_CHECK_ARG(ops8,
                "fs2_conv_wgrad(bf16): channel counts / strides must be multiples of 8, operands 16-B aligned");
  const WgradPlan p = plan_conv_wgrad(s, g_tune);
  if (p.kernel == WGRAD_WIDE) {
    const int rc = launch_wgrad_wide(p, c, st);
    return rc ? rc : launch_status("fs2_conv_wgrad(bf16, wide)");
  }
  if (p.kernel == WGRAD_BAND) {
    const int rc = launch_wgrad_band(p, c, st);
    return rc ? rc : launch_status("fs2_conv_wgrad(bf16, band)");
  }
  const int rc = launch_wgrad_splitk(p, c, st);
  return rc ? rc : launch_status("fs2_conv_wgrad(bf16)");
}

}  // namespace fs2

using namespace fs2;

extern "C" int fs2_debug_conv_plan(int op, int64_t rows, int64_t seq_len, int64_t c_in,
                                   int64_t c_out, int taps, int pad, int dilation, int flags,
                                   int facts, const int64_t* jobs, int n_jobs, int cu_count,
                                   char* out, int cap) {
  FS2_CHECK_ARG(out && cap > 0, "fs2_debug_conv_plan: no output buffer");
  FS2_CHECK_ARG(op >= FS2_PLAN_GEMM && op <= FS2_PLAN_WGRAD_K1_MULTI, "fs2_debug_conv_plan: unknown op %d", op);
  FS2_CHECK_ARG(rows > 0 && taps >= 1 && dilation >= 1 && cu_count > 0 &&
                    (op == FS2_PLAN_WGRAD_K1_MULTI || (seq_len > 0 && c_in > 0 && c_out > 0)),
                "fs2_debug_conv_plan: rows, seq_len, c_in, c_out, taps, dilation, cu_count must be positive");
  const bool lens = facts & FS2_PLAN_HAS_LENS;
  if (op == FS2_PLAN_WGRAD_K1_MULTI) {
    FS2_CHECK_ARG(jobs && n_jobs >= 1 && n_jobs <= 4, "fs2_debug_conv_plan: 1..4 jobs");
    for (int j = 0; j < n_jobs; ++j)
      FS2_CHECK_ARG(jobs[8 * j + 6] > 0 && jobs[8 * j + 7] > 0, "fs2_debug_conv_plan: job %d: channel counts must be positive", j);
    wgrad_plan_describe(plan_wgrad_k1_multi(jobs, n_jobs, rows, g_tune), out, cap);
  } else if (op == FS2_PLAN_WGRAD) {
    const WgradShape s{rows, seq_len, c_in, c_out, taps, pad, lens, (facts & FS2_PLAN_HAS_DB) != 0,
                       (facts & FS2_PLAN_DW16) != 0, (facts & FS2_PLAN_WS16) != 0};
    wgrad_plan_describe(plan_conv_wgrad(s, g_tune), out, cap);
  } else {
    const ConvShape s{rows, seq_len, c_in, c_out, taps, pad, dilation, flags, lens,
                      (facts & FS2_PLAN_HAS_Y) != 0, (facts & FS2_PLAN_VEC) != 0};
    const ConvPlan p = op == FS2_PLAN_GEMM ? plan_conv_gemm(s, g_tune, cu_count)
                                           : plan_conv_gemm_ln(s, g_tune, op == FS2_PLAN_GEMM_LN_BWD);
    conv_plan_describe(p, out, cap);
  }
  return FS2_OK;
}
