// Around the speaker encoder's training step (train_speech_embedder.py, data_load.py): batches
// cut on the device from a device-resident corpus, the d-vector reduction, the EER scoring of
// test() and the per-batch statistics of the epoch loop.  fp32 throughout; every reduction runs
// in a fixed order (no atomics), so all results are bitwise repeatable.
#include <math.h>

#include "common.hpp"

namespace fs2 {

// ---------------------------------------------------------------- crop + transpose gather
// out[r, t, c] = store[row_off[r] + c * row_stride[r] + row_start[r] + t].  A block moves one
// (n_mels, MG_T frames) tile of one row through LDS: the reads run along frames (one wave reads
// 64 consecutive frames of one mel channel, 256 B), the writes along the contiguous
// (frames, n_mels) tile of the output.  The LDS row stride MG_T + 1 = 65 is 1 mod 32, so the
// ds_write_b32 (lanes along t) and the ds_read_b32 (lanes along c) both touch 32 different banks
// per 32-lane group.  Source addresses are formed in 64 bits.
constexpr int MG_T = 64, MG_TP = MG_T + 1, MG_CMAX = 128, MG_LMAX = 256;

__global__ __launch_bounds__(256) void mel_crop_gather_kernel(
    const float* __restrict__ store, const int64_t* __restrict__ row_off,
    const int32_t* __restrict__ row_stride, const int32_t* __restrict__ row_start, int n_mels,
    int len, float* __restrict__ out) {
  __shared__ float tile[MG_CMAX * MG_TP];
  const int64_t r = blockIdx.x;
  const int t0 = blockIdx.y * MG_T;
  const int tt = min(MG_T, len - t0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t stride = row_stride[r];
  const float* src = store + row_off[r] + (int64_t)row_start[r] + t0;
  if (lane < tt)
    for (int c = wave; c < n_mels; c += 4) tile[c * MG_TP + lane] = src[c * stride + lane];
  __syncthreads();
  float* dst = out + (r * len + t0) * n_mels;
  const int n = tt * n_mels;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int t = i / n_mels, c = i - t * n_mels;
    dst[i] = tile[c * MG_TP + t];
  }
}

// ---------------------------------------------------------------- segment mean, unit length
// out[s] = m / ||m||, m = mean of rows seg_start[s] .. seg_start[s + 1] - 1 of x (rows, dim).
// One block per segment; thread d adds its column in row order; the norm is one wave's sum of
// squares (lanes take d = lane, lane + 64, ... in order, then the fixed wave reduction).
constexpr int RM_DMAX = 1024;

__global__ __launch_bounds__(256) void rows_mean_unit_kernel(const float* __restrict__ x,
                                                             const int64_t* __restrict__ seg_start,
                                                             int dim, float* __restrict__ out) {
  __shared__ float mean[RM_DMAX];
  __shared__ float inv;
  const int64_t s = blockIdx.x, r0 = seg_start[s], r1 = seg_start[s + 1];
  const float cnt = (float)(r1 - r0);
  for (int d = threadIdx.x; d < dim; d += 256) {
    float a = 0.f;
    for (int64_t r = r0; r < r1; ++r) a += x[r * dim + d];
    mean[d] = a / cnt;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    float q = 0.f;
    for (int d = threadIdx.x; d < dim; d += 64) q = fmaf(mean[d], mean[d], q);
    q = wave_sum(q);
    if (threadIdx.x == 0) inv = sqrtf(q);
  }
  __syncthreads();
  const float nrm = inv;
  for (int d = threadIdx.x; d < dim; d += 256) out[s * dim + d] = mean[d] / nrm;
}

// ---------------------------------------------------------------- EER scoring of one batch
// One block, 16 waves (the shape of ge2e_softmax_kernel).  Phases, block barriers between:
//   A  enrolment centroids (means over m_enr) and their norms, verification sums per speaker;
//   B  one wave per verification row: cos against every enrolment centroid, for k = j against
//      the row's exclude-self verification centroid; + 1e-6; written to sim;
//   C  one wave per threshold: the number of accepted entries and of accepted same-speaker
//      entries as integers, FAR and FRR from them by fp32 divisions in the reference's order;
//   D  thread 0 keeps the first threshold with the strictly smallest |FAR - FRR| below 1.
constexpr int EER_WAVES = 16, EER_DMAX = 256, EER_DS = EER_DMAX / 64, EER_THR = 50;

struct Eer {
  const float* enroll;
  const float* verify;
  int N, Me, Mv, D;
  float* sim;
  float* table;
  float* result;
  float* ws;
  float thr[EER_THR];
};

FS2_DEV float eer_clamp(float n) { return fmaxf(n, 1e-8f); }  // F.cosine_similarity's eps

FS2_DEV int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64 * EER_WAVES) void ge2e_eer_kernel(Eer a) {
  __shared__ float far_s[EER_THR], frr_s[EER_THR];
  const int N = a.N, Me = a.Me, Mv = a.Mv, D = a.D, NM = N * Mv;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* cmean = a.ws;          // (N, D)
  float* vsum = cmean + N * D;  // (N, D)
  float* cnrm = vsum + N * D;   // (N)
  const float inv_m1 = 1.f / (float)(Mv - 1);

  for (int idx = tid; idx < N * D; idx += blockDim.x) {
    const int k = idx / D, d = idx % D;
    float s = 0.f, v = 0.f;
    for (int i = 0; i < Me; ++i) s += a.enroll[((int64_t)k * Me + i) * D + d];
    for (int i = 0; i < Mv; ++i) v += a.verify[((int64_t)k * Mv + i) * D + d];
    cmean[idx] = s / (float)Me;
    vsum[idx] = v;
  }
  __threadfence_block();
  __syncthreads();
  for (int k = tid; k < N; k += blockDim.x) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(cmean[k * D + d], cmean[k * D + d], s);
    cnrm[k] = sqrtf(s);
  }
  __threadfence_block();
  __syncthreads();

  for (int row = wave; row < NM; row += EER_WAVES) {
    const int j = row / Mv;
    float ev[EER_DS], cx[EER_DS];
    float na2 = 0.f, nx2 = 0.f;
#pragma unroll
    for (int s = 0; s < EER_DS; ++s) {
      const int d = lane + 64 * s;
      ev[s] = d < D ? a.verify[(int64_t)row * D + d] : 0.f;
      cx[s] = d < D ? (vsum[j * D + d] - ev[s]) * inv_m1 : 0.f;
      na2 = fmaf(ev[s], ev[s], na2);
      nx2 = fmaf(cx[s], cx[s], nx2);
    }
    const float na = eer_clamp(sqrtf(wave_sum(na2))), nx = eer_clamp(sqrtf(wave_sum(nx2)));
    for (int k = 0; k < N; ++k) {
      const bool own = k == j;
      float dot = 0.f;
#pragma unroll
      for (int s = 0; s < EER_DS; ++s) {
        const int d = lane + 64 * s;
        const float bv = own ? cx[s] : d < D ? cmean[k * D + d] : 0.f;
        dot = fmaf(ev[s], bv, dot);
      }
      dot = wave_sum(dot);
      const float nb = own ? nx : eer_clamp(cnrm[k]);
      if (lane == 0) a.sim[(int64_t)row * N + k] = dot / (na * nb) + 1e-6f;
    }
  }
  __threadfence_block();
  __syncthreads();

  const int total = NM * N;
  for (int i = wave; i < EER_THR; i += EER_WAVES) {
    const float thr = a.thr[i];
    int acc = 0, same = 0;
    for (int e = lane; e < total; e += 64) {
      const int row = e / N, k = e - row * N;
      const bool on = a.sim[e] > thr;
      acc += on ? 1 : 0;
      same += on && k == row / Mv ? 1 : 0;
    }
    acc = wave_sum_int(acc);
    same = wave_sum_int(same);
    if (lane == 0) {
      const float far = (float)(acc - same) / (float)(N - 1) / (float)Mv / (float)N;
      const float frr = (float)(NM - same) / (float)Mv / (float)N;
      far_s[i] = far;
      frr_s[i] = frr;
      a.table[2 * i] = far;
      a.table[2 * i + 1] = frr;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float diff = 1.f, eer = 0.f, thr = 0.f, far = 0.f, frr = 0.f;
    for (int i = 0; i < EER_THR; ++i) {
      const float d = fabsf(far_s[i] - frr_s[i]);
      if (diff > d) diff = d, eer = (far_s[i] + frr_s[i]) / 2.f, thr = a.thr[i], far = far_s[i], frr = frr_s[i];
    }
    a.result[0] = eer;
    a.result[1] = thr;
    a.result[2] = far;
    a.result[3] = frr;
  }
}

// ---------------------------------------------------------------- per-batch statistics
// totals += [loss, da_loss, 100 * correct / n, 1], correct = #{round(sigmoid(logit)) == y}
// (utils.py:238-247; torch.round is half-to-even, so a sigmoid of exactly 0.5 is class 0).
__global__ __launch_bounds__(64) void epoch_stats_kernel(float* totals, const float* loss,
                                                         const float* da_loss, const float* logit,
                                                         const float* y, int n, float* correct) {
  const int lane = threadIdx.x;
  int ok = 0;
  if (logit)
    for (int i = lane; i < n; i += 64) {
      const float p = 1.f / (1.f + expf(-logit[i]));
      ok += rintf(p) == y[i] ? 1 : 0;
    }
  ok = wave_sum_int(ok);
  if (lane != 0) return;
  if (loss) totals[0] += loss[0];
  if (da_loss) totals[1] += da_loss[0];
  if (logit) totals[2] += (float)ok / (float)n * 100.f;
  totals[3] += 1.f;
  if (correct) correct[0] = (float)ok;
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_mel_crop_gather(const float* store, const int64_t* row_off, const int32_t* row_stride,
                        const int32_t* row_start, int64_t n_rows, int64_t n_mels, int64_t len,
                        float* out, void* stream) {
  FS2_CHECK_ARG(len >= 1 && len <= MG_LMAX, "fs2_mel_crop_gather: len %lld (1..%d)",
                (long long)len, MG_LMAX);
  FS2_CHECK_ARG(n_mels >= 1 && n_mels <= MG_CMAX, "fs2_mel_crop_gather: n_mels %lld (1..%d)",
                (long long)n_mels, MG_CMAX);
  FS2_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31), "fs2_mel_crop_gather: n_rows %lld",
                (long long)n_rows);
  if (n_rows == 0) return FS2_OK;
  FS2_CHECK_ARG(store && row_off && row_stride && row_start && out,
                "fs2_mel_crop_gather: missing operand");
  const dim3 grid((unsigned)n_rows, (unsigned)((len + MG_T - 1) / MG_T));
  mel_crop_gather_kernel<<<grid, 256, 0, as_stream(stream)>>>(store, row_off, row_stride, row_start,
                                                             (int)n_mels, (int)len, out);
  return launch_status("fs2_mel_crop_gather");
}

int fs2_rows_mean_unit(const float* x, const int64_t* seg_start, int64_t n_seg, int64_t dim,
                       float* out, void* stream) {
  FS2_CHECK_ARG(dim >= 1 && dim <= RM_DMAX, "fs2_rows_mean_unit: dim %lld (1..%d)", (long long)dim,
                RM_DMAX);
  FS2_CHECK_ARG(n_seg >= 0 && n_seg < (1ll << 31), "fs2_rows_mean_unit: n_seg %lld",
                (long long)n_seg);
  if (n_seg == 0) return FS2_OK;
  FS2_CHECK_ARG(x && seg_start && out, "fs2_rows_mean_unit: missing operand");
  rows_mean_unit_kernel<<<(unsigned)n_seg, 256, 0, as_stream(stream)>>>(x, seg_start, (int)dim, out);
  return launch_status("fs2_rows_mean_unit");
}

int64_t fs2_ge2e_eer_ws_bytes(int64_t n_spk, int64_t dim) {
  if (n_spk < 1 || dim < 1) return 0;
  return (2 * n_spk * dim + n_spk) * 4;
}

int fs2_ge2e_eer(const float* enroll, const float* verify, int64_t n_spk, int64_t m_enr,
                 int64_t m_ver, int64_t dim, float* sim, float* table, float* result, float* ws,
                 int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(n_spk >= 2 && m_enr >= 1 && m_ver >= 2 && dim >= 1 && dim <= EER_DMAX,
                "fs2_ge2e_eer: n_spk %lld (>= 2), m_enr %lld (>= 1), m_ver %lld (>= 2), dim %lld "
                "(1..%d)", (long long)n_spk, (long long)m_enr, (long long)m_ver, (long long)dim,
                EER_DMAX);
  FS2_CHECK_ARG(n_spk < (1 << 12) && m_enr < (1 << 12) && m_ver < (1 << 12) &&
                    n_spk * m_ver * n_spk < (1ll << 24) && n_spk * (m_enr + m_ver) * dim < (1ll << 28),
                "fs2_ge2e_eer: batch too large (n_spk %lld, m_enr %lld, m_ver %lld)",
                (long long)n_spk, (long long)m_enr, (long long)m_ver);
  FS2_CHECK_ARG(ws_bytes >= fs2_ge2e_eer_ws_bytes(n_spk, dim), "fs2_ge2e_eer: workspace too small");
  FS2_CHECK_ARG(enroll && verify && sim && table && result && ws, "fs2_ge2e_eer: missing operand");
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  Eer a{enroll, verify, (int)n_spk, (int)m_enr, (int)m_ver, (int)dim, sim, table, result, ws, {}};
  for (int i = 0; i < EER_THR; ++i) {
    volatile double t = 0.01 * (double)i;  // two roundings, as the host expression 0.01 * i + 0.5
    a.thr[i] = (float)(t + 0.5);
  }
  ge2e_eer_kernel<<<1, 64 * EER_WAVES, 0, st>>>(a);
  return launch_status("fs2_ge2e_eer");
}

int fs2_epoch_stats_add(float* totals, const float* loss, const float* da_loss, const float* logit,
                        const float* y, int64_t n, float* correct, void* stream) {
  FS2_CHECK_ARG(totals, "fs2_epoch_stats_add: missing totals");
  FS2_CHECK_ARG(!logit || (y && n >= 1 && n < (1ll << 24)),
                "fs2_epoch_stats_add: logits need labels and 1 <= n < 2^24 (n %lld)", (long long)n);
  FS2_CHECK_ARG(!correct || logit, "fs2_epoch_stats_add: a count needs logits");
  epoch_stats_kernel<<<1, 64, 0, as_stream(stream)>>>(totals, loss, da_loss, logit, y, (int)n,
                                                     correct);
  return launch_status("fs2_epoch_stats_add");
}

}  // extern "C"
