// The FastSpeech2 corpus resident on the device (dataset.py:112-172, utils/tools.py:18-125,
// evaluate.py:52-75): one launch pads B utterances of the flat per-field stores into the
// training batch, and one tiny launch keeps the validation sums of a pass on the device.
#include "common.hpp"

namespace fs2 {

// ---------------------------------------------------------------- padded batch gather
// grid (chunks + 1, B), 256 threads.  Block (c < chunks, b) copies float4s
// [c * BG_CHUNK, (c + 1) * BG_CHUNK) of utterance b's padded mel row: the utterance's
// mel_len * n_mels floats are contiguous in the store and in the batch, what follows them up to
// Tm * n_mels is zero.  A thread issues its BG_PER 16-byte loads before its stores.  Block
// (chunks, b) writes utterance b's small fields: text, duration, accent (int64), pitch (fp32),
// energy (4- or 8-byte words, moved as bits), each zero past the utterance's length, the
// metadata row and the three scalars.  Every output element is written exactly once, by plain
// vector stores; nothing is read outside an utterance's own extent in a store.
constexpr int BG_THREADS = 256, BG_PER = 4, BG_CHUNK = BG_THREADS * BG_PER;

struct BatchGather {
  const int32_t* idx;
  const int32_t* src_len;
  const int32_t* mel_len;
  const int64_t* src_off;
  const int64_t* mel_off;
  const int64_t* speaker;
  const int64_t* text;
  const int64_t* dur;
  const int64_t* accent;
  const float* mel;
  const float* pitch;
  const void* energy;
  const float* meta;
  int n_mels, meta_dim, energy_bytes, pitch_frame, energy_frame, Ts, Tm, chunks;
  int64_t* o_text;
  int64_t* o_dur;
  int64_t* o_accent;
  float* o_mel;
  float* o_pitch;
  void* o_energy;
  int64_t* o_src_len;
  int64_t* o_mel_len;
  int64_t* o_speaker;
  float* o_meta;
};

template <typename T>
FS2_DEV void pad_row(const T* __restrict__ src, int n, T* __restrict__ dst, int width) {
  for (int t = threadIdx.x; t < width; t += BG_THREADS) dst[t] = t < n ? src[t] : T(0);
}

__global__ __launch_bounds__(BG_THREADS) void batch_gather_kernel(BatchGather a) {
  const int b = blockIdx.y;
  const int u = a.idx[b];
  const int M = a.mel_len[u];
  if ((int)blockIdx.x < a.chunks) {
    const int64_t valid4 = (int64_t)M * a.n_mels / 4, total4 = (int64_t)a.Tm * a.n_mels / 4;
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(a.mel + a.mel_off[u]);
    f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(a.o_mel + (int64_t)b * a.Tm * a.n_mels);
    const int64_t i0 = (int64_t)blockIdx.x * BG_CHUNK + threadIdx.x;
    f32x4 v[BG_PER];
#pragma unroll
    for (int k = 0; k < BG_PER; ++k) {
      const int64_t i = i0 + k * BG_THREADS;
      v[k] = i < valid4 ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < BG_PER; ++k) {
      const int64_t i = i0 + k * BG_THREADS;
      if (i < total4) dst[i] = v[k];
    }
    return;
  }
  const int L = a.src_len[u], Ts = a.Ts, Tm = a.Tm;
  const int64_t so = a.src_off[u], fo = a.mel_off[u] / a.n_mels;  // phoneme / frame offsets
  pad_row(a.text + so, L, a.o_text + (int64_t)b * Ts, Ts);
  pad_row(a.dur + so, L, a.o_dur + (int64_t)b * Ts, Ts);
  if (a.o_accent) pad_row(a.accent + so, L, a.o_accent + (int64_t)b * Ts, Ts);
  {
    const int n = a.pitch_frame ? M : L, w = a.pitch_frame ? Tm : Ts;
    pad_row(a.pitch + (a.pitch_frame ? fo : so), n, a.o_pitch + (int64_t)b * w, w);
  }
  {
    const int n = a.energy_frame ? M : L, w = a.energy_frame ? Tm : Ts;
    const int64_t off = a.energy_frame ? fo : so;
    if (a.energy_bytes == 8)
      pad_row(static_cast<const uint64_t*>(a.energy) + off, n,
              static_cast<uint64_t*>(a.o_energy) + (int64_t)b * w, w);
    else
      pad_row(static_cast<const uint32_t*>(a.energy) + off, n,
              static_cast<uint32_t*>(a.o_energy) + (int64_t)b * w, w);
  }
  for (int j = threadIdx.x; j < a.meta_dim; j += BG_THREADS)
    a.o_meta[(int64_t)b * a.meta_dim + j] = a.meta[(int64_t)u * a.meta_dim + j];
  if (threadIdx.x == 0) {
    a.o_src_len[b] = L;
    a.o_mel_len[b] = M;
    a.o_speaker[b] = a.speaker[u];
  }
}

// ---------------------------------------------------------------- validation sums
// evaluate.py:68-72 for one batch: sums[i] += float(losses[i]) * batch in fp64 (the product of an
// fp32 value and a batch size is exact there), esum += eloss * batch in fp32 (the product is
// rounded before the sum, as the reference's tensor expression rounds it).
__global__ __launch_bounds__(64) void eval_accum_kernel(double* sums, float* esum,
                                                        const float* losses, const float* eloss,
                                                        int batch) {
  const int i = threadIdx.x;
  if (i < 6) sums[i] = __dadd_rn(sums[i], __dmul_rn((double)losses[i], (double)batch));
  if (i == 6 && eloss) esum[0] = __fadd_rn(esum[0], __fmul_rn(eloss[0], (float)batch));
}

}  // namespace fs2

using namespace fs2;

extern "C" {

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
                     int64_t* o_speaker, float* o_meta, void* stream) {
  FS2_CHECK_ARG(batch >= 1 && batch <= 65535, "fs2_batch_gather: batch %lld (1..65535)",
                (long long)batch);
  FS2_CHECK_ARG(n_utt >= 1 && n_utt < (1ll << 31), "fs2_batch_gather: n_utt %lld",
                (long long)n_utt);
  FS2_CHECK_ARG(n_mels >= 4 && n_mels % 4 == 0 && n_mels <= 1024,
                "fs2_batch_gather: n_mels %lld (a multiple of 4, 4..1024)", (long long)n_mels);
  FS2_CHECK_ARG(meta_dim >= 1 && meta_dim <= 65536, "fs2_batch_gather: meta_dim %lld",
                (long long)meta_dim);
  FS2_CHECK_ARG(energy_bytes == 4 || energy_bytes == 8,
                "fs2_batch_gather: energy_bytes %lld (4 or 8)", (long long)energy_bytes);
  FS2_CHECK_ARG(max_src_len >= 1 && max_src_len < (1ll << 24) && max_mel_len >= 1 &&
                    max_mel_len * n_mels < (1ll << 31),
                "fs2_batch_gather: max_src_len %lld, max_mel_len %lld out of range",
                (long long)max_src_len, (long long)max_mel_len);
  FS2_CHECK_ARG(idx && idx_host && src_len_host && mel_len_host && src_len && mel_len && src_off &&
                    mel_off && speaker && text && dur && mel && pitch && energy && meta,
                "fs2_batch_gather: missing input");
  FS2_CHECK_ARG(o_text && o_dur && o_mel && o_pitch && o_energy && o_src_len && o_mel_len &&
                    o_speaker && o_meta,
                "fs2_batch_gather: missing output");
  FS2_CHECK_ARG(!o_accent || accent, "fs2_batch_gather: accents asked for, none stored");
  FS2_CHECK_ARG(((uintptr_t)mel | (uintptr_t)o_mel) % 16 == 0,
                "fs2_batch_gather: the mel store and output must be 16-byte aligned");
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t u = idx_host[b];
    FS2_CHECK_ARG(u >= 0 && u < n_utt, "fs2_batch_gather: index %lld of row %lld outside 0..%lld",
                  (long long)u, (long long)b, (long long)n_utt - 1);
    FS2_CHECK_ARG(src_len_host[u] >= 0 && src_len_host[u] <= max_src_len,
                  "fs2_batch_gather: utterance %lld has %d phonemes, max_src_len is %lld",
                  (long long)u, (int)src_len_host[u], (long long)max_src_len);
    FS2_CHECK_ARG(mel_len_host[u] >= 0 && mel_len_host[u] <= max_mel_len,
                  "fs2_batch_gather: utterance %lld has %d frames, max_mel_len is %lld",
                  (long long)u, (int)mel_len_host[u], (long long)max_mel_len);
  }
  BatchGather a;
  a.idx = idx, a.src_len = src_len, a.mel_len = mel_len, a.src_off = src_off, a.mel_off = mel_off;
  a.speaker = speaker, a.text = text, a.dur = dur, a.accent = accent, a.mel = mel;
  a.pitch = pitch, a.energy = energy, a.meta = meta;
  a.n_mels = (int)n_mels, a.meta_dim = (int)meta_dim, a.energy_bytes = (int)energy_bytes;
  a.pitch_frame = pitch_frame != 0, a.energy_frame = energy_frame != 0;
  a.Ts = (int)max_src_len, a.Tm = (int)max_mel_len;
  a.chunks = (int)((max_mel_len * n_mels / 4 + BG_CHUNK - 1) / BG_CHUNK);
  a.o_text = o_text, a.o_dur = o_dur, a.o_accent = o_accent, a.o_mel = o_mel, a.o_pitch = o_pitch;
  a.o_energy = o_energy, a.o_src_len = o_src_len, a.o_mel_len = o_mel_len;
  a.o_speaker = o_speaker, a.o_meta = o_meta;
  const dim3 grid((unsigned)a.chunks + 1, (unsigned)batch);
  batch_gather_kernel<<<grid, BG_THREADS, 0, as_stream(stream)>>>(a);
  return launch_status("fs2_batch_gather");
}

int fs2_eval_accum(double* sums, float* esum, const float* losses, const float* eloss,
                   int64_t batch, void* stream) {
  FS2_CHECK_ARG(sums && esum && losses, "fs2_eval_accum: missing operand");
  FS2_CHECK_ARG(batch >= 1 && batch < (1ll << 24), "fs2_eval_accum: batch %lld", (long long)batch);
  eval_accum_kernel<<<1, 64, 0, as_stream(stream)>>>(sums, esum, losses, eloss, (int)batch);
  return launch_status("fs2_eval_accum");
}

}  // extern "C"
