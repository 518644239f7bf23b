// The speaker encoder's corpus from waveforms (Multilingual-Speaker-Encoder-with-Domain-
// Adaptation/data_preprocess.py:39-67) around fs2_melspec: the voice-activity split
// (librosa.effects.split, line 46), the gather of the kept intervals into rows for the mel
// front end (line 56) and the half-overlapping tisv windows of each interval's mel (lines
// 63-66).  include/fs2hip.h has the definitions.  fp32 sums in a fixed order, no atomics: every
// result is bitwise repeatable and depends on its own row only.
//
// fs2_nonsilent_split is two launches.
//   1  frame powers.  A block owns `fpb` consecutive frames of one row (the host picks fpb <= 8
//      so that their sample span, (fpb - 1) hop + frame_length floats, fits 48 KiB of LDS; one
//      frame always fits).  The span is read once -- the padding resolved against the row's own
//      length, nothing past len is touched, 16 bytes per lane wherever four samples of the row
//      lie on a 16-byte boundary -- and its SQUARES are staged, so a sample shared by
//      frame_length / hop frames (4 at librosa's defaults) is loaded and squared once per block
//      instead of once per frame.  One wave then sums one frame: lane l adds the squares
//      l, l + 64, ... in ascending order (consecutive lanes, consecutive LDS words: no bank
//      conflict), then the fixed wave butterfly, then one division by frame_length.  The order
//      depends on the frame alone, not on fpb, the block or the batch.
//   2  one block per row: the row's maximum (any order gives the same maximum), the decision
//      per frame in fp64 in the power domain, and the ordered compaction of the run edges by a
//      ballot / popcount scan, 256 frames per step with the counts carried from step to step.
// Both are streaming passes over at most a few thousand frames per row; neither is near any
// limit of the machine, the launch latency is what they cost.
#include <math.h>

#include "common.hpp"
#include "fft.hpp"  // reflect_index only: no float arithmetic crosses the pragma below

#pragma clang fp contract(off)

namespace fs2 {

constexpr int VAD_THREADS = 256, VAD_WAVES = VAD_THREADS / 64;
constexpr int VAD_MAX_FPB = 8, VAD_MAX_FRAME = 4096;
constexpr int VAD_SPAN_CAP = 12288;  // floats of LDS a block's squares may take (48 KiB)

struct Vad {
  const float* wav;
  const int64_t* lens;
  int64_t S, F_max;
  int frame, hop, fpb, tiles, pad_zero, wav_al16;
  float* power;
};

FS2_DEV int64_t vad_len(const int64_t* lens, int64_t b, int64_t S) {
  const int64_t n = lens ? lens[b] : S;
  return n < 0 ? 0 : n > S ? S : n;
}

__global__ __launch_bounds__(VAD_THREADS) void frame_power_kernel(Vad a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t b = blockIdx.x / a.tiles;
  const int64_t f0 = (int64_t)(blockIdx.x - b * a.tiles) * a.fpb;
  const int len = (int)vad_len(a.lens, b, a.S);
  const int64_t n_f = len > 0 ? 1 + len / a.hop : 0;
  float* out = a.power + b * a.F_max;
  const int live = (int)(n_f - f0 < a.fpb ? n_f - f0 : a.fpb);  // block-uniform
  const int p0 = (int)f0 * a.hop - a.frame / 2;
  // Span element i is sample p0 + i of the row, at global element b S + p0 + i.  `head` of them
  // come before the first 16-byte boundary of the source; the squares sit `pre` floats into the
  // LDS so that the same boundary is a 16-byte boundary there: from it on a lane moves four
  // samples with one global_load_dwordx4 and one ds_write_b128 wherever all four are samples of
  // the row, and one by one through the padding rule elsewhere.
  const int head = a.wav_al16 ? (int)((4 - ((b * a.S + p0) & 3)) & 3) : 0;
  const int pre = (4 - head) & 3;
  float* sq = lds + pre;
  if (live > 0) {
    const float* row = a.wav + b * a.S;
    const int span_n = (live - 1) * a.hop + a.frame;
    auto one = [&](int i) {
      const int p = p0 + i;
      const float v = a.pad_zero ? (p >= 0 && p < len ? row[p] : 0.f) : row[reflect_index(p, len)];
      sq[i] = v * v;
    };
    const int quads = a.wav_al16 && span_n > head ? (span_n - head) / 4 : 0;
    for (int g = tid; g < quads; g += VAD_THREADS) {
      const int i = head + 4 * g, p = p0 + i;
      if (p >= 0 && p + 3 < len) {
        const f32x4 v = ld4(row + p);
        st4(sq + i, f32x4{v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w});
      } else {
        one(i), one(i + 1), one(i + 2), one(i + 3);
      }
    }
    // what the quads leave: the head and the tail, at most 3 + 3 samples (everything without
    // an aligned source)
    const int rest = span_n - 4 * quads;
    for (int k = tid; k < rest; k += VAD_THREADS) one(k < head ? k : 4 * quads + k);
  }
  __syncthreads();
  for (int j = wave; j < a.fpb; j += VAD_WAVES) {
    const int64_t f = f0 + j;
    if (f >= a.F_max) break;
    float acc = 0.f;
    if (j < live) {
      const float* s = sq + j * a.hop;
      for (int i = lane; i < a.frame; i += 64) acc = acc + s[i];
      acc = wave_sum(acc) / (float)a.frame;
    }
    if (lane == 0) out[f] = acc;  // zeros at f >= n_f
  }
}

struct VadRuns {
  const float* power;
  const int64_t* lens;
  int64_t S, F_max, max_iv;
  int hop;
  double floor_p, factor;  // 1e-10 and 10^(-top_db / 10)
  int64_t* intervals;
  int32_t* n_intervals;
};

FS2_DEV int block_offsets(bool flag, int* wave_tot, int& total) {
  // exclusive count of `flag` over the threads before this one; total over the block
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned long long m = __ballot(flag);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();  // wave_tot may still be read from the previous call
  if (lane == 0) wave_tot[wave] = __popcll(m);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < VAD_WAVES; ++w) {
    base += w < wave ? wave_tot[w] : 0;
    total += wave_tot[w];
  }
  return base + before;
}

__global__ __launch_bounds__(VAD_THREADS) void nonsilent_runs_kernel(VadRuns a) {
  __shared__ float wmax[VAD_WAVES];
  __shared__ int tot_a[VAD_WAVES], tot_b[VAD_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t b = blockIdx.x;
  const int64_t len = vad_len(a.lens, b, a.S);
  const int64_t n_f = len > 0 ? 1 + len / a.hop : 0;
  const float* p = a.power + b * a.F_max;
  int64_t* iv = a.intervals + b * a.max_iv * 2;

  float m = 0.f;  // powers are >= 0
  for (int64_t f = tid; f < n_f; f += VAD_THREADS) m = fmaxf(m, p[f]);
  m = wave_max(m);
  if (lane == 0) wmax[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const double thr = fmax(a.floor_p, (double)m) * a.factor;

  // frame n_f stands for the silence after the row: it closes a run that reaches the end
  int64_t starts = 0, ends = 0;
  for (int64_t f0 = 0; f0 <= n_f && n_f > 0; f0 += VAD_THREADS) {
    const int64_t f = f0 + tid;
    const bool in = f <= n_f;
    const bool cur = in && f < n_f && fmax(a.floor_p, (double)p[f]) > thr;
    const bool prev = in && f > 0 && fmax(a.floor_p, (double)p[f - 1]) > thr;
    const bool is_start = cur && !prev, is_end = prev && !cur;
    int n_s, n_e;
    const int64_t si = starts + block_offsets(is_start, tot_a, n_s);
    const int64_t ei = ends + block_offsets(is_end, tot_b, n_e);
    const int64_t edge = f * a.hop < len ? f * a.hop : len;
    if (is_start && si < a.max_iv) iv[2 * si] = edge;
    if (is_end && ei < a.max_iv) iv[2 * ei + 1] = edge;
    starts += n_s;
    ends += n_e;
  }
  for (int64_t i = starts + tid; i < a.max_iv; i += VAD_THREADS) iv[2 * i] = iv[2 * i + 1] = 0;
  if (tid == 0) a.n_intervals[b] = (int32_t)starts;
}

// ---------------------------------------------------------------- interval gather
// out[s, i] = wav[seg_row[s], seg_first[s] + i], i < seg_len[s], zeros after.  A thread moves
// four consecutive samples: one 16-byte store where the output row allows it, one 16-byte load
// where the segment's first sample is 4-aligned in the source as well (block-uniform), four
// dword loads otherwise -- a wave's lanes still cover 1 KiB of consecutive source bytes.
constexpr int WS_PER = 4, WS_TILE = VAD_THREADS * WS_PER;

struct Segs {
  const float* wav;
  int64_t batch, S;
  const int32_t* seg_row;
  const int64_t* seg_first;
  const int64_t* seg_len;
  float* out;
  int64_t out_samples;
  int tiles, wav_al16, out_al16;
};

__global__ __launch_bounds__(VAD_THREADS) void wave_segments_kernel(Segs a) {
  const int64_t s = blockIdx.x / a.tiles;
  const int64_t i0 = (int64_t)(blockIdx.x - s * a.tiles) * WS_TILE + threadIdx.x * WS_PER;
  if (i0 >= a.out_samples) return;
  // the descriptors are the caller's promise; they are read clamped so that nothing outside
  // wav is touched if it is broken
  int64_t r = a.seg_row[s], first = a.seg_first[s], n = a.seg_len[s];
  r = r < 0 ? 0 : r >= a.batch ? a.batch - 1 : r;
  first = first < 0 ? 0 : first > a.S ? a.S : first;
  n = n < 0 ? 0 : n > a.S - first ? a.S - first : n;
  n = n > a.out_samples ? a.out_samples : n;
  const int64_t src0 = r * a.S + first;
  const float* src = a.wav + src0 + i0;
  float* dst = a.out + s * a.out_samples + i0;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i0 + WS_PER <= n) {
    if (a.wav_al16 && (src0 & 3) == 0) {
      v = ld4(src);
    } else {
      v.x = src[0], v.y = src[1], v.z = src[2], v.w = src[3];
    }
  } else if (i0 < n) {
    v.x = src[0];
    if (i0 + 1 < n) v.y = src[1];
    if (i0 + 2 < n) v.z = src[2];
  }
  if (a.out_al16 && i0 + WS_PER <= a.out_samples) {
    st4(dst, v);
  } else {
    dst[0] = v.x;
    if (i0 + 1 < a.out_samples) dst[1] = v.y;
    if (i0 + 2 < a.out_samples) dst[2] = v.z;
    if (i0 + 3 < a.out_samples) dst[3] = v.w;
  }
}

// ---------------------------------------------------------------- tisv windows
// One block per output window w: its row r is the one with win_off[r] <= w < win_off[r + 1]
// (binary search, rows + 1 offsets), j = w - win_off[r], first frame floor(tisv j / 2).  The
// copy runs along frames: tisv consecutive floats of one mel channel in, the same out.
constexpr int TW_TMAX = 256, TW_CMAX = 128;

__global__ __launch_bounds__(VAD_THREADS) void tisv_windows_kernel(
    const float* __restrict__ mel, const int64_t* __restrict__ n_frames, int64_t rows, int n_mels,
    int64_t F_max, int tisv, const int64_t* __restrict__ win_off, float* __restrict__ out) {
  const int64_t w = blockIdx.x;
  int64_t lo = 0, hi = rows - 1;  // the last r with win_off[r] <= w
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (win_off[mid] <= w) lo = mid; else hi = mid - 1;
  }
  const int64_t r = lo, j = w - win_off[r];
  int64_t F = n_frames[r];
  F = F < 0 ? 0 : F > F_max ? F_max : F;
  // a window the offsets promise but the row does not have (broken offsets) is written as zeros
  const bool ok = j >= 0 && w < win_off[r + 1] && 2 * F >= (int64_t)tisv * (j + 2);
  const int64_t s0 = ok ? ((int64_t)tisv * j) >> 1 : 0;
  const float* src = mel + r * n_mels * F_max + s0;
  float* dst = out + w * n_mels * tisv;
  const int n = n_mels * tisv;
  for (int i = threadIdx.x; i < n; i += VAD_THREADS) {
    const int c = i / tisv, t = i - c * tisv;
    dst[i] = ok ? src[c * F_max + t] : 0.f;
  }
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int64_t fs2_nonsilent_split_ws_bytes(int64_t batch, int64_t samples, int64_t hop) {
  if (batch < 1 || samples < 1 || hop < 1) return 0;
  return batch * (1 + samples / hop) * (int64_t)sizeof(float);
}

int fs2_nonsilent_split(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                        int64_t frame_length, int64_t hop, double top_db, int pad_mode,
                        int64_t* intervals, int64_t max_intervals, int32_t* n_intervals,
                        float* power, float* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(frame_length >= 2 && frame_length <= VAD_MAX_FRAME && frame_length % 2 == 0,
                "fs2_nonsilent_split: frame_length %lld (even, 2..%d)", (long long)frame_length,
                VAD_MAX_FRAME);
  FS2_CHECK_ARG(hop >= 1 && hop <= frame_length, "fs2_nonsilent_split: hop %lld (1..%lld)",
                (long long)hop, (long long)frame_length);
  FS2_CHECK_ARG(pad_mode == 0 || pad_mode == 1, "fs2_nonsilent_split: pad_mode %d (0 reflect, 1 zero)",
                pad_mode);
  FS2_CHECK_ARG(top_db == top_db, "fs2_nonsilent_split: top_db is NaN");
  FS2_CHECK_ARG(samples >= 1 && samples < (1ll << 30), "fs2_nonsilent_split: samples %lld (1..2^30 - 1)",
                (long long)samples);
  FS2_CHECK_ARG(batch >= 0 && max_intervals >= 0, "fs2_nonsilent_split: batch %lld, max_intervals %lld",
                (long long)batch, (long long)max_intervals);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && n_intervals && (intervals || max_intervals == 0),
                "fs2_nonsilent_split: missing operand");
  const int64_t F_max = 1 + samples / hop;
  FS2_CHECK_ARG(power || (ws && ws_bytes >= fs2_nonsilent_split_ws_bytes(batch, samples, hop)),
                "fs2_nonsilent_split: without power the workspace holds it (%lld bytes)",
                (long long)fs2_nonsilent_split_ws_bytes(batch, samples, hop));
  int64_t fpb = (VAD_SPAN_CAP - frame_length) / hop + 1;
  fpb = fpb > VAD_MAX_FPB ? VAD_MAX_FPB : fpb;
  const int64_t tiles = (F_max + fpb - 1) / fpb;
  FS2_CHECK_ARG(batch * tiles < (1ll << 31), "fs2_nonsilent_split: batch %lld x %lld tiles too large",
                (long long)batch, (long long)tiles);
  hipStream_t st = as_stream(stream);
  float* pw = power;
  if (!pw) {
    poison(ws, ws_bytes, st);
    pw = ws;
  }
  Vad a{wav, lens, samples, F_max, (int)frame_length, (int)hop, (int)fpb, (int)tiles, pad_mode,
        ((uintptr_t)wav & 15) == 0, pw};
  const size_t lds = sizeof(float) * (size_t)((fpb - 1) * hop + frame_length + 3);  // + the shift
  frame_power_kernel<<<(unsigned)(batch * tiles), VAD_THREADS, lds, st>>>(a);
  int rc = launch_status("fs2_nonsilent_split (frame powers)");
  if (rc != FS2_OK) return rc;
  VadRuns q{pw, lens, samples, F_max, max_intervals, (int)hop, 1e-10, pow(10.0, -top_db / 10.0),
            intervals, n_intervals};
  nonsilent_runs_kernel<<<(unsigned)batch, VAD_THREADS, 0, st>>>(q);
  return launch_status("fs2_nonsilent_split (runs)");
}

int fs2_wave_segments(const float* wav, int64_t batch, int64_t samples, const int32_t* seg_row,
                      const int64_t* seg_first, const int64_t* seg_len, int64_t n_seg, float* out,
                      int64_t out_samples, void* stream) {
  FS2_CHECK_ARG(batch >= 1 && samples >= 1 && samples < (1ll << 40),
                "fs2_wave_segments: wav of %lld x %lld", (long long)batch, (long long)samples);
  FS2_CHECK_ARG(out_samples >= 1 && out_samples < (1ll << 40), "fs2_wave_segments: out_samples %lld",
                (long long)out_samples);
  FS2_CHECK_ARG(n_seg >= 0, "fs2_wave_segments: n_seg %lld", (long long)n_seg);
  if (n_seg == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && seg_row && seg_first && seg_len && out, "fs2_wave_segments: missing operand");
  const int64_t tiles = (out_samples + WS_TILE - 1) / WS_TILE;
  FS2_CHECK_ARG(n_seg * tiles < (1ll << 31), "fs2_wave_segments: %lld segments x %lld tiles too large",
                (long long)n_seg, (long long)tiles);
  Segs a{wav, batch, samples, seg_row, seg_first, seg_len, out, out_samples, (int)tiles,
         ((uintptr_t)wav & 15) == 0,
         ((uintptr_t)out & 15) == 0 && out_samples % 4 == 0};
  wave_segments_kernel<<<(unsigned)(n_seg * tiles), VAD_THREADS, 0, as_stream(stream)>>>(a);
  return launch_status("fs2_wave_segments");
}

int fs2_tisv_windows(const float* mel, const int64_t* n_frames, int64_t rows, int64_t n_mels,
                     int64_t frames, int64_t tisv, const int64_t* win_off, int64_t n_windows,
                     float* out, void* stream) {
  FS2_CHECK_ARG(tisv >= 1 && tisv <= TW_TMAX, "fs2_tisv_windows: tisv %lld (1..%d)", (long long)tisv,
                TW_TMAX);
  FS2_CHECK_ARG(n_mels >= 1 && n_mels <= TW_CMAX, "fs2_tisv_windows: n_mels %lld (1..%d)",
                (long long)n_mels, TW_CMAX);
  FS2_CHECK_ARG(rows >= 0 && frames >= 1 && n_windows >= 0 && n_windows < (1ll << 31),
                "fs2_tisv_windows: rows %lld, frames %lld, n_windows %lld", (long long)rows,
                (long long)frames, (long long)n_windows);
  if (n_windows == 0) return FS2_OK;
  FS2_CHECK_ARG(rows >= 1, "fs2_tisv_windows: %lld windows of no row", (long long)n_windows);
  FS2_CHECK_ARG(mel && n_frames && win_off && out, "fs2_tisv_windows: missing operand");
  tisv_windows_kernel<<<(unsigned)n_windows, VAD_THREADS, 0, as_stream(stream)>>>(
      mel, n_frames, rows, (int)n_mels, frames, (int)tisv, win_off, out);
  return launch_status("fs2_tisv_windows");
}

}  // extern "C"
