// fs2_resample: the rational polyphase FIR resampler that stands where the reference's
// Preprocessor.process_utterance calls librosa.load(wav_path, sr=22050)
// (preprocessor/preprocessor.py:186-189), over a ragged batch, with the trim of lines 187-189 as
// a per-row output window.  The filter is the caller's table (audio.resample_filter: a
// Kaiser-windowed sinc evaluated in fp64 exactly at the offsets needed, rounded once to fp32 and
// already scaled by L); include/fs2hip.h has the definition.
//
// Output g reads the table at r + k L, r = (g M + half) mod L, k = 0 .. K - 1 with
// K = floor(2 half / L) + 1, against the samples j = floor((g M + half) / L) - k.  Outputs L
// apart have the same r, hence the same taps, and samples exactly M apart.
//
// Tiling.  A block owns a tile of R P consecutive outputs of one row, P a multiple of L
// (L ceil(256 / L) for L <= 256, L itself up to 1024) and R = 4: thread t < P computes the
// outputs t, t + P, t + 2 P, t + 3 P of the tile, which share their taps, so a tap is loaded once
// for four multiply-adds.  The tile's sample span is contiguous ((R P - 1) M / L + K + 1 samples
// at the most) and is staged into LDS once, zeros where j falls outside [0, len) of the row --
// nothing past len is read.  A ratio whose span would not fit 48 KiB of LDS that way (or
// L > 1024) runs the same kernel with R = 1, P = 256.  g M + half is formed in 64 bits once per
// thread; everything after is a 32-bit offset from the tile's first sample.
//
// Table placement.  The table (43 227 floats = 169 KiB at 48 000 -> 22 050 Hz) does not fit the
// 160 KiB of LDS and is read from global memory in its natural order: at tap step k the lanes
// of a wave read table[r + k L] with their r spread over one window of L consecutive floats, so
// a wave instruction touches at most ceil(4 L / 128) + 1 cache lines (6 at L = 147, one address
// at L = 1), and the next step's window is the adjacent one.  The whole table stays in L2
// (4 MiB); no transposed copy is kept.
//
// Order.  One fp32 accumulator per output, samples ascending (k descending from K - 1), each
// product rounded before it is added: floating-point contraction is off in this file.  A tap
// past the table's end or a sample outside the row contributes a product of 0, which leaves the
// sum as it was, so the value is the sum over the live taps in ascending j and depends on the
// row's samples and on g only -- not on the batch, the tile, R or the window.
#include "common.hpp"

#pragma clang fp contract(off)

namespace fs2 {

constexpr int RS_MIN_P = 256, RS_MAX_P = 1024, RS_R = 4;
constexpr int RS_SPAN_CAP = 12288;  // floats of LDS a tile's samples may take (48 KiB)

struct Resample {
  const float* wav;
  const int64_t* lens;
  const float* table;
  const int64_t* first;
  const int64_t* count;
  int64_t S, out_cols;
  int L, M, half, K;
  int P;      // outputs per slot: a thread's outputs are P apart
  int tiles;  // blocks per row
  float* out;
  int64_t* out_lens;
};

template <int R>
__global__ __launch_bounds__(RS_MAX_P) void resample_kernel(Resample a) {
  extern __shared__ float span[];
  const int tid = threadIdx.x;
  const int L = a.L, M = a.M, half = a.half, K = a.K, P = a.P;
  const int64_t b = blockIdx.x / a.tiles;
  const int64_t n0 = (int64_t)(blockIdx.x - b * a.tiles) * (R * P);  // first output column
  int64_t len = a.lens ? a.lens[b] : a.S;
  len = len < 0 ? 0 : len > a.S ? a.S : len;
  const int64_t n_out = (len * L + M - 1) / M;
  int64_t first = a.first ? a.first[b] : 0;
  first = first < 0 ? 0 : first > n_out ? n_out : first;
  int64_t cnt = n_out - first;
  if (a.count) {
    const int64_t c = a.count[b];
    cnt = c < 0 ? 0 : c < cnt ? c : cnt;
  }
  cnt = cnt > a.out_cols ? a.out_cols : cnt;
  if (n0 == 0 && tid == 0) a.out_lens[b] = cnt;
  float* out_b = a.out + b * a.out_cols;
  if (n0 >= cnt) {  // past the row's window: zeros (block-uniform)
    if (tid < P) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int64_t col = n0 + tid + q * P;
        if (col < a.out_cols) out_b[col] = 0.f;
      }
    }
    return;
  }

  // the tile's samples: j_lo .. j_hi of its first and last live output
  const int64_t g0 = first + n0;
  const int live = (int)(cnt - n0 < R * P ? cnt - n0 : R * P);
  const int64_t j_lo = (g0 * M + half) / L - (K - 1);
  const int64_t j_hi = ((g0 + live - 1) * M + half) / L;
  const int span_n = (int)(j_hi - j_lo + 1);  // K <= span_n <= the launch's LDS (host)
  const float* row = a.wav + b * a.S;
  for (int i = tid; i < span_n; i += blockDim.x) {
    const int64_t p = j_lo + i;
    span[i] = p >= 0 && p < len ? row[p] : 0.f;
  }
  __syncthreads();
  if (tid >= P) return;

  const int64_t at = (g0 + tid) * M + half;
  const int64_t jt = at / L;
  const int r = (int)(at - jt * L);
  const int step = (P / L) * M;  // samples between a thread's outputs (R > 1: L divides P)
  const float* mine[R];          // mine[q][-k] is sample jt + q step - k
  bool ok[R];
#pragma unroll
  for (int q = 0; q < R; ++q) {
    ok[q] = tid + q * P < live;
    mine[q] = span + (ok[q] ? (int)(jt - j_lo) + q * step : K - 1);  // dead: anywhere staged
  }
  const float* tab = a.table + r;
  const int last = 2 * half - r;  // largest offset from tab inside the table
  float acc[R];
#pragma unroll
  for (int q = 0; q < R; ++q) acc[q] = 0.f;
#pragma unroll 2
  for (int k = K - 1; k >= 0; --k) {
    const int o = k * L;
    const float t = o <= last ? tab[o] : 0.f;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const float prod = t * mine[q][-k];
      acc[q] = acc[q] + prod;
    }
  }
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int64_t col = n0 + tid + q * P;
    if (col < a.out_cols) out_b[col] = ok[q] ? acc[q] : 0.f;
  }
}

static int64_t gcd64(int64_t x, int64_t y) {
  while (y) {
    const int64_t t = x % y;
    x = y;
    y = t;
  }
  return x;
}

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_resample(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                 const float* table, int64_t table_len, int64_t up, int64_t down, int64_t half,
                 const int64_t* out_first, const int64_t* out_count, float* out,
                 int64_t out_samples, int64_t* out_lens, void* stream) {
  FS2_CHECK_ARG(up >= 1 && down >= 1 && up < (1 << 20) && down < (1 << 20),
                "fs2_resample: L %lld, M %lld (1..2^20 - 1)", (long long)up, (long long)down);
  FS2_CHECK_ARG(gcd64(up, down) == 1, "fs2_resample: L %lld and M %lld are not coprime",
                (long long)up, (long long)down);
  FS2_CHECK_ARG(half >= 1 && half < (1 << 28), "fs2_resample: half %lld", (long long)half);
  FS2_CHECK_ARG(table_len == 2 * half + 1, "fs2_resample: table of %lld taps, 2 half + 1 = %lld",
                (long long)table_len, (long long)(2 * half + 1));
  FS2_CHECK_ARG(samples >= 1 && samples < (1ll << 30), "fs2_resample: samples %lld (1..2^30 - 1)",
                (long long)samples);
  FS2_CHECK_ARG(batch >= 0, "fs2_resample: batch %lld", (long long)batch);
  FS2_CHECK_ARG(out_samples >= 1 && out_samples < (1ll << 40), "fs2_resample: out_samples %lld",
                (long long)out_samples);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && table && out && out_lens, "fs2_resample: missing operand");
  const int64_t taps = 2 * half / up + 1;
  // R outputs per thread where the ratio allows it, else one
  int64_t slots = RS_R, P = up <= RS_MIN_P ? up * ((RS_MIN_P + up - 1) / up) : up;
  int64_t span_cap = (slots * P - 1) * down / up + taps + 2;
  if (up > RS_MAX_P || span_cap > RS_SPAN_CAP) {
    slots = 1, P = RS_MIN_P;
    span_cap = (P - 1) * down / up + taps + 2;
  }
  FS2_CHECK_ARG(span_cap <= RS_SPAN_CAP,
                "fs2_resample: a tile of %lld outputs at %lld/%lld spans %lld samples (at most %d)",
                (long long)P, (long long)up, (long long)down, (long long)span_cap, RS_SPAN_CAP);
  const int64_t tiles = (out_samples + slots * P - 1) / (slots * P);
  FS2_CHECK_ARG(batch * tiles < (1ll << 31), "fs2_resample: batch %lld x %lld tiles too large",
                (long long)batch, (long long)tiles);
  Resample a{wav, lens, table, out_first, out_count, samples, out_samples, (int)up, (int)down,
             (int)half, (int)taps, (int)P, (int)tiles, out, out_lens};
  const dim3 grid((unsigned)(batch * tiles)), block((unsigned)((P + 63) / 64 * 64));
  const size_t lds = sizeof(float) * (size_t)span_cap;
  if (slots == RS_R)
    resample_kernel<RS_R><<<grid, block, lds, as_stream(stream)>>>(a);
  else
    resample_kernel<1><<<grid, block, lds, as_stream(stream)>>>(a);
  return launch_status("fs2_resample");
}

}  // extern "C"
