// Phoneme error rate: a general CTC loss with its logits gradient, the greedy CTC
// decoder and a batched edit distance with the substitution / deletion / insertion split.
//
//   ctc_loss        log-softmax over C classes per frame, alpha / beta in fp64 in the log domain
//                   over the 2L + 1 states of the blank-interleaved target, repeated labels allowed
//   ctc_greedy      per-frame arg-max, repeats collapsed, blanks dropped, labels compacted in order
//   edit_distance   one Levenshtein table per pair, swept by anti-diagonals, traced back in the
//                   same launch
//
// All three run one workgroup per utterance (or pair) with device int64 lengths that are never
// read back.  There are no atomics and every reduction has a fixed order, so a row has the same
// bits wherever it sits in a batch and from run to run.
//
// The loss kernel works in stages: (A) the frames' log-sum-exp, a wave per frame; (B) alpha, one
// state per thread and one barrier per frame, the previous row in LDS and every state's alpha to
// the workspace; (C) beta the same way backwards, each state's alpha replaced in the workspace by
// its posterior occupancy exp(alpha + beta - emission - ll); (D) the gradient, parallel over
// (frame, class): softmax minus the occupancies of the states that carry the class, summed in
// ascending state order along a class-to-positions chain built once per utterance (head[c] = the
// first target position with label c, next[i] = the next position with the label of i).  The
// blank's L + 1 states are summed per frame, in order, by a thread per frame before (D).
#include <math.h>

#include "common.hpp"

namespace fs2 {

constexpr int CT_T = 256, CT_W = CT_T / 64;
constexpr int CT_SI_MAX = (2 * FS2_CTC_MAX_TARGET + 1 + CT_T - 1) / CT_T;  // states per thread

FS2_DEV int ct_clamp(int64_t v, int lo, int hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }

FS2_DEV double ct_lse2(double a, double b) {
  const double m = fmax(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m));
}
FS2_DEV double ct_lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// the block's sum of v (integers: any order gives the same sum), the same in every thread
FS2_DEV int ct_block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < CT_W; ++w) s += red[w];
  return s;
}

// ---------------------------------------------------------------- ctc_loss
struct CtcArgs {
  const float* logits;
  const int64_t* targets;
  const int64_t* frame_lens;
  const int64_t* target_lens;
  const float* w;
  int T, ld, C, blank, L_max;
  float* nll;
  float* grad;
  double* ws;  // per row T x (2 L_max + 1): alpha, then the occupancies
};

// LDS: norm (T doubles), two state rows (2 x (2 L_max + 1) doubles), lab and next (L_max ints
// each), head (C ints).  CT_SI: the states a thread owns, (2 L_max + 1) / 256 rounded up to an
// instantiated count -- a batch of ordinary utterances (L_max <= 127) runs the one-state kernel
// without the register arrays of the widest.
template <int CT_SI>
__global__ __launch_bounds__(CT_T) void ctc_loss_kernel(CtcArgs a) {
  extern __shared__ double ct_lds[];
  __shared__ double ll_s;
  __shared__ int red[CT_W];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int T = a.T, ld = a.ld, C = a.C, blank = a.blank, L_max = a.L_max;
  const int M = ct_clamp(a.frame_lens[b], 1, T), L = ct_clamp(a.target_lens[b], 0, L_max);
  const int S = 2 * L + 1, SP = 2 * L_max + 1;
  double* norm = ct_lds;
  double* rows = norm + T;
  int* lab = reinterpret_cast<int*>(rows + 2 * SP);
  int* nxt = lab + L_max;
  int* head = nxt + L_max;
  int* has_prev = reinterpret_cast<int*>(rows);  // set-up only, before the rows are used
  const float* lg = a.logits + (int64_t)b * T * ld;
  float* gr = a.grad + (int64_t)b * T * ld;
  double* ws = a.ws + (int64_t)b * T * SP;
  const int64_t* tg = a.targets + (int64_t)b * L_max;
  const int cells = T * ld;

  // ---- the target: labels into LDS, a label outside [0, C) or equal to blank counted
  int bad = 0;
  for (int i = tid; i < L; i += CT_T) {
    const int64_t v = tg[i];
    const bool ok = v >= 0 && v < C && v != blank;
    bad += ok ? 0 : 1;
    lab[i] = ok ? (int)v : -1;
    has_prev[i] = 0;
  }
  for (int c = tid; c < C; c += CT_T) head[c] = -1;
  bad = ct_block_sum(bad, red);  // its barriers also publish lab
  int rep = 0;
  for (int i = tid + 1; i < L; i += CT_T) rep += lab[i] == lab[i - 1] ? 1 : 0;
  rep = ct_block_sum(rep, red);
  if (bad > 0 || M < L + rep) {  // no valid path (block-uniform)
    for (int e = tid; e < cells; e += CT_T) gr[e] = 0.f;
    if (tid == 0) a.nll[b] = INFINITY;
    return;
  }
  // ---- the chains: next position with the same label; a position nobody points at is a head
  for (int i = tid; i < L; i += CT_T) {
    const int v = lab[i];
    int j = i + 1;
    while (j < L && lab[j] != v) ++j;
    nxt[i] = j < L ? j : -1;
    if (j < L) has_prev[j] = 1;  // one writer: position j has one nearest predecessor
  }
  __syncthreads();
  for (int i = tid; i < L; i += CT_T)
    if (!has_prev[i]) head[lab[i]] = i;  // one writer per class
  // this thread's states j = tid + i CT_T: even = blank, odd = label (j - 1) / 2
  int col[CT_SI];
  bool sk_in[CT_SI], sk_out[CT_SI];
#pragma unroll
  for (int i = 0; i < CT_SI; ++i) {
    const int j = tid + i * CT_T, k = (j - 1) >> 1;
    const bool odd = (j & 1) && j < S;
    col[i] = odd ? lab[k] : blank;
    sk_in[i] = odd && k > 0 && lab[k] != lab[k - 1];
    sk_out[i] = odd && k + 1 < L && lab[k + 1] != lab[k];
  }
  __syncthreads();  // has_prev (in rows) has been read: the rows may be written
  // ---- (A) the frames' normalisers, a wave per frame
  for (int t = wave; t < M; t += CT_W) {
    const float* row = lg + (int64_t)t * ld;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
    m = wave_max(m);
    double sum = 0.0;
    for (int c = lane; c < C; c += 64) sum += exp((double)row[c] - (double)m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) norm[t] = (double)m + log(sum);
  }
  __syncthreads();
  const double ninf = -INFINITY;
  float el[CT_SI], el_next[CT_SI];
  // ---- (B) alpha
#pragma unroll
  for (int i = 0; i < CT_SI; ++i) el_next[i] = tid + i * CT_T < S ? lg[col[i]] : 0.f;
  for (int t = 0; t < M; ++t) {
    double* cur = rows + (t & 1) * SP;
    const double* prv = rows + ((t + 1) & 1) * SP;
    const double nt = norm[t];
#pragma unroll
    for (int i = 0; i < CT_SI; ++i) {
      el[i] = el_next[i];
      if (t + 1 < M && tid + i * CT_T < S) el_next[i] = lg[(int64_t)(t + 1) * ld + col[i]];
    }
#pragma unroll
    for (int i = 0; i < CT_SI; ++i) {
      const int j = tid + i * CT_T;
      if (j >= S) continue;
      const double e = (double)el[i] - nt;
      double al;
      if (t == 0) {
        al = j < 2 ? e : ninf;
      } else {
        al = e + ct_lse3(prv[j], j > 0 ? prv[j - 1] : ninf, sk_in[i] ? prv[j - 2] : ninf);
      }
      cur[j] = al;
      ws[(int64_t)t * SP + j] = al;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double* last = rows + ((M - 1) & 1) * SP;
    ll_s = S > 1 ? ct_lse2(last[S - 1], last[S - 2]) : last[0];
  }
  __syncthreads();
  const double ll = ll_s;
  if (!(ll > ninf && ll < INFINITY)) {  // scores that leave no path of finite probability
    for (int e = tid; e < cells; e += CT_T) gr[e] = 0.f;
    if (tid == 0) a.nll[b] = INFINITY;
    return;
  }
  if (tid == 0) a.nll[b] = (float)-ll;
  // ---- (C) beta, each state's alpha in the workspace replaced by its occupancy
  double a_cur[CT_SI], a_next[CT_SI];
#pragma unroll
  for (int i = 0; i < CT_SI; ++i) {
    const bool live = tid + i * CT_T < S;
    el_next[i] = live ? lg[(int64_t)(M - 1) * ld + col[i]] : 0.f;
    a_next[i] = live ? ws[(int64_t)(M - 1) * SP + tid + i * CT_T] : 0.0;
  }
  for (int t = M - 1; t >= 0; --t) {
    double* cur = rows + (t & 1) * SP;
    const double* nx = rows + ((t + 1) & 1) * SP;
    const double nt = norm[t];
#pragma unroll
    for (int i = 0; i < CT_SI; ++i) {
      el[i] = el_next[i];
      a_cur[i] = a_next[i];
      if (t > 0 && tid + i * CT_T < S) {
        el_next[i] = lg[(int64_t)(t - 1) * ld + col[i]];
        a_next[i] = ws[(int64_t)(t - 1) * SP + tid + i * CT_T];
      }
    }
#pragma unroll
    for (int i = 0; i < CT_SI; ++i) {
      const int j = tid + i * CT_T;
      if (j >= S) continue;
      const double e = (double)el[i] - nt;
      double be;
      if (t == M - 1) {
        be = j >= S - 2 ? e : ninf;
      } else {
        be = e + ct_lse3(nx[j], j + 1 < S ? nx[j + 1] : ninf, sk_out[i] ? nx[j + 2] : ninf);
      }
      cur[j] = be;
      // a state no path passes through at t (a -inf logit on its class makes alpha, beta and the
      // emission all -inf, and -inf - -inf is no number) has occupancy 0
      ws[(int64_t)t * SP + j] =
          a_cur[i] == ninf || be == ninf ? 0.0 : exp(a_cur[i] + be - e - ll);
    }
    __syncthreads();
  }
  // ---- the blank's L + 1 states per frame, in state order, left in the slot of state 0
  for (int t = tid; t < M; t += CT_T) {
    double* oc = ws + (int64_t)t * SP;
    double sum = 0.0;
    for (int s = 0; s <= L; ++s) sum += oc[2 * s];
    oc[0] = sum;
  }
  __syncthreads();  // written by this block: visible to it after the barrier
  // ---- (D) grad[t, c] = w (softmax[t, c] - occupancy of class c at t)
  const double wb = (double)a.w[b];
  for (int e = tid; e < cells; e += CT_T) {
    const int t = e / ld, c = e - t * ld;
    float g = 0.f;
    if (t < M && c < C) {
      const double* oc = ws + (int64_t)t * SP;
      double occ = 0.0;
      if (c == blank) {
        occ = oc[0];
      } else {
        for (int i = head[c]; i >= 0; i = nxt[i]) occ += oc[2 * i + 1];
      }
      g = (float)(wb * (exp((double)lg[e] - norm[t]) - occ));
    }
    gr[e] = g;
  }
}

// ---------------------------------------------------------------- ctc_greedy
// exclusive count of `flag` over the threads before this one; total over the block
FS2_DEV int ct_block_offsets(bool flag, int* wave_tot, int& total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(flag);
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();  // wave_tot may still be read from the previous call
  if (lane == 0) wave_tot[wave] = __popcll(m);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < CT_W; ++w) {
    base += w < wave ? wave_tot[w] : 0;
    total += wave_tot[w];
  }
  return base + before;
}

__global__ __launch_bounds__(CT_T) void ctc_greedy_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ frame_lens, int T, int ld, int C,
    int blank, int64_t* __restrict__ ids, int64_t* __restrict__ lens, int* __restrict__ argmax) {
  __shared__ int am[FS2_CTC_MAX_T];
  __shared__ int wave_tot[CT_W];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int M = ct_clamp(frame_lens[b], 1, T);
  const float* lg = logits + (int64_t)b * T * ld;
  // a wave per frame: the largest value that is not a NaN, the lowest class on a tie
  for (int t = wave; t < M; t += CT_W) {
    const float* row = lg + (int64_t)t * ld;
    float bv = 0.f;
    int bi = -1;
    for (int c = lane; c < C; c += 64) {
      const float v = row[c];
      if (v == v && (bi < 0 || v > bv)) bv = v, bi = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
    }
    if (lane == 0) am[t] = bi < 0 ? blank : bi;
  }
  __syncthreads();
  int64_t* out = ids + (int64_t)b * T;
  int count = 0;
  for (int t0 = 0; t0 < M; t0 += CT_T) {
    const int t = t0 + tid;
    const bool keep = t < M && am[t] != blank && (t == 0 || am[t] != am[t - 1]);
    int n;
    const int pos = count + ct_block_offsets(keep, wave_tot, n);
    if (keep) out[pos] = am[t];
    count += n;
  }
  for (int i = count + tid; i < T; i += CT_T) out[i] = 0;
  if (tid == 0) lens[b] = count;
  if (argmax)
    for (int t = tid; t < T; t += CT_T) argmax[(int64_t)b * T + t] = t < M ? am[t] : blank;
}

// ---------------------------------------------------------------- edit_distance
// Cell (i, j) = the distance between the first i reference and the first j hypothesis symbols.
// Lanes run along i on the anti-diagonal d = i + j; the diagonals d - 1 and d - 2 are in LDS.
// One step code per cell, diagonal-major, to the workspace: 0 match, 3 substitution, 1 deletion,
// 2 insertion.
__global__ __launch_bounds__(CT_T) void edit_distance_kernel(
    const int64_t* __restrict__ ref, const int64_t* __restrict__ hyp,
    const int64_t* __restrict__ ref_lens, const int64_t* __restrict__ hyp_lens, int R_max,
    int H_max, int64_t* __restrict__ out, unsigned char* __restrict__ steps) {
  extern __shared__ int ed_lds[];  // 3 x (R_max + 1)
  __shared__ int dist_s;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int R = ct_clamp(ref_lens[p], 0, R_max), H = ct_clamp(hyp_lens[p], 0, H_max);
  const int inner = R_max + 1;
  const int64_t* r = ref + (int64_t)p * R_max;
  const int64_t* h = hyp + (int64_t)p * H_max;
  unsigned char* st = steps + (int64_t)p * (R_max + H_max + 1) * inner;
  for (int d = 0; d <= R + H; ++d) {
    int* cur = ed_lds + (d % 3) * inner;
    const int* p1 = ed_lds + ((d + 2) % 3) * inner;  // diagonal d - 1
    const int* p2 = ed_lds + ((d + 1) % 3) * inner;  // diagonal d - 2
    const int lo = max(0, d - H), hi = min(d, R);
    for (int i = lo + tid; i <= hi; i += CT_T) {
      const int j = d - i;
      int D, code;
      if (i == 0) {
        D = j, code = 2;
      } else if (j == 0) {
        D = i, code = 1;
      } else {
        const int sub = r[i - 1] != h[j - 1] ? 1 : 0;
        D = p2[i - 1] + sub, code = sub ? 3 : 0;      // (i-1, j-1)
        const int del = p1[i - 1] + 1;                // (i-1, j): a reference symbol alone
        const int ins = p1[i] + 1;                    // (i, j-1)
        if (del < D) D = del, code = 1;
        if (ins < D) D = ins, code = 2;
      }
      cur[i] = D;
      st[(int64_t)d * inner + i] = (unsigned char)code;
      if (d == R + H) dist_s = D;  // the one cell of the last diagonal
    }
    __syncthreads();  // diagonal d complete; its readers (d + 1, d + 2) come before d + 3 writes
  }
  if (tid == 0) {  // the step bytes were written by this block: visible after the barrier
    int i = R, j = H, ns = 0, nd = 0, ni = 0;
    while (i > 0 || j > 0) {
      const int c = i == 0 ? 2 : j == 0 ? 1 : st[(int64_t)(i + j) * inner + i];
      if (c == 1) ++nd, --i;
      else if (c == 2) ++ni, --j;
      else ns += c == 3 ? 1 : 0, --i, --j;
    }
    int64_t* o = out + (int64_t)p * 4;
    o[0] = dist_s, o[1] = ns, o[2] = nd, o[3] = ni;
  }
}

static bool ct_batch_ok(int64_t b) { return b >= 0 && b <= 65535; }
static bool ct_frames_ok(int64_t t) { return t >= 1 && t <= FS2_CTC_MAX_T; }
static bool ct_classes_ok(int64_t c, int64_t ld, int64_t blank) {
  return c >= 1 && c <= FS2_CTC_MAX_CLASSES && ld >= c && ld <= 65535 && blank >= 0 && blank < c;
}
static bool ed_len_ok(int64_t n) { return n >= 0 && n <= FS2_EDIT_MAX_LEN; }

}  // namespace fs2

using namespace fs2;

extern "C" {

int64_t fs2_ctc_loss_ws_bytes(int64_t batch, int64_t t, int64_t l_max) {
  if (batch < 1 || !ct_batch_ok(batch) || !ct_frames_ok(t) || l_max < 0 ||
      l_max > FS2_CTC_MAX_TARGET)
    return 0;
  return batch * t * (2 * l_max + 1) * 8;
}

int fs2_ctc_loss(const float* logits, const int64_t* targets, const int64_t* frame_lens,
                 const int64_t* target_lens, const float* w, int64_t batch, int64_t t,
                 int64_t n_classes, int64_t ld, int64_t blank, int64_t l_max, float* nll,
                 float* grad, void* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(ct_frames_ok(t), "fs2_ctc_loss: T %lld (1..%d)", (long long)t, FS2_CTC_MAX_T);
  FS2_CHECK_ARG(l_max >= 0 && l_max <= FS2_CTC_MAX_TARGET, "fs2_ctc_loss: L_max %lld (0..%d)",
                (long long)l_max, FS2_CTC_MAX_TARGET);
  FS2_CHECK_ARG(ct_classes_ok(n_classes, ld, blank),
                "fs2_ctc_loss: C %lld (1..%d), ld %lld (C..65535), blank %lld (0..C - 1)",
                (long long)n_classes, FS2_CTC_MAX_CLASSES, (long long)ld, (long long)blank);
  FS2_CHECK_ARG(ct_batch_ok(batch), "fs2_ctc_loss: batch %lld (0..65535)", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(logits && (targets || l_max == 0) && frame_lens && target_lens && w && nll &&
                    grad && ws,
                "fs2_ctc_loss: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_ctc_loss_ws_bytes(batch, t, l_max),
                "fs2_ctc_loss: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_ctc_loss_ws_bytes(batch, t, l_max));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  CtcArgs a;
  a.logits = logits, a.targets = targets, a.frame_lens = frame_lens, a.target_lens = target_lens;
  a.w = w, a.T = (int)t, a.ld = (int)ld, a.C = (int)n_classes, a.blank = (int)blank;
  a.L_max = (int)l_max, a.nll = nll, a.grad = grad, a.ws = (double*)ws;
  const size_t lds = (size_t)(t + 2 * (2 * l_max + 1)) * sizeof(double) +
                     (size_t)(2 * l_max + n_classes) * sizeof(int);
  const int64_t need = (2 * l_max + 1 + CT_T - 1) / CT_T;
  if (need <= 1) ctc_loss_kernel<1><<<(unsigned)batch, CT_T, lds, st>>>(a);
  else if (need <= 2) ctc_loss_kernel<2><<<(unsigned)batch, CT_T, lds, st>>>(a);
  else if (need <= 4) ctc_loss_kernel<4><<<(unsigned)batch, CT_T, lds, st>>>(a);
  else ctc_loss_kernel<CT_SI_MAX><<<(unsigned)batch, CT_T, lds, st>>>(a);
  return launch_status("fs2_ctc_loss");
}

int fs2_ctc_greedy(const float* logits, const int64_t* frame_lens, int64_t batch, int64_t t,
                   int64_t n_classes, int64_t ld, int64_t blank, int64_t* ids, int64_t* lens,
                   int* argmax, void* stream) {
  FS2_CHECK_ARG(ct_frames_ok(t), "fs2_ctc_greedy: T %lld (1..%d)", (long long)t, FS2_CTC_MAX_T);
  FS2_CHECK_ARG(ct_classes_ok(n_classes, ld, blank),
                "fs2_ctc_greedy: C %lld (1..%d), ld %lld (C..65535), blank %lld (0..C - 1)",
                (long long)n_classes, FS2_CTC_MAX_CLASSES, (long long)ld, (long long)blank);
  FS2_CHECK_ARG(ct_batch_ok(batch), "fs2_ctc_greedy: batch %lld (0..65535)", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(logits && frame_lens && ids && lens, "fs2_ctc_greedy: missing operand");
  ctc_greedy_kernel<<<(unsigned)batch, CT_T, 0, as_stream(stream)>>>(
      logits, frame_lens, (int)t, (int)ld, (int)n_classes, (int)blank, ids, lens, argmax);
  return launch_status("fs2_ctc_greedy");
}

int64_t fs2_edit_distance_ws_bytes(int64_t batch, int64_t r_max, int64_t h_max) {
  if (batch < 1 || !ct_batch_ok(batch) || !ed_len_ok(r_max) || !ed_len_ok(h_max)) return 0;
  return batch * (r_max + h_max + 1) * (r_max + 1);
}

int fs2_edit_distance(const int64_t* ref, const int64_t* ref_lens, const int64_t* hyp,
                      const int64_t* hyp_lens, int64_t batch, int64_t r_max, int64_t h_max,
                      int64_t* out, void* ws, int64_t ws_bytes, void* stream) {
  FS2_CHECK_ARG(ed_len_ok(r_max) && ed_len_ok(h_max),
                "fs2_edit_distance: padded lengths %lld x %lld (0..%d each)", (long long)r_max,
                (long long)h_max, FS2_EDIT_MAX_LEN);
  FS2_CHECK_ARG(ct_batch_ok(batch), "fs2_edit_distance: batch %lld (0..65535)", (long long)batch);
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG((ref || r_max == 0) && (hyp || h_max == 0) && ref_lens && hyp_lens && out && ws,
                "fs2_edit_distance: missing operand");
  FS2_CHECK_ARG(ws_bytes >= fs2_edit_distance_ws_bytes(batch, r_max, h_max),
                "fs2_edit_distance: workspace %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)fs2_edit_distance_ws_bytes(batch, r_max, h_max));
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const size_t lds = 3 * (size_t)(r_max + 1) * sizeof(int);
  edit_distance_kernel<<<(unsigned)batch, CT_T, lds, st>>>(ref, hyp, ref_lens, hyp_lens,
                                                           (int)r_max, (int)h_max, out,
                                                           (unsigned char*)ws);
  return launch_status("fs2_edit_distance");
}

}  // extern "C"
