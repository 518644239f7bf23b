// pYIN (Mauch & Dixon 2014) as include/fs2hip.h defines it at fs2_f0_pyin: the thresholds of a
// prior distribution each vote for the lag plain YIN would pick, and a Viterbi pass over
// (pitch bin, voiced / unvoiced) states picks the track.
//
// pyin_candidates_kernel.  The block and LDS layout of f0_yin_kernel (pitch.hip): 4 waves, 8
// frames, the staged span, TL lags per lane, d' left in LDS by the shared pt_dprime.  A pick can
// begin only where d' sets a new running minimum, so a wave scans the lag range once, 64 lags at
// a time (a prefix-min over the lanes marks the new minima), and hands each new minimum the
// thresholds it is the first to fall under: they are sorted, so each minimum takes a contiguous
// run off the top.  The runs ("groups", at most 100) are then taken in ascending threshold
// order -- the order the definition fixes for a bin's fp64 sum -- refined by the shared descent
// and parabola, binned, and merged into a per-frame entry list in the LDS slice that held the
// running sums.  That part is wave-uniform: every lane computes the same values and stores them
// to the same addresses, so no lane reads what another wrote.  The entries are scattered into
// dense (frame, bin) rows the block zeroed before its first barrier.
//
// pyin_viterbi_kernel.  One workgroup per row, delta double-buffered in LDS, the two transition
// rows tri * 0.99 and tri * 0.01 beside it.  A thread owns the bins tid, tid + 256, ... and both
// states of each, which read the same 2 (2 R + 1) predecessors: per frame it maximises over them
// (voiced before unvoiced, bins ascending, strict comparisons: the first maximum, as numpy's
// argmax; the loop is unrolled by 4 so that the LDS reads of four bins are in flight together),
// multiplies by the observation (its loads issued before the maximisation), and after the
// block-wide maximum (first barrier) writes the normalised value (second barrier).  Back-pointers
// are int16 in the caller's workspace; one lane traces them back.  Every operation is an IEEE
// fp64 multiply, divide or compare with contraction off, so numpy gives the same bits.
#include <math.h>

#include "yin_core.hpp"

#pragma clang fp contract(off)

namespace fs2 {

constexpr int PY_NTHR = 100;        // thresholds i / 100, i = 1..100
constexpr double PY_STEP = 60.0;    // bins per octave: 12 semitones of 5
constexpr double PY_ABSENT = 0.01;  // weight of a threshold nothing fell under
constexpr double PY_FLOOR = 1e-9, PY_STAY = 0.99, PY_SWITCH = 0.01;
constexpr int PY_BIN_CAP = 1024, PY_REACH_CAP = 1023;

// one frame's scratch inside its PT_DLEN-float slice of region A (2080 bytes)
constexpr int PY_OFF_F0 = 8 * PY_NTHR, PY_OFF_BIN = PY_OFF_F0 + 4 * PY_NTHR,
              PY_OFF_GTAU = PY_OFF_BIN + 2 * PY_NTHR, PY_OFF_GILO = PY_OFF_GTAU + 2 * (PY_NTHR + 4),
              PY_SCRATCH = PY_OFF_GILO + 2 * (PY_NTHR + 4);
static_assert(PY_SCRATCH <= PT_DLEN * 4, "a frame's scratch fits the slice its running sums had");

struct PyinCand {
  const float* wav;
  const int64_t* lens;
  int64_t S;
  int hop;
  int64_t F_max;
  int chunks;  // blocks per utterance
  int tmin, tmax;
  float sr, lo, hi;
  int nb;
  const double* prior;  // w_1 .. w_100
  double* mass;         // (batch, F_max, nb)
  float* cf0;           // (batch, F_max, nb)
  double* voiced;       // (batch, F_max)
  float* unvoiced;      // (batch, F_max), nullable
  int64_t* n_frames;
};

FS2_DEV float py_theta(int i) { return (float)((double)i / 100.0); }

// the entry holding `bin` among the first `ne` (every lane has stored every entry), or -1
FS2_DEV int py_find(const short* ebin, int ne, int bin, int lane) {
  const unsigned long long m0 = __ballot(lane < ne && ebin[lane] == bin);
  const unsigned long long m1 = __ballot(lane + 64 < ne && ebin[lane + 64] == bin);
  return m0 ? __ffsll((long long)m0) - 1 : m1 ? 64 + __ffsll((long long)m1) - 1 : -1;
}

template <int TL>
__global__ __launch_bounds__(64 * PT_WAVES) void pyin_candidates_kernel(PyinCand a) {
  extern __shared__ double smem_f64[];
  float* smem = reinterpret_cast<float*>(smem_f64);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hop = a.hop, tmin = a.tmin, tmax = a.tmax, nb = a.nb;
  const int64_t b = blockIdx.x / a.chunks;
  const int fr0 = (int)(blockIdx.x - b * a.chunks) * PT_FPB;
  const int64_t F_max = a.F_max;
  const int len = pt_row_len(a.lens, b, a.S);
  const int nf = 1 + len / hop;
  if (fr0 == 0 && tid == 0) a.n_frames[b] = nf;
  const int fcnt = (int)(F_max - fr0 < PT_FPB ? F_max - fr0 : PT_FPB);
  const int64_t fbase = b * F_max + fr0;
  double* mass_blk = a.mass + fbase * nb;
  float* cf0_blk = a.cf0 + fbase * nb;
  // the dense rows start as zeros; the barriers of pt_dprime order this before the scatter
  for (int i = tid; i < fcnt * nb; i += 64 * PT_WAVES) mass_blk[i] = 0.0, cf0_blk[i] = 0.f;
  if (fr0 >= nf) {  // past the utterance (block-uniform)
    if (tid < fcnt) {
      a.voiced[fbase + tid] = 0.0;
      if (a.unvoiced) a.unvoiced[fbase + tid] = 0.f;
    }
    return;
  }
  const float* dall = pt_dprime<TL>(smem, a.wav + b * a.S, len, fr0, hop, tmax);

#pragma unroll 1
  for (int q = 0; q < PT_FPW; ++q) {
    const int jf = wave * PT_FPW + q, fr = fr0 + jf;
    if (fr >= F_max) continue;  // wave-uniform
    if (fr >= nf) {
      if (lane == 0) {
        a.voiced[fbase + jf] = 0.0;
        if (a.unvoiced) a.unvoiced[fbase + jf] = 0.f;
      }
      continue;
    }
    const float* d = dall + jf * PT_DLEN;
    char* scr = reinterpret_cast<char*>(smem) + (size_t)jf * PT_DLEN * 4;
    double* emass = reinterpret_cast<double*>(scr);
    float* ef0 = reinterpret_cast<float*>(scr + PY_OFF_F0);
    short* ebin = reinterpret_cast<short*>(scr + PY_OFF_BIN);
    short* gtau = reinterpret_cast<short*>(scr + PY_OFF_GTAU);
    short* gilo = reinterpret_cast<short*>(scr + PY_OFF_GILO);

    // one ascending scan: group g starts at lag gtau[g] and holds the thresholds
    // gilo[g] .. gilo[g - 1] - 1 (.. 100 for g = 0); next_i is the highest threshold still open
    int next_i = PY_NTHR, ng = 0, last_new = tmin;
    float run = INFINITY;
    for (int base = tmin; base <= tmax && next_i >= 1; base += 64) {
      const int tau = base + lane;
      const float v = tau <= tmax ? d[tau] : INFINITY;
      float p = v;  // inclusive prefix minimum over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(p, o, 64);
        if (lane >= o) p = fminf(p, t);
      }
      float excl = __shfl_up(p, 1, 64);
      excl = lane == 0 ? run : fminf(excl, run);
      unsigned long long mask = __ballot(v < excl);
      run = fminf(run, __shfl(p, 63, 64));
      while (mask && next_i >= 1) {
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const float val = __shfl(v, l, 64);
        last_new = base + l;
        const int before = next_i;
        while (next_i >= 1 && val < py_theta(next_i)) --next_i;
        if (next_i < before) {
          gtau[ng] = (short)(base + l);
          gilo[ng] = (short)(next_i + 1);
          ++ng;
        }
      }
    }

    // ascending thresholds: those nothing fell under (g = ng, the first minimum of d', which is
    // the last new running minimum of a completed scan), then the groups last to first
    int ne = 0;
    for (int g = ng; g >= 0; --g) {
      const bool absent = g == ng;
      int tau, ilo, ihi;
      if (absent) {
        if (next_i < 1) continue;
        tau = last_new, ilo = 1, ihi = next_i;
        if (!(d[tau] < 1.f)) continue;  // d' is 1 by convention where there is no energy: no vote
      } else {
        tau = gtau[g], ilo = gilo[g], ihi = g == 0 ? PY_NTHR : gilo[g - 1] - 1;
      }
      const float f = pt_refine(d, tau, tmax, a.sr);
      if (f < a.lo || f > a.hi) continue;  // counts as unvoiced
      const double pos = rint(PY_STEP * log2((double)f / (double)a.lo));
      const int bin = pos < 0.0 ? 0 : pos > (double)(nb - 1) ? nb - 1 : (int)pos;
      int e = py_find(ebin, ne, bin, lane);
      double m = 0.0;
      if (e < 0) {
        e = ne++;
        ebin[e] = (short)bin;
        ef0[e] = f;
      } else {
        m = emass[e];
      }
      for (int i = ilo; i <= ihi; ++i) {
        const double w = a.prior[i - 1];
        const double wa = w * PY_ABSENT;
        m = m + (absent ? wa : w);
      }
      emass[e] = m;
    }

    // v = min(sum_b mass_b, 1), b ascending
    double v = 0.0;
    int last = -1;
    for (int n = 0; n < ne; ++n) {
      const int c0 = lane < ne && ebin[lane] > last ? ebin[lane] : 0x7fff;
      const int c1 = lane + 64 < ne && ebin[lane + 64] > last ? ebin[lane + 64] : 0x7fff;
      int c = c0 < c1 ? c0 : c1;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(c, o, 64);
        c = c < t ? c : t;
      }
      v = v + emass[py_find(ebin, ne, c, lane)];
      last = c;
    }
    v = v < 1.0 ? v : 1.0;

    double* mass_row = mass_blk + (int64_t)jf * nb;
    float* cf0_row = cf0_blk + (int64_t)jf * nb;
    for (int e = lane; e < ne; e += 64) {
      mass_row[ebin[e]] = emass[e];
      cf0_row[ebin[e]] = ef0[e];
    }
    if (lane == 0) {
      a.voiced[fbase + jf] = v;
      if (a.unvoiced) a.unvoiced[fbase + jf] = (float)(1.0 - v);
    }
  }
}

// ------------------------------------------------------------------ Viterbi
constexpr int PV_T = 256, PV_WAVES = PV_T / 64, PV_PER = PY_BIN_CAP / PV_T;

struct PyinVit {
  const double* mass;    // (batch, F, nb)
  const double* voiced;  // (batch, F)
  const int64_t* n_frames;
  int64_t F;
  int nb, R;
  const double* tri;     // tri(0 .. R)
  const float* cf0;      // (batch, F, nb), with f0
  const float* centres;  // (nb), with f0
  int16_t* bp;           // (batch, F, 2 nb)
  int* path;             // (batch, F)
  float* f0;             // (batch, F), nullable
};

FS2_DEV double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// A thread owns the bins tid, tid + PV_T, ... and of each both states.  obs_k of its voiced
// states; every unvoiced state has obs_k = un.
FS2_DEV void pv_load_obs(const PyinVit& a, const double* mass_b, const double* voiced_b, int64_t k,
                         double (&o)[PV_PER], double& un) {
  const int nb = a.nb;
  un = (1.0 - voiced_b[k]) / (double)nb + PY_FLOOR;
#pragma unroll
  for (int r = 0; r < PV_PER; ++r) {
    const int bq = (int)threadIdx.x + r * PV_T;
    o[r] = bq < nb ? mass_b[k * nb + bq] + PY_FLOOR : 0.0;
  }
}

// the block-wide maximum of the threads' values (all non-negative); one barrier
FS2_DEV double pv_block_max(const double (&vv)[PV_PER], const double (&vu)[PV_PER], int nb,
                            double* wmax) {
  double m = 0.0;
#pragma unroll
  for (int r = 0; r < PV_PER; ++r)
    if ((int)threadIdx.x + r * PV_T < nb) m = fmax(m, fmax(vv[r], vu[r]));
  m = wave_max_f64(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  double mx = wmax[0];
#pragma unroll
  for (int w = 1; w < PV_WAVES; ++w) mx = fmax(mx, wmax[w]);
  return mx;
}

__global__ __launch_bounds__(PV_T) void pyin_viterbi_kernel(PyinVit a) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = a.nb, S = 2 * nb, R = a.R;
  double* p_stay = sm + 2 * S;
  double* p_move = p_stay + (R + 1);
  double* wmax = p_move + (R + 1);
  int* widx = reinterpret_cast<int*>(wmax + PV_WAVES);
  const int64_t b = blockIdx.x, F = a.F;
  int64_t nf = a.n_frames ? a.n_frames[b] : F;
  nf = nf < 0 ? 0 : nf > F ? F : nf;
  int* path_b = a.path + b * F;
  float* f0_b = a.f0 ? a.f0 + b * F : nullptr;
  for (int64_t k = nf + tid; k < F; k += PV_T) {
    path_b[k] = -1;
    if (f0_b) f0_b[k] = 0.f;
  }
  if (nf == 0) return;  // block-uniform
  for (int dl = tid; dl <= R; dl += PV_T) {
    const double t = a.tri[dl];
    p_stay[dl] = t * PY_STAY;
    p_move[dl] = t * PY_SWITCH;
  }
  const double* mass_b = a.mass + b * F * nb;
  const double* voiced_b = a.voiced + b * F;
  int16_t* bp_b = a.bp + b * F * S;

  double val_v[PV_PER], val_u[PV_PER], obs[PV_PER], un;
  pv_load_obs(a, mass_b, voiced_b, 0, obs, un);
#pragma unroll
  for (int r = 0; r < PV_PER; ++r) val_v[r] = obs[r] / (double)S, val_u[r] = un / (double)S;
  {
    const double mx = pv_block_max(val_v, val_u, nb, wmax);
#pragma unroll
    for (int r = 0; r < PV_PER; ++r) {
      const int bq = tid + r * PV_T;
      if (bq < nb) sm[bq] = val_v[r] / mx, sm[nb + bq] = val_u[r] / mx;
    }
  }
  __syncthreads();  // also covers p_stay / p_move

  for (int64_t k = 1; k < nf; ++k) {
    const double* cur = (k & 1) ? sm : sm + S;  // delta_(k - 1)
    double* nxt = (k & 1) ? sm + S : sm;
    pv_load_obs(a, mass_b, voiced_b, k, obs, un);  // consumed after the maximisation below
#pragma unroll
    for (int r = 0; r < PV_PER; ++r) {
      const int bq = tid + r * PV_T;
      val_v[r] = val_u[r] = 0.0;
      if (bq < nb) {
        // predecessors (voiced, bb) and (unvoiced, bb) of the targets (voiced, bq) and
        // (unvoiced, bq), bb ascending; strict comparisons: the first maximum
        double vv = 0.0, uv = 0.0, vu = 0.0, uu = 0.0;  // predecessor, target
        int a_vv = 0, a_uv = 0, a_vu = 0, a_uu = 0;
        const int lo = bq - R > 0 ? bq - R : 0, hi = bq + R < nb - 1 ? bq + R : nb - 1;
#pragma unroll 4
        for (int bb = lo; bb <= hi; ++bb) {
          const int ad = bb < bq ? bq - bb : bb - bq;
          const double ps = p_stay[ad], pm = p_move[ad];
          const double cv = cur[bb], cu = cur[nb + bb];
          const double t_vv = cv * ps, t_uv = cu * pm, t_vu = cv * pm, t_uu = cu * ps;
          if (t_vv > vv) vv = t_vv, a_vv = bb;
          if (t_uv > uv) uv = t_uv, a_uv = bb;
          if (t_vu > vu) vu = t_vu, a_vu = bb;
          if (t_uu > uu) uu = t_uu, a_uu = bb;
        }
        // an unvoiced predecessor only if strictly better; every product 0: numpy's first
        // maximum is state 0
        const int to_v = uv > vv ? nb + a_uv : vv > 0.0 ? a_vv : 0;
        const int to_u = uu > vu ? nb + a_uu : vu > 0.0 ? a_vu : 0;
        bp_b[k * S + bq] = (int16_t)to_v;
        bp_b[k * S + nb + bq] = (int16_t)to_u;
        val_v[r] = (uv > vv ? uv : vv) * obs[r];
        val_u[r] = (uu > vu ? uu : vu) * un;
      }
    }
    const double mx = pv_block_max(val_v, val_u, nb, wmax);
#pragma unroll
    for (int r = 0; r < PV_PER; ++r) {
      const int bq = tid + r * PV_T;
      if (bq < nb) nxt[bq] = val_v[r] / mx, nxt[nb + bq] = val_u[r] / mx;
    }
    __syncthreads();
  }

  // the lowest state whose normalised value is the maximum, 1
  {
    const double* fin = ((nf - 1) & 1) ? sm + S : sm;
    int idx = 0x7fffffff;
#pragma unroll
    for (int r = PV_PER - 1; r >= 0; --r) {
      const int bq = tid + r * PV_T;
      if (bq < nb && fin[nb + bq] == 1.0) idx = nb + bq;
    }
#pragma unroll
    for (int r = PV_PER - 1; r >= 0; --r) {  // a voiced state is the lower index
      const int bq = tid + r * PV_T;
      if (bq < nb && fin[bq] == 1.0) idx = bq;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int t = __shfl_xor(idx, o, 64);
      idx = idx < t ? idx : t;
    }
    if (lane == 0) widx[wave] = idx;
  }
  __syncthreads();  // the back-pointers are visible to the block as well
  if (tid == 0) {
    int s = widx[0];
    for (int w = 1; w < PV_WAVES; ++w) s = s < widx[w] ? s : widx[w];
    s = s < S ? s : 0;
    path_b[nf - 1] = s;
    for (int64_t k = nf - 1; k >= 1; --k) {
      s = bp_b[k * S + s];
      path_b[k - 1] = s;
    }
  }
  if (!f0_b) return;
  __syncthreads();
  const float* cf0_b = a.cf0 + b * F * nb;
  for (int64_t k = tid; k < nf; k += PV_T) {
    const int s = path_b[k];
    float f = 0.f;
    if (s < nb) {
      f = cf0_b[k * nb + s];
      if (f == 0.f) f = a.centres[s];
    }
    f0_b[k] = f;
  }
}

// ------------------------------------------------------------------ host side
struct PyinLags {
  int tmin, tmax;
};

static int pyin_check(const char* who, int64_t batch, int64_t samples, int64_t hop, double sr,
                      double f0_floor, double f0_ceil, int64_t n_bins, PyinLags* lags) {
  FS2_CHECK_ARG(hop >= 1 && hop <= 1024, "%s: hop %lld (1..1024)", who, (long long)hop);
  FS2_CHECK_ARG(samples >= 1 && samples < (1ll << 30), "%s: samples %lld (1..2^30 - 1)", who,
                (long long)samples);
  FS2_CHECK_ARG(batch >= 0, "%s: batch %lld", who, (long long)batch);
  FS2_CHECK_ARG(sr > 0 && f0_floor > 0 && f0_ceil >= f0_floor, "%s: sr %g, f0 range %g..%g", who,
                sr, f0_floor, f0_ceil);
  FS2_CHECK_ARG(n_bins >= 1 && n_bins <= PY_BIN_CAP, "%s: %lld pitch bins (1..%d)", who,
                (long long)n_bins, PY_BIN_CAP);
  const double tmax_d = floor(sr / f0_floor), tmin_d = ceil(sr / f0_ceil);
  FS2_CHECK_ARG(tmax_d <= PT_TAU_CAP, "%s: sr / f0_floor = %g lags (at most %d are built)", who,
                tmax_d, PT_TAU_CAP);
  FS2_CHECK_ARG(tmin_d >= 1 && tmin_d <= tmax_d, "%s: lags %g..%g", who, tmin_d, tmax_d);
  const int64_t F_max = 1 + samples / hop;
  FS2_CHECK_ARG(batch * ((F_max + PT_FPB - 1) / PT_FPB) < (1ll << 31),
                "%s: batch %lld x %lld frames too large", who, (long long)batch, (long long)F_max);
  lags->tmin = (int)tmin_d, lags->tmax = (int)tmax_d;
  return FS2_OK;
}

static int viterbi_check(const char* who, int64_t batch, int64_t frames, int64_t n_bins,
                         int64_t reach) {
  FS2_CHECK_ARG(batch >= 0 && batch < (1ll << 31), "%s: batch %lld", who, (long long)batch);
  FS2_CHECK_ARG(frames >= 1 && frames < (1ll << 31), "%s: frames %lld", who, (long long)frames);
  FS2_CHECK_ARG(n_bins >= 1 && n_bins <= PY_BIN_CAP, "%s: %lld pitch bins (1..%d)", who,
                (long long)n_bins, PY_BIN_CAP);
  FS2_CHECK_ARG(reach >= 0 && reach <= PY_REACH_CAP, "%s: reach %lld bins (0..%d)", who,
                (long long)reach, PY_REACH_CAP);
  return FS2_OK;
}

static int candidates_launch(const PyinCand& a, int64_t batch, hipStream_t st) {
  const int tl = pt_lags_per_lane(a.tmax);
  const size_t lds = pt_lds_bytes(a.hop, tl);
  const dim3 grid((unsigned)(batch * a.chunks));
  switch (tl) {
    case 1: pyin_candidates_kernel<1><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    case 3: pyin_candidates_kernel<3><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    case 5: pyin_candidates_kernel<5><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    case 7: pyin_candidates_kernel<7><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
    default: pyin_candidates_kernel<9><<<grid, 64 * PT_WAVES, lds, st>>>(a); break;
  }
  return launch_status("fs2_f0_pyin_candidates");
}

static int viterbi_launch(const PyinVit& a, int64_t batch, hipStream_t st) {
  const size_t lds = sizeof(double) * (size_t)(4 * a.nb + 2 * (a.R + 1) + PV_WAVES) +
                     sizeof(int) * PV_WAVES;
  pyin_viterbi_kernel<<<dim3((unsigned)batch), PV_T, lds, st>>>(a);
  return launch_status("fs2_f0_pyin_viterbi");
}

static int64_t round8(int64_t v) { return (v + 7) & ~int64_t(7); }

}  // namespace fs2

using namespace fs2;

extern "C" {

int fs2_f0_pyin_candidates(const float* wav, const int64_t* lens, int64_t batch, int64_t samples,
                           int64_t hop, double sr, double f0_floor, double f0_ceil,
                           const double* prior, int64_t n_bins, double* mass, float* cand_f0,
                           double* voiced, float* unvoiced, int64_t* n_frames, void* stream) {
  PyinLags lags;
  const int rc = pyin_check("fs2_f0_pyin_candidates", batch, samples, hop, sr, f0_floor, f0_ceil,
                            n_bins, &lags);
  if (rc != FS2_OK) return rc;
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && prior && mass && cand_f0 && voiced && n_frames,
                "fs2_f0_pyin_candidates: missing operand");
  const int64_t F_max = 1 + samples / hop;
  PyinCand a{wav, lens, samples, (int)hop, F_max, (int)((F_max + PT_FPB - 1) / PT_FPB), lags.tmin,
             lags.tmax, (float)sr, (float)f0_floor, (float)f0_ceil, (int)n_bins, prior, mass,
             cand_f0, voiced, unvoiced, n_frames};
  return candidates_launch(a, batch, as_stream(stream));
}

int64_t fs2_f0_pyin_viterbi_ws_bytes(int64_t batch, int64_t frames, int64_t n_bins) {
  if (batch < 1 || frames < 1 || frames >= (1ll << 31) || n_bins < 1 || n_bins > PY_BIN_CAP)
    return 0;
  return round8(batch * frames * 2 * n_bins * (int64_t)sizeof(int16_t));
}

int fs2_f0_pyin_viterbi(const double* mass, const double* voiced, const int64_t* n_frames,
                        int64_t batch, int64_t frames, int64_t n_bins, const double* tri,
                        int64_t reach, const float* cand_f0, const float* centres, int* path,
                        float* f0, void* ws, int64_t ws_bytes, void* stream) {
  const int rc = viterbi_check("fs2_f0_pyin_viterbi", batch, frames, n_bins, reach);
  if (rc != FS2_OK) return rc;
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(mass && voiced && tri && path && ws, "fs2_f0_pyin_viterbi: missing operand");
  FS2_CHECK_ARG(!f0 || (cand_f0 && centres),
                "fs2_f0_pyin_viterbi: f0 needs the candidate f0 and the bin centres");
  const int64_t need = fs2_f0_pyin_viterbi_ws_bytes(batch, frames, n_bins);
  FS2_CHECK_ARG(ws_bytes >= need, "fs2_f0_pyin_viterbi: workspace %lld bytes, %lld needed",
                (long long)ws_bytes, (long long)need);
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  PyinVit a{mass, voiced, n_frames, frames, (int)n_bins, (int)reach, tri, cand_f0, centres,
            reinterpret_cast<int16_t*>(ws), path, f0};
  return viterbi_launch(a, batch, st);
}

int64_t fs2_f0_pyin_ws_bytes(int64_t batch, int64_t samples, int64_t hop, int64_t n_bins) {
  if (batch < 1 || samples < 1 || samples >= (1ll << 30) || hop < 1 || hop > 1024 || n_bins < 1 ||
      n_bins > PY_BIN_CAP)
    return 0;
  const int64_t n = batch * (1 + samples / hop);
  // masses, voiced, candidate f0, states, back-pointers
  return n * n_bins * 8 + n * 8 + round8(n * n_bins * 4) + round8(n * 4) +
         fs2_f0_pyin_viterbi_ws_bytes(batch, 1 + samples / hop, n_bins);
}

int fs2_f0_pyin(const float* wav, const int64_t* lens, int64_t batch, int64_t samples, int64_t hop,
                double sr, double f0_floor, double f0_ceil, const double* prior, const double* tri,
                int64_t reach, const float* centres, int64_t n_bins, float* f0, float* unvoiced,
                int64_t* n_frames, int* states, void* ws, int64_t ws_bytes, void* stream) {
  PyinLags lags;
  int rc = pyin_check("fs2_f0_pyin", batch, samples, hop, sr, f0_floor, f0_ceil, n_bins, &lags);
  if (rc != FS2_OK) return rc;
  const int64_t F_max = 1 + samples / hop;
  rc = viterbi_check("fs2_f0_pyin", batch, F_max, n_bins, reach);
  if (rc != FS2_OK) return rc;
  if (batch == 0) return FS2_OK;
  FS2_CHECK_ARG(wav && prior && tri && centres && f0 && unvoiced && n_frames && ws,
                "fs2_f0_pyin: missing operand");
  const int64_t need = fs2_f0_pyin_ws_bytes(batch, samples, hop, n_bins);
  FS2_CHECK_ARG(ws_bytes >= need, "fs2_f0_pyin: workspace %lld bytes, %lld needed",
                (long long)ws_bytes, (long long)need);
  hipStream_t st = as_stream(stream);
  poison(ws, ws_bytes, st);
  const int64_t n = batch * F_max;
  char* p = reinterpret_cast<char*>(ws);
  double* mass = reinterpret_cast<double*>(p);
  p += n * n_bins * 8;
  double* voiced = reinterpret_cast<double*>(p);
  p += n * 8;
  float* cf0 = reinterpret_cast<float*>(p);
  p += round8(n * n_bins * 4);
  int* path = states ? states : reinterpret_cast<int*>(p);
  p += round8(n * 4);
  PyinCand c{wav, lens, samples, (int)hop, F_max, (int)((F_max + PT_FPB - 1) / PT_FPB), lags.tmin,
             lags.tmax, (float)sr, (float)f0_floor, (float)f0_ceil, (int)n_bins, prior, mass, cf0,
             voiced, unvoiced, n_frames};
  rc = candidates_launch(c, batch, st);
  if (rc != FS2_OK) return rc;
  PyinVit v{mass, voiced, n_frames, F_max, (int)n_bins, (int)reach, tri, cf0, centres,
            reinterpret_cast<int16_t*>(p), path, f0};
  return viterbi_launch(v, batch, st);
}

}  // extern "C"
