// bf16 helpers around the conv / GEMM kernels: weight re-layout (fp32 master weights to the
// bf16 forward and data-gradient layouts), the fp32 -> bf16 cast and the bf16 column sum.  The
// GEMMs themselves are in gemm_glds / gemm_tapreg / wgrad_splitk / wgrad / wgrad_band.
#include "glds.hpp"

namespace fs2 {

__global__ void weight_prep_bf16(const float* w, int Cout, int Cin, int taps, u16* wf, u16* wb) {
  const int64_t total = (int64_t)Cout * Cin * taps;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = e / ((int64_t)Cin * taps);
    const int rem = (int)(e - o * Cin * taps);
    const int c = rem / taps, j = rem - c * taps;
    const u16 v = to_bf16(w[e]);
    if (wf) wf[o * (int64_t)taps * Cin + (int64_t)j * Cin + c] = v;
    if (wb) wb[(int64_t)c * taps * Cout + (int64_t)(taps - 1 - j) * Cout + o] = v;
  }
}

// All layers' re-layouts in one launch.  jobs[j] = {src, c_out, c_in, taps, w_fwd, w_bwd,
// first tile, end tile} (int64); a job has ceil(c_out/64) x ceil(c_in/CT) tiles, numbered
// consecutively over the jobs (CT = fs2_weight_prep_tile_channels).  Block b re-lays out
// one tile: 64 output channels x CT input channels x all taps.  The source rows are read as
// contiguous CT*taps runs into LDS (already cast), then w_fwd is written as CT-long runs per
// (o, tap) and w_bwd as 64-long runs per (c, tap).
template <typename OutT>
__global__ __launch_bounds__(256) void weight_prep_tiles(const int64_t* __restrict__ jobs, int n_jobs) {
  constexpr int CT = sizeof(OutT) == 2 ? 32 : 16;
  constexpr int MAXT = 9;
  constexpr int LD = CT * MAXT + 1;  // odd row stride (in OutT units of 2 or 4 B)
  __shared__ OutT tile[64 * LD];
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {  // last job whose first tile <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid * 8 + 6] <= (int64_t)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const int64_t* jb = jobs + (int64_t)lo * 8;
  const float* w = (const float*)jb[0];
  const int Cout = (int)jb[1], Cin = (int)jb[2], taps = (int)jb[3];
  OutT* wf = (OutT*)jb[4];
  OutT* wb = (OutT*)jb[5];
  const int t = (int)(blockIdx.x - jb[6]), tiles_c = (Cin + CT - 1) / CT;
  const int tc = t % tiles_c, to = t / tiles_c;
  const int o0 = to * 64, c0 = tc * CT;
  const int no = Cout - o0 < 64 ? Cout - o0 : 64;
  const int nc = Cin - c0 < CT ? Cin - c0 : CT;
  const int run = nc * taps;  // contiguous source elements per row
  const int64_t Q = (int64_t)Cin * taps;
  if constexpr (sizeof(OutT) == 2) {
    // 16-B vector path (full tiles of aligned rows: every step weight but the odd edges):
    // float4 source reads, 8 x bf16 = 16-B stores of w_fwd (8 channels of one (o, tap)) and
    // w_bwd (8 output channels of one (c, tap))
    const bool vec = no == 64 && nc == CT && (Q % 4) == 0 && (Cin % 8) == 0 && (Cout % 8) == 0 &&
                     (((uintptr_t)w | (uintptr_t)wf | (uintptr_t)wb) & 15) == 0;
    if (vec) {
      const int run4 = run / 4;  // CT * taps is a multiple of 4 (CT = 32)
      for (int e = threadIdx.x; e < 64 * run4; e += 256) {
        const int r = e / run4, q4 = e - r * run4;
        const f32x4 v = ld4(w + (int64_t)(o0 + r) * Q + (int64_t)c0 * taps + 4 * q4);
        OutT* t = tile + r * LD + 4 * q4;
        t[0] = to_bf16(v.x);
        t[1] = to_bf16(v.y);
        t[2] = to_bf16(v.z);
        t[3] = to_bf16(v.w);
      }
      __syncthreads();
      if (wf) {  // wf[o, j*Cin + c]: per (o, j) a run of CT = 4 x 8 channels
        for (int e = threadIdx.x; e < 64 * taps * (CT / 8); e += 256) {
          const int c8 = (e % (CT / 8)) * 8, rj = e / (CT / 8), j = rj % taps, r = rj / taps;
          const OutT* t = tile + r * LD + c8 * taps + j;
          uint4 o;
          o.x = (uint32_t)t[0] | ((uint32_t)t[taps] << 16);
          o.y = (uint32_t)t[2 * taps] | ((uint32_t)t[3 * taps] << 16);
          o.z = (uint32_t)t[4 * taps] | ((uint32_t)t[5 * taps] << 16);
          o.w = (uint32_t)t[6 * taps] | ((uint32_t)t[7 * taps] << 16);
          *reinterpret_cast<uint4*>(wf + (int64_t)(o0 + r) * Q + (int64_t)j * Cin + c0 + c8) = o;
        }
      }
      if (wb) {  // wb[c*taps + taps-1-j, o]: per (c, j) a run of 64 = 8 x 8 output channels
        for (int e = threadIdx.x; e < CT * taps * 8; e += 256) {
          const int r8 = (e & 7) * 8, cj = e >> 3, j = cj % taps, c = cj / taps;
          const OutT* t = tile + r8 * LD + c * taps + j;
          uint4 o;
          o.x = (uint32_t)t[0] | ((uint32_t)t[LD] << 16);
          o.y = (uint32_t)t[2 * LD] | ((uint32_t)t[3 * LD] << 16);
          o.z = (uint32_t)t[4 * LD] | ((uint32_t)t[5 * LD] << 16);
          o.w = (uint32_t)t[6 * LD] | ((uint32_t)t[7 * LD] << 16);
          *reinterpret_cast<uint4*>(wb + ((int64_t)(c0 + c) * taps + (taps - 1 - j)) * Cout + o0 + r8) = o;
        }
      }
      return;
    }
  }
  for (int e = threadIdx.x; e < no * run; e += 256) {
    const int r = e / run, q = e - r * run;
    const float v = w[(int64_t)(o0 + r) * Q + (int64_t)c0 * taps + q];
    if constexpr (sizeof(OutT) == 2) tile[r * LD + q] = to_bf16(v);
    else tile[r * LD + q] = v;
  }
  __syncthreads();
  if (wf) {  // wf[o, j*Cin + c]
    for (int e = threadIdx.x; e < no * taps * CT; e += 256) {
      const int c = e % CT, rj = e / CT, j = rj % taps, r = rj / taps;
      if (c < nc) wf[(int64_t)(o0 + r) * Q + (int64_t)j * Cin + c0 + c] = tile[r * LD + c * taps + j];
    }
  }
  if (wb) {  // wb[c*taps + taps-1-j, o]
    for (int e = threadIdx.x; e < nc * taps * 64; e += 256) {
      const int r = e & 63, cj = e >> 6, j = cj % taps, c = cj / taps;
      if (r < no)
        wb[((int64_t)(c0 + c) * taps + (taps - 1 - j)) * Cout + o0 + r] = tile[r * LD + c * taps + j];
    }
  }
}

__global__ void cast_bf16_kernel(const float* x, u16* y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    y[i] = to_bf16(x[i]);
}

__global__ void colsum_partial_bf16(const u16* x, int64_t ldx, int64_t rows, int64_t cols, float* part) {
  const int64_t c = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int ry = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * 256;
  __shared__ float red[4][64];
  float s = 0.f;
  if (c < cols) {
    const int64_t r1 = r0 + 256 < rows ? r0 + 256 : rows;
    for (int64_t r = r0 + ry; r < r1; r += 4) s += bf2f(x[r * ldx + c]);
  }
  red[ry][threadIdx.x & 63] = s;
  __syncthreads();
  if (ry == 0 && c < cols)
    part[(int64_t)blockIdx.y * cols + c] = red[0][threadIdx.x] + red[1][threadIdx.x] +
                                          red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ------------------------------------------------------------------------ launchers
int weight_prep_bf16_launch(const float* w, int64_t c_out, int64_t c_in, int taps, void* wf,
                            void* wb, hipStream_t st) {
  const int64_t total = c_out * c_in * taps;
  unsigned blocks = (unsigned)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  weight_prep_bf16<<<blocks, 256, 0, st>>>(w, (int)c_out, (int)c_in, taps, (u16*)wf, (u16*)wb);
  return launch_status("fs2_conv_weight_prep(bf16)");
}

int colsum_bf16_launch(const void* x, int64_t ldx, int64_t rows, int64_t cols, float* out, int acc,
                       float* ws, hipStream_t st) {
  const int64_t nparts = (rows + 255) / 256;
  dim3 grid((unsigned)((cols + 63) / 64), (unsigned)nparts);
  colsum_partial_bf16<<<grid, 256, 0, st>>>((const u16*)x, ldx, rows, cols, ws);
  return colsum_final_launch(ws, nparts, cols, out, acc, st);
}

}  // namespace fs2

extern "C" int fs2_weight_prep_tile_channels(int dtype) { return dtype == FS2_BF16 ? 32 : 16; }

extern "C" int fs2_weight_prep_batch(int dtype, const int64_t* jobs, int n_jobs, int64_t n_tiles,
                                     void* stream) {
  if (n_jobs <= 0 || n_tiles <= 0) return FS2_OK;
  if (dtype == FS2_BF16)
    fs2::weight_prep_tiles<unsigned short><<<(unsigned)n_tiles, 256, 0, as_stream(stream)>>>(jobs, n_jobs);
  else if (dtype == FS2_F32)
    fs2::weight_prep_tiles<float><<<(unsigned)n_tiles, 256, 0, as_stream(stream)>>>(jobs, n_jobs);
  else {
    fs2::set_error("fs2_weight_prep_batch: dtype %d not built", dtype);
    return FS2_ERR_DTYPE;
  }
  return fs2::launch_status("fs2_weight_prep_batch");
}

extern "C" int fs2_cast_bf16(const float* x, void* y, int64_t n, void* stream) {
  if (n <= 0) return FS2_OK;
  int64_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  fs2::cast_bf16_kernel<<<(unsigned)b, 256, 0, as_stream(stream)>>>(x, (unsigned short*)y, n);
  return fs2::launch_status("fs2_cast_bf16");
}
