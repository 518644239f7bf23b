// LDS-DMA staging, transposed LDS reads and the hand-counted waits that go with them: the one
// copy shared by the conv / GEMM kernels (gemm_glds, gemm_tapreg, wgrad_splitk, wgrad, wgrad_band),
// attention_bf16, gemm_bf16 and resblock.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace fs2 {

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// zero source for out-of-range 16-B chunks of the LDS-DMA stagers.  The build has no
// relocatable device code, so every translation unit that stages from it holds its own copy.
static __device__ __attribute__((aligned(128))) uint4 g_zero_line[8];

// bf16 -> fp32 (the other direction is to_bf16, common.hpp: round to nearest even)
FS2_DEV float bf2f(u16 v) { return __uint_as_float(((uint32_t)v) << 16); }

// Are rows [r0, r1) all padding (t >= lens[b] for r = b*T + t)?  Scalar, block-uniform.
FS2_DEV bool rows_all_padding(const int64_t* lens, int64_t T, int64_t r0, int64_t r1) {
  int64_t s = r0 / T;
  if (r0 - s * T < lens[s]) return false;
  for (++s; s * T < r1; ++s)
    if (lens[s] > 0) return false;
  return true;
}

// fn(integral_constant<0>), ..., fn(integral_constant<N - 1>), in order
template <int N, typename Fn>
FS2_DEV void static_for(Fn&& fn) {
  if constexpr (N > 0) {
    static_for<N - 1>(fn);
    fn(std::integral_constant<int, N - 1>{});
  }
}

// global_load_lds_dwordx4: the wave's 64 x 16 B land contiguously at lds_wave_base (the
// buffer-descriptor forms, glds16_buf / glds4_buf, are in common.hpp)
FS2_DEV void glds16(const void* src, u16* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ds_read_b64_tr_b16 as inline asm.  The builtin's memory operand carries no alias scope, so
// hipcc's wait-count pass makes every such read wait for ALL LDS-DMA in flight (vmcnt(0)):
// issued after the next k-tile's DMA it drained the prefetch every k-tile, serialising the
// weight-gradient loops on one global round trip.  The asm read is invisible to that pass:
// the caller orders it after the DMA of the tile it reads (counted vmcnt + barrier, as the
// k-loops do) and waits for its result with lgkm_wait<N>() before use.
FS2_DEV s16x4 ds_tr16(const u16* p) {
  s16x4 r;
  const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) u16*)p;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(a));
  return r;
}
// ... at a per-lane base + a compile-time byte offset (the instruction's 16-bit immediate):
// every fragment address of a main loop is one of a few per-lane bases
template <int OFF>
FS2_DEV s16x4 ds_tr16_at(uint32_t base) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(base), "n"(OFF));
  return r;
}
// the two 4-k halves of a fragment as one MFMA operand
FS2_DEV bf16x8 tr16_cat(s16x4 lo, s16x4 hi) {
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// s_waitcnt lgkmcnt(N), then a scheduling fence: register-only MFMAs must not be hoisted
// above the wait (the asm reads' results are unknown to the compiler)
template <int N>
FS2_DEV void lgkm_wait() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// s_waitcnt lgkmcnt(0) with vmcnt / expcnt left at their maxima (gfx9 simm16 encoding), for
// __builtin_amdgcn_s_waitcnt: unlike inline asm, the compiler's wait-count pass sees it.
constexpr int kLgkm0 = 0xC07F;

// Wait until at most n (0..8, wave-uniform) vector-memory instructions are in flight.
FS2_DEV void vm_wait_n(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
  }
}

// Wait until at most `ahead` (<= 3) tiles of PER LDS-DMA instructions each are still in flight.
template <int PER>
FS2_DEV void vm_wait_tiles(int ahead) {
  switch (ahead) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PER) : "memory"); break;
  }
}

// The k-loop.  STAGES == 1: load; vmcnt(0); barrier; MFMA; barrier.  STAGES >= 2: a ring of
// LDS stages with STAGES-1 tiles issued ahead; per tile: counted vmcnt (the tile landed, later
// ones may stay in flight), ONE raw barrier (the tile is visible to every wave AND every wave
// has finished the previous tile, whose slot the refill below overwrites), refill, MFMA.
template <int STAGES, int PER, typename Issue, typename Compute>
FS2_DEV void kloop(int nk, Issue&& issue, Compute&& compute) {
  if constexpr (STAGES == 1) {
    for (int kt = 0; kt < nk; ++kt) {
      issue(kt, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      compute(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  } else {
    for (int t = 0; t < STAGES - 1 && t < nk; ++t) issue(t, t);
    for (int kt = 0; kt < nk; ++kt) {
      const int ahead = nk - 1 - kt < STAGES - 2 ? nk - 1 - kt : STAGES - 2;
      vm_wait_tiles<PER>(ahead);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + STAGES - 1 < nk) issue(kt + STAGES - 1, (kt + STAGES - 1) % STAGES);
      compute(kt % STAGES);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
}

// Workgroup barrier of the epilogues: LDS writes retired (lgkmcnt(0)), then a raw s_barrier.
// __syncthreads() would also wait vmcnt(0); at the end of the kernels no DMA is in flight and
// the two are the same.  (The epilogues share no global memory between threads.)
FS2_DEV void epi_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

}  // namespace fs2
