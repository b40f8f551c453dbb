// search_params.h -- part of the gfx950 search engine (device code: included by every kernel translation unit and, through
// kernel_table.h, by the host units).  What the kernels need on top of search_types.h: the load-pipelining knobs and the
// scalar-register helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <limits>

#include <flatnav/util/StlExact.h>
#include "../../include/flatnav_hip.h"
#include "search_types.h"
namespace fnv_dev {

// Passes (vectors per lane group) whose loads are in flight together.  3 keeps the kernel at 124-128 VGPRs = 4 waves
// per SIMD (16 per CU); 4 needs 148 VGPRs (12 per CU) and measured 2-14 % slower on every configuration tried.
#ifndef FNV_PU
#define FNV_PU 3
#endif
constexpr int PU_DEFAULT = FNV_PU;  // vector "passes" whose loads are issued back to back before any use
// Rows of a whole number of 192-chunk spans (768-d, 1536-d float32 ...) run with G = 64, CU = 3 -- every lane loads
// exactly its three chunks, no clamping -- and four vectors in flight: the same 12 loads per lane as PU_DEFAULT x 4.
// Round 3 experiment (gpurun_out/r3_run11): rows of 3 KB and more (G = 64) keep so few queries resident (LDS: 8-10 per CU at
// 768-d) that half the register file is idle; compiling those instantiations for two waves per SIMD with 6 or 8 passes
// (18-24 loads per lane in flight, what a pure gather of 3 KB rows needs to reach its ceiling) gained nothing -- 85.7 k ->
// 86.0 k / 84.6 k queries/s at 3M x 768, ef=800, and cost a resident query at ef=200: that kernel's hop is paced by the
// on-chip work between two gathers (a 13-chunk LDS merge, the visited probe), not by bytes in flight.  Defaults unchanged;
// the knobs stay for the next look.  Which vectors are in flight together never changes a distance.
#ifndef FNV_PU_64_3
#define FNV_PU_64_3 4
#endif
#ifndef FNV_PU_64_4
#define FNV_PU_64_4 3
#endif
#ifndef FNV_WAVES_G64
#define FNV_WAVES_G64 4
#endif
template <int G, int CU>
constexpr int passes() {
  return (G == 64 && CU == 3) ? FNV_PU_64_3 : (G == 64 && CU == 4) ? FNV_PU_64_4 : PU_DEFAULT;
}
constexpr int passes_of(int G, int CU) { return (G == 64 && CU == 3) ? FNV_PU_64_3 : (G == 64 && CU == 4) ? FNV_PU_64_4 : PU_DEFAULT; }
template <int G>
constexpr int waves_per_simd(int deflt) {
  return G == 64 ? FNV_WAVES_G64 : deflt;
}
#ifndef FNV_MIN_WAVES_PER_SIMD
#define FNV_MIN_WAVES_PER_SIMD 4  // __launch_bounds__ 2nd argument: register budget 512/4 = 128 per lane
#endif

// Broadcast of lane 0's value into a scalar register ("this value is wave-uniform").
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float rfl(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// Register discipline.  The parameter block is ~330 bytes = 80+ scalar registers if every field stays live, and the
// search kernels are persistent (one loop over many queries), so the compiler would keep them all live and spill.
// Fields that are needed once per query or in rare branches are therefore NOT read from the by-value copy but
// re-loaded from the kernel-argument segment at the point of use (scalar loads that hit the scalar cache);
// the empty asm makes the pointer opaque so that the loads are not hoisted back to the kernel entry.
// The block must be the kernel's first (and only) argument.
typedef const __attribute__((address_space(4))) SearchParams* ColdArgs;
__device__ __forceinline__ ColdArgs cold_args() {
  ColdArgs k = (ColdArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

}  // namespace fnv_dev
