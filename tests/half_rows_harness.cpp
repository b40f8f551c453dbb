// half_rows_harness.cpp -- the half-width mirror's rules (flatnav_amd/csrc/half_rows.hpp) on the CPU, for tests/test_half_rows.py:
// compiled with g++ as a shared library (ctypes), and once as a stand-alone program (-DHRH_MAIN, with the host sanitizers).
//
// Besides thin wrappers of the header it exports the plain-C++ EMULATION of what the 64 lanes of a wave compute for one vector
// (csrc/distance.hpp), which lives in tests/distance_model_harness.cpp: the float32 FULL path of batch_dists with Dist<float>,
// and the mirror path with Dist<f32h> reading 16-byte units -- each lane's chunks in its order, std::fmaf where the kernels use
// fused multiply-adds, then the pairing of group_sum.  Compile with -ffp-contract=off: nothing but the written fmaf may fuse.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../flatnav_amd/csrc/half_rows.hpp"
#include "../flatnav_amd/csrc/launch_plan.hpp"
#include "distance_model_harness.cpp"  // hrh_dist_f32, hrh_dist_half: the lane-by-lane emulations

using namespace fnv_dev;

using dm::as_float;

extern "C" {

int hrh_eligible(int dtype, uint32_t dim, uint64_t capacity) {
  PlanInputs ix;
  ix.dtype = dtype;
  ix.dim = dim;
  ix.capacity = capacity;
  const RowLayout lay = row_layout(dim, dtype, capacity);
  ix.row_bytes = lay.row_bytes;
  ix.tail_bytes = lay.tail_bytes;
  return half_rows_eligible(dtype, row_geometry(&ix)) ? 1 : 0;
}
int hrh_eligible_cfg(int dtype, int cfg, int full, uint32_t tail_chunks) { return half_rows_eligible(dtype, cfg, full != 0, tail_chunks) ? 1 : 0; }
int hrh_num_cfgs() { return kNumCfgs; }
void hrh_cfg(int cfg, int* G, int* CU) {
  *G = kCfgs[cfg].G;
  *CU = kCfgs[cfg].CU;
}
void hrh_unit_map(uint32_t nchunks, uint32_t G, uint32_t CU, uint32_t* unit, uint32_t* half) {
  for (uint32_t c = 0; c < nchunks; c++) {
    const HalfUnit u = half_unit_of_chunk(c, G, CU);
    unit[c] = u.unit;
    half[c] = u.half;
  }
}
uint32_t hrh_first_chunk_of_unit(uint32_t u, uint32_t G, uint32_t CU) { return half_first_chunk_of_unit(u, G, CU); }
void hrh_round_trip(const uint32_t* bits, uint64_t n, uint32_t* back, uint8_t* lossless) {
  for (uint64_t i = 0; i < n; i++) {
    back[i] = half_bits_widen(half_bits_trunc(bits[i]));
    lossless[i] = half_lossless(bits[i]) ? 1 : 0;
  }
}
int hrh_convert_row(const uint32_t* row, uint16_t* mirror, uint32_t nchunks, uint32_t G, uint32_t CU) {
  return half_convert_row(row, mirror, nchunks, G, CU) ? 1 : 0;
}

}  // extern "C"

#ifdef HRH_MAIN
// Stand-alone run (built with -fsanitize=address,undefined by the test): every eligible configuration, one and two spans --
// the map is a bijection onto the mirror row, conversion stays inside it, and both emulations agree bit for bit.
int main() {
  uint32_t rng = 12345u;
  auto next = [&]() { return rng = rng * 1664525u + 1013904223u; };
  for (int cfg = 0; cfg < kNumCfgs; cfg++) {
    if (!half_rows_eligible(FNV_DTYPE_FLOAT32, cfg, true, 0)) continue;
    const int G = kCfgs[cfg].G, CU = kCfgs[cfg].CU;
    for (uint32_t spans = 1; spans <= 2; spans++) {
      const uint32_t nchunks = spans * G * CU;
      std::vector<int> seen(nchunks, 0);
      for (uint32_t c = 0; c < nchunks; c++) {
        const HalfUnit u = half_unit_of_chunk(c, G, CU);
        if (u.unit >= nchunks / 2 || u.half > 1 || seen[u.unit * 2 + u.half]++) return 1;
        if (half_first_chunk_of_unit(u.unit, G, CU) + u.half * G != c) return 2;
      }
      std::vector<uint32_t> row(nchunks * 4);
      std::vector<float> rowf(nchunks * 4), q(nchunks * 4);
      for (uint32_t i = 0; i < nchunks * 4; i++) {
        row[i] = half_bits_widen((uint16_t)(next() >> 16) & 0xBBFFu);  // finite binary16 values
        rowf[i] = as_float(row[i]);
        q[i] = (float)(int32_t)next() / 1.7e9f;
      }
      std::vector<uint16_t> mirror(nchunks * 4);
      if (!half_convert_row(row.data(), mirror.data(), nchunks, G, CU)) return 3;
      for (int metric = 0; metric < 2; metric++) {
        const float a = hrh_dist_f32(q.data(), rowf.data(), nchunks, G, CU, metric);
        const float b = hrh_dist_half(q.data(), mirror.data(), nchunks, G, CU, metric, 0);
        if (memcmp(&a, &b, 4) != 0 || a != a) return 4;
      }
    }
  }
  printf("half_rows_harness OK\n");
  return 0;
}
#endif
