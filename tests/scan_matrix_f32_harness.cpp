// scan_matrix_f32_harness.cpp -- test infrastructure (tests/test_scan_matrix_f32_plan.py compiles it with g++ and loads it with
// ctypes): scan_matrix_shape with the three matrix options, and scan_margin_f32 of flatnav_amd/csrc/scan_select.hpp, on the CPU.
#include "../flatnav_amd/csrc/launch_plan.hpp"

using namespace fnv_dev;

// c = {dtype, dim, capacity, num_cus, scan_segment_rows, scan_matrix, scan_matrix_float, scan_matrix_float32, nq, K, live}
// out = {on, float_rows, float32_rows, group_lanes, tile, tiles, segments, lds, block}
extern "C" void smf32_shape(const int64_t* c, int64_t* out) {
  PlanInputs ix;
  ix.dtype = (int)c[0], ix.dim = (uint32_t)c[1], ix.capacity = (uint64_t)c[2], ix.num_cus = (int)c[3];
  ix.scan_segment_rows = c[4], ix.scan_matrix = c[5], ix.scan_matrix_float = c[6], ix.scan_matrix_float32 = c[7];
  const RowLayout lay = row_layout(ix.dim, ix.dtype, ix.capacity);
  ix.row_bytes = lay.row_bytes, ix.tail_bytes = lay.tail_bytes;
  const ScanMatrixShape s = scan_matrix_shape(&ix, row_geometry(&ix), (uint64_t)c[8], (int)c[9], (uint64_t)c[10]);
  for (int64_t v : {(int64_t)s.on, (int64_t)s.float_rows, (int64_t)s.float32_rows, (int64_t)s.group_lanes, (int64_t)s.tile, (int64_t)s.tiles,
                    (int64_t)s.segments, (int64_t)s.lds, (int64_t)s.block})
    *out++ = v;
}

extern "C" void smf32_margin(uint32_t P, int ip, const float* rn, const float* qn, uint64_t n, float* out) {
  for (uint64_t i = 0; i < n; i++) out[i] = scan_margin_f32(P, rn[i], qn[i], ip != 0);
}
