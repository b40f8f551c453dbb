// scan_matrix_grouped_harness.cpp -- test infrastructure (tests/test_scan_matrix_grouped_plan.py compiles it with g++ and loads it
// with ctypes): scan_matrix_shape of flatnav_amd/csrc/launch_plan.hpp for a grouped call, on the CPU.
#include "../flatnav_amd/csrc/launch_plan.hpp"

using namespace fnv_dev;

// c = {dtype, dim, capacity, num_cus, scan_segment_rows, scan_matrix, scan_matrix_float, scan_matrix_float32, scan_matrix_grouped,
//      nq, K, live, filter_rows (-1: the argument is left out)}
// out = {on, tile, tiles, segments, lds, group_tile_bound(nq, filter_rows, tile), MATRIX_QUEUE_IDS * 4, kScanMaxLds}
extern "C" void smg_shape(const int64_t* c, int64_t* out) {
  PlanInputs ix;
  ix.dtype = (int)c[0], ix.dim = (uint32_t)c[1], ix.capacity = (uint64_t)c[2], ix.num_cus = (int)c[3];
  ix.scan_segment_rows = c[4], ix.scan_matrix = c[5], ix.scan_matrix_float = c[6], ix.scan_matrix_float32 = c[7], ix.scan_matrix_grouped = c[8];
  const RowLayout lay = row_layout(ix.dim, ix.dtype, ix.capacity);
  ix.row_bytes = lay.row_bytes, ix.tail_bytes = lay.tail_bytes;
  const RowGeometry g = row_geometry(&ix);
  const uint64_t nq = (uint64_t)c[9], live = (uint64_t)c[11];
  const ScanMatrixShape s = c[12] < 0 ? scan_matrix_shape(&ix, g, nq, (int)c[10], live) : scan_matrix_shape(&ix, g, nq, (int)c[10], live, (uint64_t)c[12]);
  for (int64_t v : {(int64_t)s.on, (int64_t)s.tile, (int64_t)s.tiles, (int64_t)s.segments, (int64_t)s.lds,
                    (int64_t)(s.on && c[12] > 0 ? group_tile_bound(nq, (uint64_t)c[12], s.tile) : 0), (int64_t)MATRIX_QUEUE_IDS * 4, (int64_t)kScanMaxLds})
    *out++ = v;
}
