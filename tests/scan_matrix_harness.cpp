// scan_matrix_harness.cpp -- test infrastructure (tests/test_scan_matrix_plan.py compiles it with g++ and loads it with ctypes):
// scan_matrix_shape of flatnav_amd/csrc/launch_plan.hpp on the CPU.
#include "../flatnav_amd/csrc/launch_plan.hpp"

using namespace fnv_dev;

// c = {dtype, dim, capacity, num_cus, scan_segment_rows, scan_matrix, nq, K, live}
// out = {on, tile, tiles, segments, lds, block, partial_bytes}
extern "C" void smh_shape(const int64_t* c, int64_t* out) {
  PlanInputs ix;
  ix.dtype = (int)c[0], ix.dim = (uint32_t)c[1], ix.capacity = (uint64_t)c[2], ix.num_cus = (int)c[3];
  ix.scan_segment_rows = c[4], ix.scan_matrix = c[5];
  const RowLayout lay = row_layout(ix.dim, ix.dtype, ix.capacity);
  ix.row_bytes = lay.row_bytes, ix.tail_bytes = lay.tail_bytes;
  const ScanMatrixShape s = scan_matrix_shape(&ix, row_geometry(&ix), (uint64_t)c[6], (int)c[7], (uint64_t)c[8]);
  for (int64_t v : {(int64_t)s.on, (int64_t)s.tile, (int64_t)s.tiles, (int64_t)s.segments, (int64_t)s.lds, (int64_t)s.block,
                    (int64_t)scan_partial_bytes((uint64_t)c[6], s, (int)c[7])})
    *out++ = v;
}
