// scan_matrix_block_harness.cpp -- test infrastructure (tests/test_scan_matrix_block_plan.py compiles it with g++ and loads it
// with ctypes): scan_matrix_shape of flatnav_amd/csrc/launch_plan.hpp with "scan_matrix_block", on the CPU.
#include "../flatnav_amd/csrc/launch_plan.hpp"

using namespace fnv_dev;

// c = {dtype, dim, capacity, num_cus, scan_segment_rows, scan_matrix, scan_matrix_float, scan_matrix_float32, scan_matrix_grouped,
//      scan_matrix_block, nq, K, live, filter_rows, range, listed}
static PlanInputs smb_inputs(const int64_t* c) {
  PlanInputs ix;
  ix.dtype = (int)c[0], ix.dim = (uint32_t)c[1], ix.capacity = (uint64_t)c[2], ix.num_cus = (int)c[3];
  ix.scan_segment_rows = c[4], ix.scan_matrix = c[5], ix.scan_matrix_float = c[6], ix.scan_matrix_float32 = c[7];
  ix.scan_matrix_grouped = c[8], ix.scan_matrix_block = c[9];
  const RowLayout lay = row_layout(ix.dim, ix.dtype, ix.capacity);
  ix.row_bytes = lay.row_bytes, ix.tail_bytes = lay.tail_bytes;
  return ix;
}
// out = {on, tile, tiles, segments, lds, block, waves, wave_subtiles}
extern "C" void smb_shape(const int64_t* c, int64_t* out) {
  const PlanInputs ix = smb_inputs(c);
  const ScanMatrixShape s = scan_matrix_shape(&ix, row_geometry(&ix), (uint64_t)c[10], (int)c[11], (uint64_t)c[12], (uint64_t)c[13], c[14] != 0, c[15] != 0);
  for (int64_t v : {(int64_t)s.on, (int64_t)s.tile, (int64_t)s.tiles, (int64_t)s.segments, (int64_t)s.lds, (int64_t)s.block, (int64_t)s.waves,
                    (int64_t)s.wave_subtiles})
    *out++ = v;
}
// The LDS of the same call's VECTOR scan (scan_shape, which scan_device_impl asks first: beyond kScanMaxLds it refuses the call;
// tests/exhaustive_sequences.py).
extern "C" int64_t smb_vector_lds(const int64_t* c) {
  const PlanInputs ix = smb_inputs(c);
  return (int64_t)scan_shape(&ix, row_geometry(&ix), (uint64_t)c[10], (int)c[11], (uint64_t)c[12], (uint64_t)c[13], c[14] != 0).lds;
}
