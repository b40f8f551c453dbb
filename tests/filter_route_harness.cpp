// filter_route_harness.cpp -- built by tests/test_filter_route_cpu.py with g++ (no HIP): the filter-routing rules of
// flatnav_amd/csrc/scan_select.hpp exactly as the device code compiles them -- the route word of a query from its filter row's
// popcount, and the grouping of the routed queries alone into the scan stage's tiles (the steps of scan.hpp's group_* kernels,
// stated sequentially over the same per-query and per-descriptor functions).
#include "../flatnav_amd/csrc/scan_select.hpp"

using namespace fnv_dev;

extern "C" {

uint32_t frh_route_by_count(uint32_t allowed_nodes, uint64_t scan_max) { return route_by_count(allowed_nodes, scan_max); }
uint32_t frh_route_graph() { return ROUTE_GRAPH; }
uint32_t frh_route_scan() { return ROUTE_SCAN; }
uint32_t frh_route_overflow() { return ROUTE_OVERFLOW; }
uint32_t frh_no_row() { return GROUP_NO_ROW; }
uint64_t frh_tile_bound(uint64_t nq, uint64_t rows, uint32_t tile) { return group_tile_bound(nq, rows, tile); }

// route[q] of every query before the search kernel runs; query_filter may be null (the single-filter call)
void frh_route_at_launch(const int32_t* query_filter, uint32_t nq, uint32_t n_filters, const uint32_t* row_count, uint64_t scan_max,
                         uint32_t* route) {
  for (uint32_t q = 0; q < nq; q++) route[q] = route_at_launch(query_filter, q, n_filters, row_count, scan_max);
}

// The scan stage's grouping of the queries whose route word is set: query_row [nq], perm [nq] (0xFFFFFFFF where no query was
// put), tiles [bound][3] = {first, count, row}.  Returns the number of real tiles.
uint32_t frh_group_routed(const int32_t* query_filter, const uint32_t* route, uint32_t nq, uint32_t n_filters, uint32_t tile,
                          uint32_t* query_row, uint32_t* perm, uint32_t* tiles, uint32_t bound) {
  const uint32_t rows = n_filters + 2u;
  uint32_t* counts = new uint32_t[rows]();
  uint32_t* cursor = new uint32_t[rows]();
  uint32_t* slot_start = new uint32_t[rows + 1];
  uint32_t* tile_start = new uint32_t[rows + 1];
  for (uint32_t q = 0; q < nq; q++) {  // group_rows_routed_kernel
    query_row[q] = routed_group_row(query_filter, q, n_filters, route);
    if (query_row[q] != GROUP_NO_ROW) counts[query_row[q]]++;
  }
  slot_start[0] = tile_start[0] = 0;  // group_prefix_kernel
  for (uint32_t g = 0; g < rows; g++) {
    slot_start[g + 1] = slot_start[g] + counts[g];
    tile_start[g + 1] = tile_start[g] + (counts[g] + tile - 1) / tile;
  }
  for (uint32_t q = 0; q < nq; q++) perm[q] = 0xFFFFFFFFu;
  for (uint32_t q = 0; q < nq; q++) {  // group_scatter_kernel
    const uint32_t r = query_row[q];
    if (r == GROUP_NO_ROW) continue;
    perm[slot_start[r] + cursor[r]++] = q;
  }
  GroupTile* out = reinterpret_cast<GroupTile*>(tiles);
  for (uint32_t d = 0; d < bound; d++) out[d] = group_tile_at(d, slot_start, tile_start, rows, tile);  // group_tiles_kernel
  const uint32_t real = tile_start[rows];
  delete[] counts;
  delete[] cursor;
  delete[] slot_start;
  delete[] tile_start;
  return real;
}

}  // extern "C"
