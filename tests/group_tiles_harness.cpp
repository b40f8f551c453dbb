// CPU harness over the grouping rules of flatnav_amd/csrc/scan_select.hpp (grouped filters: the row of a query_filter value,
// the tile bound, the tile descriptors), for tests/test_grouped_filters_cpu.py:
//   g++ -std=c++17 -O2 -fPIC -shared tests/group_tiles_harness.cpp -o libgroup_tiles_harness.so
// and, with a main of its own that runs the same rules over random groupings (for a sanitizer build):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DGROUP_TILES_MAIN tests/group_tiles_harness.cpp -o group_tiles_check
#include <stdint.h>

#include <vector>

#include "../flatnav_amd/csrc/scan_select.hpp"

using namespace fnv_dev;

extern "C" {

uint32_t gth_filter_row(int32_t value, uint32_t n_filters) { return filter_row(value, n_filters); }
uint64_t gth_tile_bound(uint64_t nq, uint64_t rows, uint32_t tile) { return group_tile_bound(nq, rows, tile); }
uint32_t gth_queue_ids() { return SCAN_QUEUE_IDS; }

// The sequential layout: out[bound][3] = (first, count, row).  Returns the real tile count.
uint32_t gth_layout(const uint32_t* counts, uint32_t rows, uint32_t tile, uint32_t* out, uint32_t bound) {
  std::vector<GroupTile> t(bound);
  const uint32_t n = group_tiles_layout(counts, rows, tile, t.data(), bound);
  for (uint32_t d = 0; d < bound; d++) {
    out[3 * d] = t[d].first;
    out[3 * d + 1] = t[d].count;
    out[3 * d + 2] = t[d].row;
  }
  return n;
}

// What the device does: the two exclusive prefixes, then one independent group_tile_at per descriptor.
void gth_by_search(const uint32_t* counts, uint32_t rows, uint32_t tile, uint32_t* out, uint32_t bound) {
  std::vector<uint32_t> slot_start(rows + 1, 0), tile_start(rows + 1, 0);
  for (uint32_t g = 0; g < rows; g++) {
    slot_start[g + 1] = slot_start[g] + counts[g];
    tile_start[g + 1] = tile_start[g] + (counts[g] + tile - 1) / tile;
  }
  for (uint32_t d = 0; d < bound; d++) {
    const GroupTile t = group_tile_at(d, slot_start.data(), tile_start.data(), rows, tile);
    out[3 * d] = t.first;
    out[3 * d + 1] = t.count;
    out[3 * d + 2] = t.row;
  }
}

}  // extern "C"

#ifdef GROUP_TILES_MAIN
#include <stdio.h>

int main() {
  uint32_t rng = 12345u;
  auto next = [&]() { return rng = rng * 1664525u + 1013904223u; };
  const uint32_t tiles_of[] = {1, 2, 31, 32};
  for (int round = 0; round < 2000; round++) {
    const uint32_t rows = 2 + next() % 40, tile = tiles_of[next() % 4];
    std::vector<uint32_t> counts(rows);
    uint64_t nq = 0;
    for (uint32_t g = 0; g < rows; g++) nq += counts[g] = (next() % 3 == 0) ? 0 : next() % 100;
    if (nq == 0) nq = counts[0] = 1;
    const uint32_t bound = (uint32_t)group_tile_bound(nq, rows, tile);
    std::vector<uint32_t> a(3 * (size_t)bound), b(3 * (size_t)bound);
    const uint32_t n = gth_layout(counts.data(), rows, tile, a.data(), bound);
    gth_by_search(counts.data(), rows, tile, b.data(), bound);
    if (n > bound || a != b) {
      printf("round %d: %u tiles, bound %u, layouts %s\n", round, n, bound, a == b ? "agree" : "differ");
      return 1;
    }
    std::vector<uint32_t> seen(nq, 0);
    for (uint32_t d = 0; d < bound; d++)
      for (uint32_t i = 0; i < a[3 * d + 1]; i++) seen[a[3 * d] + i]++;
    for (uint64_t q = 0; q < nq; q++)
      if (seen[q] != 1) return 2;
  }
  for (int32_t v : {-1, 0, 4, 5, -2, -7, INT32_MAX, INT32_MIN})
    if (gth_filter_row(v, 5) != (v == -1 ? 5u : (v >= 0 && v < 5) ? (uint32_t)v : 6u)) return 3;
  printf("group tiles: ok\n");
  return 0;
}
#endif
