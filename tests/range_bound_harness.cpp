// Harness of tests/test_range_search_cpu.py: the range search's key bound (flatnav_amd/csrc/scan_select.hpp), as it is.
#include "../flatnav_amd/csrc/scan_select.hpp"

using namespace fnv_dev;

extern "C" {
// in_range[i * nd + j] = whether a candidate with distance bits dist[j] and node id node[j] lies within radius bits radius[i]
void rbh_in_range(const uint32_t* radius, uint64_t nr, const uint32_t* dist, const uint32_t* node, uint64_t nd, uint8_t* in_range) {
  for (uint64_t i = 0; i < nr; i++) {
    const uint64_t bound = scan_range_bound(radius[i]);
    for (uint64_t j = 0; j < nd; j++) in_range[i * nd + j] = scan_in_range(scan_key(dist[j], node[j]), bound) ? 1 : 0;
  }
}
int rbh_radius_valid(int64_t value) { return scan_radius_valid(value) ? 1 : 0; }
}
