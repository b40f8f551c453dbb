// CPU harness over flatnav_amd/csrc/scan_select.hpp (the exhaustive search's key and merge rules), for tests/test_exhaustive_cpu.py:
//   g++ -std=c++17 -O2 -fPIC -shared tests/scan_select_harness.cpp -o libscan_select_harness.so
#include <stdint.h>

#include <vector>

#include "../flatnav_amd/csrc/scan_select.hpp"

using namespace fnv_dev;

extern "C" {

uint64_t ssh_pad() { return SCAN_PAD; }
int ssh_max_k() { return SCAN_MAX_K; }

void ssh_keys(const uint32_t* dist_bits, const uint32_t* nodes, uint64_t n, uint64_t* out) {
  for (uint64_t i = 0; i < n; i++) out[i] = scan_key(dist_bits[i], nodes[i]);
}
void ssh_unkeys(const uint64_t* keys, uint64_t n, uint32_t* dist_bits, uint32_t* nodes) {
  for (uint64_t i = 0; i < n; i++) {
    dist_bits[i] = scan_key_dist_bits(keys[i]);
    nodes[i] = scan_key_node(keys[i]);
  }
}
// out[i] = key a[i] ranks before key b[i]
void ssh_less(const uint64_t* a, const uint64_t* b, uint64_t n, uint8_t* out) {
  for (uint64_t i = 0; i < n; i++) out[i] = scan_key_less(a[i], b[i]) ? 1 : 0;
}
uint32_t ssh_lower_bound(const uint64_t* list, uint32_t n, uint64_t key) { return scan_lower_bound(list, n, key); }
uint32_t ssh_upper_bound(const uint64_t* list, uint32_t n, uint64_t key) { return scan_upper_bound(list, n, key); }

// out[0, K) = the K first of two sorted, padded lists.  `written` (K entries): how often each position was written.
void ssh_merge(const uint64_t* a, const uint64_t* b, uint32_t K, uint64_t* out, uint32_t* written) {
  for (uint32_t i = 0; i < K; i++) written[i] = 0;
  for (uint32_t i = 0; i < K; i++) {
    const uint32_t pa = scan_merge_pos_a(i, a[i], b, K), pb = scan_merge_pos_b(i, b[i], a, K);
    if (pa < K) {
      out[pa] = a[i];
      written[pa]++;
    }
    if (pb < K) {
      out[pb] = b[i];
      written[pb]++;
    }
  }
}

// lists: [S][K] sorted, padded; folded left to right as the merge kernel folds a query's segments.
void ssh_merge_many(const uint64_t* lists, uint32_t S, uint32_t K, uint64_t* out) {
  std::vector<uint64_t> a(lists, lists + K), b(K);
  for (uint32_t s = 1; s < S; s++) {
    scan_merge_lists(a.data(), lists + (uint64_t)s * K, b.data(), K);
    a.swap(b);
  }
  for (uint32_t i = 0; i < K; i++) out[i] = a[i];
}

}  // extern "C"
