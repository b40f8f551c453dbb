// scan_select.hpp -- part of the gfx950 search engine, free of HIP (device code includes it through scan.hpp, the host code
// through kernel_table.h, tests/scan_select_harness.cpp as it is).  The SELECTION rules of the exhaustive search
// (fnv_search_batch_exhaustive): how a (distance, node id) pair becomes one sortable key, and how two sorted partial lists of K
// keys become the K smallest of their union -- each stated here once, used by the scan kernel's per-query lists, by the merge
// kernel and by the CPU test.
//
// Order.  Ascending by (distance, node id); a NaN distance ranks after every number, +inf included; among NaNs by node id.  That
// is a TOTAL order on distinct node ids, so a result depends neither on how rows were tiled into segments nor on which lane
// saw a row first.  (The graph search orders equal distances as libstdc++'s heaps leave them; this order is not that one.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FNV_SCAN_HD __host__ __device__
#else
#define FNV_SCAN_HD
#endif

namespace fnv_dev {

constexpr int SCAN_MAX_K = 1024;          // the widest result list of an exhaustive search
constexpr uint64_t SCAN_PAD = ~0ull;      // "no entry": sorts after every real key (a real node id is never 0xFFFFFFFF)
constexpr uint32_t SCAN_NAN_ORD = 0xFFFFFFFFu;

// float32 bits -> an unsigned integer that orders like the number; every NaN -> SCAN_NAN_ORD (above +inf); -0 and +0 coincide.
FNV_SCAN_HD inline uint32_t scan_dist_ord(uint32_t bits) {
  const uint32_t mag = bits & 0x7FFFFFFFu;
  if (mag > 0x7F800000u) return SCAN_NAN_ORD;
  if (mag == 0u) return 0x80000000u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
// ... and back: the distance's bits (a NaN comes back as the quiet NaN 0x7FC00000, a zero as +0).
FNV_SCAN_HD inline uint32_t scan_ord_dist(uint32_t ord) {
  if (ord == SCAN_NAN_ORD) return 0x7FC00000u;
  return (ord & 0x80000000u) ? (ord & 0x7FFFFFFFu) : ~ord;
}
FNV_SCAN_HD inline uint64_t scan_key(uint32_t dist_bits, uint32_t node) {
  return ((uint64_t)scan_dist_ord(dist_bits) << 32) | node;
}
FNV_SCAN_HD inline uint32_t scan_key_dist_bits(uint64_t key) { return scan_ord_dist((uint32_t)(key >> 32)); }
FNV_SCAN_HD inline uint32_t scan_key_node(uint64_t key) { return (uint32_t)key; }
// a ranks before b
FNV_SCAN_HD inline bool scan_key_less(uint64_t a, uint64_t b) { return a < b; }

// Entries of the sorted list[0, n) that rank before `key` / that do not rank after it.
FNV_SCAN_HD inline uint32_t scan_lower_bound(const uint64_t* list, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (scan_key_less(list[mid], key)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
FNV_SCAN_HD inline uint32_t scan_upper_bound(const uint64_t* list, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (!scan_key_less(key, list[mid])) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Merge of two sorted lists a[0, K), b[0, K) (each padded with SCAN_PAD), by RANK: a[i] lands at i + (entries of b before it),
// b[j] at j + (entries of a not after it).  Real keys are distinct (a node is in one list), equal keys are pads, and the two
// rules send equal keys of a before those of b: every position below K is written exactly once, by whoever holds it -- one
// independent binary search per entry, which is what lets 64 lanes do a merge without talking to each other.
FNV_SCAN_HD inline uint32_t scan_merge_pos_a(uint32_t i, uint64_t key, const uint64_t* b, uint32_t K) {
  return i + scan_lower_bound(b, K, key);
}
FNV_SCAN_HD inline uint32_t scan_merge_pos_b(uint32_t j, uint64_t key, const uint64_t* a, uint32_t K) {
  return j + scan_upper_bound(a, K, key);
}
// out[0, K) = the K first of a merged with b (out overlaps neither)
inline void scan_merge_lists(const uint64_t* a, const uint64_t* b, uint64_t* out, uint32_t K) {
  for (uint32_t i = 0; i < K; i++) {
    const uint32_t pa = scan_merge_pos_a(i, a[i], b, K), pb = scan_merge_pos_b(i, b[i], a, K);
    if (pa < K) out[pa] = a[i];
    if (pb < K) out[pb] = b[i];
  }
}

// Parameter block of the exhaustive search's kernels (scan.hpp).
struct ScanParams {
  const uint8_t* vectors;      // [capacity][row_bytes]: the table the filtered search kernel reads
  const uint8_t* tails;        // split rows: the side table, else null
  const int32_t* labels;       // null: node ids go out
  const uint8_t* queries;      // [nq][dim] elements
  const uint32_t* cand_ids;    // filtered: the allowed node ids, in any order; null: the candidates are nodes [0, n_live)
  const uint32_t* cand_count;  // filtered: how many (device memory: the host never waits for it)
  uint64_t* partial;           // [nq][segments][K] keys: every (query, segment)'s sorted list
  float* out_dist;             // [nq][K]
  int32_t* out_labels;         // [nq][K]
  int32_t* out_count;          // [nq] or null
  uint64_t* out_ndist;         // [nq] or null
  uint64_t n_live;
  uint32_t nq, dim, row_bytes, nchunks, q_chunks, tail_chunks;
  uint32_t K;
  uint32_t segments;           // row segments: block b scans segment b / tiles for query tile b % tiles
  uint32_t tile_queries;       // queries staged in LDS per block: that many share one load of a row
  uint32_t tiles;              // ceil(nq / tile_queries)
};

// ---- grouped filters (fnv_search_batch_*_grouped): one allowed set per query ---------------------------------------------
// A grouped launch keeps n_filters + 2 node bitmaps ("filter rows"): row f < n_filters is filter f, row n_filters holds every
// live node (query_filter == -1: no filter), row n_filters + 1 is empty (any other value, which only the _device entry points
// can meet: the host entry points refuse it).  So no value of query_filter[q] leads outside the table.
FNV_SCAN_HD inline uint32_t filter_row(int32_t query_filter, uint32_t n_filters) {
  if (query_filter == -1) return n_filters;
  return (uint32_t)query_filter < n_filters ? (uint32_t)query_filter : n_filters + 1u;
}

// ---- filter routing ("filter_scan_max" / "filter_scan_on_overflow"): graph search or scan, per query, inside one call --------
// A filtered graph search keeps one ROUTE WORD per query.  Before the search kernel runs, a query whose filter row allows at
// most `scan_max` live nodes (the row's popcount: a -1 row counts every live node, the empty row 0) is handed to the scan;
// scan_max == 0 turns the rule off, whatever the count.  The search kernel skips such a query, and -- when overflow routing is
// on -- marks a query whose candidates heap outgrew its room instead of failing the launch.  The scan stage that follows
// answers exactly the queries whose word is not ROUTE_GRAPH.
enum : uint32_t { ROUTE_GRAPH = 0u, ROUTE_SCAN = 1u, ROUTE_OVERFLOW = 2u };
FNV_SCAN_HD inline uint32_t route_by_count(uint32_t allowed_nodes, uint64_t scan_max) {
  return scan_max != 0u && (uint64_t)allowed_nodes <= scan_max ? ROUTE_SCAN : ROUTE_GRAPH;
}
// The filter row of query q in a routed launch: a null query_filter is the single-filter call -- a table of one, row 0 for all.
FNV_SCAN_HD inline uint32_t routed_filter_row(const int32_t* query_filter, uint32_t q, uint32_t n_filters) {
  return filter_row(query_filter ? query_filter[q] : 0, n_filters);
}
// ... and its route word before the search kernel runs, from the rows' popcounts.
FNV_SCAN_HD inline uint32_t route_at_launch(const int32_t* query_filter, uint32_t q, uint32_t n_filters, const uint32_t* row_count,
                                            uint64_t scan_max) {
  return route_by_count(row_count[routed_filter_row(query_filter, q, n_filters)], scan_max);
}
// The scan stage groups the routed queries only: what query q puts into query_row (GROUP_NO_ROW: it takes no part, neither in
// the rows' counts nor in the permutation; a real row is at most 2^31).
constexpr uint32_t GROUP_NO_ROW = 0xFFFFFFFFu;
FNV_SCAN_HD inline uint32_t routed_group_row(const int32_t* query_filter, uint32_t q, uint32_t n_filters, const uint32_t* route) {
  return route[q] != ROUTE_GRAPH ? routed_filter_row(query_filter, q, n_filters) : GROUP_NO_ROW;
}

// The grouped scan's tiles.  Queries are permuted so that every filter row's queries are contiguous, and a tile holds at most
// `tile` queries of ONE row: a block then walks one bitmap for all its queries.  How many tiles that takes depends on the data,
//   sum_g ceil(c_g / tile)  <=  ceil(nq / tile) + min(rows, nq)   and never more than nq,
// so the host launches this bound and the descriptors past the real ones have count 0.
struct GroupTile {
  uint32_t first;  // first slot of the permutation
  uint32_t count;  // queries of the tile, at most `tile`; 0: not a tile, its blocks return at once
  uint32_t row;    // the filter row they all use
};
FNV_SCAN_HD inline uint64_t group_tile_bound(uint64_t nq, uint64_t rows, uint32_t tile) {
  const uint64_t b = (nq + tile - 1) / tile + (rows < nq ? rows : nq);
  return b < nq ? b : nq;
}
// Descriptor d from the rows' exclusive prefixes: slot_start[g] = queries of the rows before g, tile_start[g] = tiles of the
// rows before g (both with a last entry [rows] = the total).  One independent binary search per descriptor.
FNV_SCAN_HD inline GroupTile group_tile_at(uint32_t d, const uint32_t* slot_start, const uint32_t* tile_start, uint32_t rows,
                                           uint32_t tile) {
  if (d >= tile_start[rows]) return GroupTile{0u, 0u, 0u};
  uint32_t lo = 0, hi = rows;  // the last g with tile_start[g] <= d (rows without queries share their successor's start)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (tile_start[mid] <= d) lo = mid;
    else hi = mid;
  }
  const uint32_t j = d - tile_start[lo], c = slot_start[lo + 1] - slot_start[lo];
  const uint32_t left = c - j * tile;
  return GroupTile{slot_start[lo] + j * tile, left < tile ? left : tile, lo};
}
// The same layout stated sequentially (the CPU test holds group_tile_at against it): out[0, bound) from the rows' query counts.
// Returns the number of real tiles.
inline uint32_t group_tiles_layout(const uint32_t* counts, uint32_t rows, uint32_t tile, GroupTile* out, uint32_t bound) {
  uint32_t n = 0, slot = 0;
  for (uint32_t g = 0; g < rows; g++) {
    for (uint32_t j = 0; j < counts[g]; j += tile) {
      if (n < bound) out[n] = GroupTile{slot + j, counts[g] - j < tile ? counts[g] - j : tile, g};
      n++;
    }
    slot += counts[g];
  }
  for (uint32_t d = n; d < bound; d++) out[d] = GroupTile{0u, 0u, 0u};
  return n;
}

// The grouped scan reads its candidates from the tile's bitmap row: set bits become node ids in an LDS queue of this many
// entries, scored in batches as they fill (scan.hpp).  256 ids = 1 KB: with a tile budget of 19 KB a block still takes sixteen
// 1280-byte LDS granules, eight blocks per CU as the plain scan; and a queue that holds less than a batch (at most 24 rows)
// plus one 32-node word could not make progress.
constexpr uint32_t SCAN_QUEUE_IDS = 256;

// Parameter block of the grouped scan and its merge: the plain block (cand_ids / cand_count null, tiles = the launched bound)
// and what grouping adds.
struct GroupedScanParams {
  ScanParams s;
  const uint32_t* node_bits;   // [n_filters + 2][row_words]
  const GroupTile* tiles;      // [s.tiles]
  const uint32_t* perm;        // [nq] query indices, contiguous per filter row
  const uint32_t* query_row;   // [nq] filter row of each query
  const uint32_t* row_count;   // [n_filters + 2] nodes set in each row = the candidates of its queries
  uint32_t row_words;          // words per bitmap row: ceil(capacity / 32)
  uint32_t live_words;         // ceil(n_live / 32): the segments cut [0, live_words) in whole words
};

}  // namespace fnv_dev
