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
#include <math.h>
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

// ---- range search (option "scan_radius"): the K nearest among the candidates within distance r, and how many there were ------
// The radius as a bound on the key: the largest key any (d <= r, node id) pair can have, so that
//     a pair is IN RANGE  iff  !scan_key_less(scan_range_bound(r), its key)
// in every engine -- the order the selection already uses decides, not a float compare of its own.  It follows that order:
// a NaN distance (SCAN_NAN_ORD, above +inf's) is in no range, r = +inf admits every number, -0 and +0 are one radius and one
// distance, and an inner-product radius may be negative.  A NaN radius is no radius: fnv_set_option refuses it, and here it
// gives a bound below every key.  A list entry must beat  min(list[K - 1], bound + 1):  it is in range AND before the K-th.
constexpr int64_t SCAN_RADIUS_OFF = -1;  // the option's "no radius" (any negative value); 0 .. 2^32 - 1: the radius's float32 bits
FNV_SCAN_HD inline uint64_t scan_range_bound(uint32_t radius_bits) {
  const uint32_t ord = scan_dist_ord(radius_bits);
  if (ord == SCAN_NAN_ORD) return 0ull;  // (no real key is 0: the smallest ord, -inf's, is 0x007FFFFF)
  return ((uint64_t)ord << 32) | 0xFFFFFFFFull;
}
FNV_SCAN_HD inline bool scan_in_range(uint64_t key, uint64_t bound) { return !scan_key_less(bound, key); }
// The option's value: off, a radius, or neither (FNV_ERR_INVALID: beyond 32 bits, or the bits of a NaN).
FNV_SCAN_HD inline bool scan_radius_valid(int64_t value) {
  return value < 0 || (value <= 0xFFFFFFFFll && scan_dist_ord((uint32_t)value) != SCAN_NAN_ORD);
}

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
  // Range search (the kernels' RANGE forms and the merge; a launch without a radius leaves both zero and runs the other forms):
  uint32_t* range_counts;      // [nq][segments]: every (query, segment)'s in-range candidates, behind the partial lists; null: no radius
  uint64_t range_bound;        // scan_range_bound(radius)
};

// ---- the float16 matrix engine's prefilter (scan_matrix_f16.hpp, option "scan_matrix_float") ---------------------------------
// That engine forms an APPROXIMATE score of a (query, row) pair from a matrix-instruction dot product and two norms,
//   L2: s~ = rn + qn - 2 dot~      IP: s~ = 1 - dot~,      rn ~ sum x_i^2,  qn ~ sum y_i^2  (each a float32 sum in some order),
// and drops the pair when  s~ - scan_margin(P, rn, qn, ip) > the query's K-th exact distance so far.  For that to lose nothing,
// scan_margin must bound |s~ - d| for every finite input, d being the float32 distance the vector scan reports for the pair
// (distance.hpp, Dist<_Float16, METRIC>: per-element fma chains, lane sums, group_sum).  P = the elements the instruction sums,
// zero padding included; u = 2^-24; D = the real-number distance; A = sum |x_i y_i| <= (RN + QN) / 2 with RN, QN the real norms;
// sum (x_i - y_i)^2 <= 2 (RN + QN).
// Assumptions, each named where it is used:
//   (a) a product of two binary16 values is exact in float32 (22 significant bits, exponents within float32's normal range);
//   (b) every accumulation step inside the matrix instruction is off by at most one unit in the last place of the running
//       magnitude, 2 u |partial|, whatever the order of the steps and whether they round or truncate;
//   (c) the norms are float32 sums of exact squares, each step rounded to nearest (the kernel's v_fma_mix_f32 chain, which
//       keeps binary16 subnormals: profiles/distance_bits.md);
//   (d) the matrix instruction MAY flush binary16 subnormal inputs to zero (not established for gfx950 either way).
// L2.  The vector scan: every difference rounded once, P fused steps and log2(64) + 1 additions:  |d - D| <= (P + 8) 2u D
//      <= (P + 8) 4u (RN + QN).  The score: |rn - RN| <= P 2u RN and the same for qn (c); |dot~ - dot| <= P 2u A (1 + P 2u)
//      (a, b); the two additions of the combination round an amount of at most 2 (rn + qn) each.  Together
//      |s~ - d| <= (4 P + 20) 2u (RN + QN) (1 + P 2u), and RN <= rn (1 + P 2u).
// IP.  |s_v - dot| <= (P + 8) u A for the vector scan's sum, |dot~ - dot| as above, and each side rounds 1 - s once:
//      |s~ - d| <= (1.5 P + 5) 2u (RN + QN) / 2 + 2u (1 + A).
// (d)  A flushed element loses its products: less than 2^-14 |other side| each, at most
//      2^-14 (sum |y_i| + sum |x_i|) <= 2^-14 (sqrt(P QN) + sqrt(P RN))  (Cauchy-Schwarz), twice that in L2's -2 dot~.
// scan_margin is kappa (P + 4) 2u (rn + qn) with kappa = 16 -- four times what L2 needs, over twenty times what IP needs, which
// also covers the float32 rounding of this function and P 2u <= 1 (rows below 4 M elements) -- plus 2^-11 sqrt(P n) per side
// for (d), four times the bound, plus 2^-21 for the rounding of 1 - s.  A margin too wide costs rescored pairs; one too narrow
// costs a wrong result, so none of these constants is tuned against a test.  NaN and infinite norms give a NaN or infinite
// margin, which the kernel's compare lets pass (tests/test_scan_matrix_f16_plan.py holds the finite case on the CPU).
// Range search ("scan_radius") asks nothing more of the margin: |s~ - d| <= margin bounds the score's distance from the vector
// scan's d whatever d is compared with, so  s~ - margin > r  implies  d > r  just as it implied d > the K-th distance: the pair
// is out of range and may go unscored and uncounted.  The engines' RANGE forms drop by r INSTEAD of the K-th distance -- a pair
// that may lie within r must be rescored to be counted, even where it cannot enter the list.  The same holds for scan_margin_f32.
constexpr float kScanMarginKappa = 16.0f;
FNV_SCAN_HD inline float scan_margin_term(uint32_t P, float n) {  // one side's share: the kernel forms it once per row and per query
  return kScanMarginKappa * (float)(P + 4u) * 0x1p-23f * n + 0x1p-11f * sqrtf((float)P * n);
}
FNV_SCAN_HD inline float scan_margin_of_terms(float row_term, float query_term, bool ip) {
  return row_term + query_term + (ip ? 0x1p-21f : 0.0f);
}
FNV_SCAN_HD inline float scan_margin(uint32_t P, float rn, float qn, bool ip) {
  return scan_margin_of_terms(scan_margin_term(P, rn), scan_margin_term(P, qn), ip);
}
// ---- the float32 matrix engine's prefilter (scan_matrix_f32.hpp, option "scan_matrix_float32") -------------------------------
// The same score from float32 rows and queries whose elements were NARROWED to bfloat16 for the matrix instruction (round to
// nearest even, 8 significant bits), with rn and qn float32 fma chains over the ORIGINAL float32 values.  scan_margin_f32 must
// bound |s~ - d|, d now Dist<float, METRIC>'s float32 distance.  Notation as above; x^ = the narrowed x.
// Assumptions:
//   (a') a product of two bfloat16 values is exact in float32 (16 significant bits; an exponent outside float32's range: (f), (g));
//   (b)  as above, for the accumulation inside the matrix instruction, on the magnitudes A^ = sum |x^_i y^_i| <= (1 + 2^-9)^2 A;
//   (c') the norms are float32 fma chains, one rounding to nearest per element: |rn - RN| <= P 2u RN as before;
//   (d') the matrix instruction MAY flush bfloat16 subnormal inputs, and the conversion float32 subnormals, to zero (neither is
//        established for gfx950); bfloat16's subnormal threshold is float32's, 2^-126;
//   (e)  every float32 step, of the vector scan and of the score alike, MAY flush a subnormal result (at most 2^-126 absolute).
// Accumulation and combination.  The derivation above carries over with this P, with A^ for A in the dot product's term and
//      one more rounding per product in the vector scan's L2 (x_i - y_i of two float32 values rounds; of two binary16 values it
//      did not): within the factor four that kappa = 16 leaves.
// Operand rounding.  x^ = x (1 + e), |e| <= 2^-9 for every x^ that is a normal number, so
//      |sum x^_i y^_i - sum x_i y_i| <= (2^-8 + 2^-18) A <= (2^-8 + 2^-18) (RN + QN) / 2;  L2's -2 dot~ takes twice that:
//      (2^-8 + 2^-18) (RN + QN).  The margin takes 2^-7 (rn + qn) for L2 and 2^-8 (rn + qn) for IP -- TWICE the bound of
//      either (both are attained, up to 2^-18, by a row equal to its query whose every element lies halfway between two
//      bfloat16 values), which also covers RN <= rn (1 + P 2u) and the float32 rounding of this function.  This term is the
//      margin for real data: 2^-7 of the norms against the 2^-18 or so of everything else.
// (d') An element that is flushed, or is a subnormal rounded absolutely rather than relatively, moves by less than 2^-126 and
//      its products by less than 2^-126 |other side| each: at most 2^-126 (sqrt(P QN) + sqrt(P RN)), twice that in L2.
//      2^-123 sqrt(P n) per side is four times the L2 bound.
// (e)  At most 4 P + 20 float32 steps lie between the inputs and |s~ - d| (P + 8 in the vector scan, P in each norm, P in the
//      dot product, the combination), the dot product's counted twice in L2: less than (6 P + 20) 2^-126.  (P + 4) 2^-122 per
//      side is more than four times that.  Both (d') and (e) vanish beside the other terms unless the norms are below 2^-100.
// (f)  An element of magnitude above 2^127 (2 - 2^-8) narrows to bfloat16 infinity.  Its float32 square overflows, so rn or qn
//      is +inf, the margin is +inf or NaN, and score - margin is -inf or NaN: the pair survives, whatever the instruction made
//      of the infinite operand.  The same holds when a norm overflows without any element doing so.
// (g)  With finite rn + qn no partial sum of the dot product exceeds A^ <= (1 + 2^-8) (rn + qn) / 2, so the dot product can
//      overflow only with norms at the very top of the range, where the vector scan's distance may still be finite.  The kernel
//      therefore lets a pair through whenever score - margin is not a FINITE number above the K-th distance.
// As above, none of these constants is tuned against a test (tests/test_scan_matrix_f32_plan.py holds the finite case on the
// CPU, with bfloat16 narrowing done by bit arithmetic, with and without the flushes).
FNV_SCAN_HD inline float scan_margin_f32_term(uint32_t P, float n, bool ip) {  // one side's share, formed once per row and per query
  return (kScanMarginKappa * (float)(P + 4u) * 0x1p-23f + (ip ? 0x1p-8f : 0x1p-7f)) * n + 0x1p-123f * (sqrtf((float)P) * sqrtf(n)) +
         (float)(P + 4u) * 0x1p-122f;  // (two roots: P n may overflow where n does not)
}
FNV_SCAN_HD inline float scan_margin_f32(uint32_t P, float rn, float qn, bool ip) {
  return scan_margin_of_terms(scan_margin_f32_term(P, rn, ip), scan_margin_f32_term(P, qn, ip), ip);
}
// The float engines' parameter block: the plain one, the lanes per vector (G) of the index's row configuration -- survivors are rescored in the
// vector scan's own lane order -- and two counters of the launch, {pairs scored, pairs rescored}, zero at launch.
struct ScanMatrixFloatParams : ScanParams {
  uint32_t group_lanes;
  unsigned long long* counters;
};
// The float engines' BLOCK form (scan_matrix_block.hpp, option "scan_matrix_block"): `waves` wavefronts per block, each owning
// `wave_subtiles` 32-query sub-tiles of the tile (tile_queries = 32 waves wave_subtiles), share every 32-row tile through a ring
// of kScanBlockRing buffers in LDS behind the wavefronts' queries and lists.  One buffer: a span of at most kScanBlockSpanSteps
// MFMA steps of the 32 rows in operand order (1 KB a step, 16-bit operands for both element types), the rows' {norm, margin
// term} pairs, their node ids.  The planner (launch_plan.hpp, scan_block_shape) and the kernel size it by this one function.
constexpr uint32_t kScanBlockRing = 2, kScanBlockSpanSteps = 8, kScanBlockMaxWaves = 4, kScanBlockMaxWaveSubtiles = 4;
FNV_SCAN_HD inline uint32_t scan_block_buffer_bytes(uint32_t steps) {
  return (steps < kScanBlockSpanSteps ? steps : kScanBlockSpanSteps) * 1024u + 32u * 8u + 32u * 4u;
}
struct ScanMatrixBlockParams : ScanMatrixFloatParams {
  uint32_t waves;
  uint32_t wave_subtiles;
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
// The matrix engines' grouped forms ("scan_matrix_grouped"; scan_matrix_feed.hpp) queue ids the same way and hand them out as
// 32-row tiles, the tile after the current one already requested from HBM: the queue is refilled whenever it holds fewer than
// two tiles, so it must take 63 leftovers and one 32-node word (95 ids) to make progress.  256 ids = 1 KB again: a refill then
// queues six tiles' worth of a dense row at once, and the prefix over the words' popcounts is paid once per six tiles.
constexpr uint32_t MATRIX_QUEUE_IDS = 256;

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
  uint32_t group_lanes;        // the float matrix engines' grouped forms only: as ScanMatrixFloatParams
  unsigned long long* counters;
};

}  // namespace fnv_dev
