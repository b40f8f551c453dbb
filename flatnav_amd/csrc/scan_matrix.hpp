// scan_matrix.hpp -- part of the gfx950 search engine (device code; included by kernel_inst.hip's `scan_m` units).
// The MATRIX ENGINE of the exhaustive search ("scan_matrix" = 1): exhaustive_scan_matrix_kernel (KSm) takes the place of
// exhaustive_scan_kernel (scan.hpp, step 2) on uint8 and int8 indexes, for an unfiltered call or one with a single filter.
// The steps before it (node filter, compaction) and after it (the partial lists, exhaustive_merge_kernel) are scan.hpp's.
//
// Why it may.  DistInt (distance.hpp) reports (float)s or 1.0f - (float)s of an EXACT int32 s; an integer sum is the same
// integer in any order, so the dot products may come from v_mfma_i32_32x32x32_i8 and every key still has the bits the vector
// scan gives it.  That holds for the 1-byte element types only: a float sum re-associated is another float.
//
// Arithmetic.  C = nchunks + tail_chunks 16-byte chunks of a row take part, P = 16 * C elements (the table's zero padding
// included); S = ceil(C / 2) MFMA steps of 32 elements each, a missing last half-step fed with zero registers on both sides.
//   int8   dot = sum x*y by MFMA.                    IP: s = dot.    L2: s = sum x^2 + sum y^2 - 2 dot  (DistInt::lane_sum's form).
//   uint8  the MFMA is signed: every byte of the P elements has its top bit flipped on both sides, x' = x - 128, dot' = sum x'y'.
//          L2: x' - y' = x - y, so s = sum x'^2 + sum y'^2 - 2 dot' (a pad is -128 on both sides and cancels).
//          IP: s = dot' + 128 (sum x' + sum y') + 128^2 P.
// Every term is an int32 and is added modulo 2^32, so s is exact whenever it fits an int32 -- the bound the vector scan's own
// int32 sums already set (sum (x - y)^2 and sum x*y below 2^31: fewer than 33 025 one-byte elements per row).  A row's own
// term (its norm, or 128 x its sum) comes from the chunks the lane has loaded for the MFMA (v_dot4), never from a table.
//
// Work split.  One wavefront per (query tile, row segment), as the vector scan; but a tile is up to 128 queries (a multiple of
// the MFMA's N = 32: scan_matrix_shape, launch_plan.hpp), staged ONCE in LDS in the MFMA's operand order -- sub-tile t, step s,
// lane l at uint4 [(t * S + s) * 64 + l] = chunk 2 s + l / 32 of query 32 t + l % 32 -- so that a step's B operand is one
// conflict-free ds_read_b128.  Rows are M: lane l loads chunk 2 s + l / 32 of row l % 32 of the 32-row tile straight from HBM
// into the A operand (the table's 16-byte chunks ARE the operand layout; filtered calls gather by cand_ids, split rows read
// chunks >= nchunks from the side table), the next row tile's loads in flight while this one is scored (two register sets that
// take turns; nothing touches a loaded value before its tile's turn -- the uint8 flip included).  A row tile stays in
// registers for every sub-tile of the query tile when it fits MS_SPAN steps (rows of at most 128 bytes); longer rows are
// re-read span by span, and the planner gives them a tile of one sub-tile, so nothing is read twice.
// In the 32 x 32 result lane l holds column l % 32 -- ONE query -- and rows 8 (v / 4) + 4 (l / 32) + v % 4 in accumulator
// registers v = 0 .. 15 (tests/test_gpu_scan_matrix.py holds this mapping to numpy from 32 x 32 x 32 up).  The lane keeps its
// query's K-th distance in a register; a score that does not reach it costs a convert and a compare.  The compare's mask is
// the ballot; only when it is not empty (about K ln(n / K) rows per query) does the wave build the key with scan_key, check it
// against the list's real K-th key -- rows past the segment's end are dropped there, before that compare -- and insert it with
// scan_insert.  The lists are scan.hpp's ([tile][K] keys) and leave through scan_flush_tile, so the merge does not change.
//
// Grouped calls ("scan_matrix_grouped" = 1 as well): exhaustive_scan_matrix_grouped_kernel, one wavefront per (tile descriptor,
// row segment) as exhaustive_scan_grouped_kernel.  The tile's queries are perm[first ..] (GroupTile), up to the matrix tile; the
// rows are the bits of the tile's filter row, turned into 32-row tiles by MatrixRowFeeder (scan_matrix_feed.hpp); the id queue
// follows the query terms in LDS.  Everything else -- staging, terms, scoring, lists -- is the one kernel template below; the
// ungrouped kernel keeps its own walk over the candidates, so it compiles to the code it was before the grouped form existed.
//
// Not taken by this engine (the call runs the vector scan): float32 and float16 indexes, grouped calls without that option, the
// scan stage of a routed filtered graph search, and shapes whose 32 queries and lists exceed a block's LDS.
#pragma once
#include "scan_matrix_feed.hpp"
namespace fnv_dev {

typedef int ms_i32x4 __attribute__((ext_vector_type(4)));
typedef int ms_i32x16 __attribute__((ext_vector_type(16)));
constexpr int MS_N = 32;    // the MFMA's N: queries per sub-tile (and its M: rows per row tile)
constexpr int MS_SPAN = 4;  // MFMA steps (32 bytes of a row each) a lane keeps in registers: rows of up to 128 bytes whole

// One kernel template for both kinds of call.  GROUPED: the parameter block is the grouped launch's, `gp` points at it.
template <typename T, int METRIC, bool GROUPED, bool RANGE = false>
__global__ __launch_bounds__(WAVE) void exhaustive_scan_matrix_any_kernel(const std::conditional_t<GROUPED, GroupedScanParams, ScanParams> kp) {
  const ScanParams& p = matrix_scan_params(kp);
  [[maybe_unused]] const GroupedScanParams* const gp = matrix_grouped_params(kp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef Dist<T, METRIC> D;
  constexpr bool FLIP = !D::SIGNED;                                // uint8: bytes go through the signed MFMA as x - 128
  constexpr bool L2 = METRIC == FNV_METRIC_L2;
  constexpr bool SIDE = L2 || FLIP;                                // a term per row and one per query on top of the dot
  const int lane = threadIdx.x, col = lane & (MS_N - 1), half = lane >> 5;
  const uint32_t tile = blockIdx.x % p.tiles, seg = blockIdx.x / p.tiles;
  GroupTile gt = {0u, 0u, 0u};
  if constexpr (GROUPED) gt = gp->tiles[tile];
  const uint32_t q0 = tile * p.tile_queries;  // (an ungrouped call's first query)
  const uint32_t nqb = GROUPED ? gt.count : min(p.tile_queries, p.nq - q0);
  if (GROUPED && nqb == 0u) return;  // (past the real tiles: the launch is an upper bound)
  const uint32_t nsub = (nqb + MS_N - 1) / MS_N;
  const int K = (int)p.K;
  const uint32_t nchunks = p.nchunks, tc = p.tail_chunks, C = nchunks + tc;
  const int S = (int)((C + 1u) / 2u);
  uint4* const qlds = reinterpret_cast<uint4*>(smem);                                                            // [tile / 32][S][64]
  uint64_t* const lists = reinterpret_cast<uint64_t*>(smem + (size_t)p.tile_queries * (uint32_t)S * 32u);        // [tile][K]
  int* const qterm = reinterpret_cast<int*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u));     // [tile]
  const auto query_of = [&](uint32_t qq) {
    if constexpr (GROUPED) return gp->perm[gt.first + qq];
    else return q0 + qq;
  };
  // RANGE (scan.hpp, "Range search"): the tile's in-range counters, behind everything else; the radius as the float the lanes
  // compare with -- d <= radius is the key order's "in range" for the numbers an integer sum gives (never a NaN)
  [[maybe_unused]] uint32_t* const counts =
      reinterpret_cast<uint32_t*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u + 4u) + (GROUPED ? MATRIX_QUEUE_IDS * 4u : 0u));
  [[maybe_unused]] const float radius = __uint_as_float(scan_key_dist_bits(p.range_bound));
  if constexpr (RANGE) scan_clear_counts(counts, nqb, lane);

  // ---- the tile's queries in operand order (zero beyond dim, flipped over the P elements the rows cover), their terms, the lists
  for (uint32_t i = lane; i < nsub * (uint32_t)S * 64u; i += WAVE) {
    const uint32_t l = i & 63u, st = i >> 6, s = st % (uint32_t)S, t = st / (uint32_t)S;
    const uint32_t qq = t * MS_N + (l & 31u), c = 2u * s + (l >> 5);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (qq < nqb && c < C) {
      const uint8_t* qsrc = p.queries + (uint64_t)(GROUPED ? query_of(qq) : q0 + qq) * p.dim;
#pragma unroll
      for (uint32_t e = 0; e < 16u; e++) {
        const uint32_t at = c * 16u + e;
        uint32_t b = at < p.dim ? qsrc[at] : 0u;
        if (FLIP) b ^= 0x80u;
        w[e >> 2] |= b << (8u * (e & 3u));
      }
    }
    qlds[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (uint32_t i = lane; i < nqb * p.K; i += WAVE) lists[i] = SCAN_PAD;
  wave_sync();
  if (SIDE) {
    for (uint32_t qq = lane; qq < nsub * MS_N; qq += WAVE) {
      const uint32_t t = qq / MS_N, j = qq % MS_N;
      int acc = 0;
      for (uint32_t c = 0; c < 2u * (uint32_t)S; c++) {
        const uint4 x = qlds[(t * (uint32_t)S + (c >> 1)) * 64u + (c & 1u) * 32u + j];
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; k++) acc = __builtin_amdgcn_sdot4((int)xs[k], L2 ? (int)xs[k] : 0x01010101, acc, false);
      }
      // L2: sum y'^2.  uint8 IP: 128 sum y' + 128^2 P (modulo 2^32, see the head of the file)
      qterm[qq] = L2 ? acc : (int)((uint32_t)acc * 128u + 16384u * 16u * C);
    }
    wave_sync();
  }

  // ---- this block's share of the candidates, 32 rows a step: slots [lo, hi) of the id list or of the live nodes (a grouped
  // call: the bits of the tile's filter row, below)
  const uint64_t ncand = GROUPED ? 0u : p.cand_ids ? (uint64_t)*p.cand_count : p.n_live;
  const uint64_t lo = ncand * seg / p.segments, hi = ncand * (seg + 1) / p.segments;
  const bool one_span = S <= MS_SPAN;
  // Row `id`'s steps s0 .. s0 + MS_SPAN - 1 (this lane's chunk of each) as they lie in the table.  No branch at all and no use
  // of a loaded value -- a wait for an older request must be able to count the younger ones -- so the requests stay in flight:
  // a lane without a row reads row 0, a step past the row's last chunk reads chunk 0: legal addresses whose data fix_span
  // discards or no MFMA step takes.
  const auto load_span = [&](ms_i32x4 (&a)[MS_SPAN], uint32_t id, int s0) {
    const uint8_t* const rowp = p.vectors + (uint64_t)id * p.row_bytes;
    const uint8_t* const tailp = p.tails + (uint64_t)id * tc * 16u;
#pragma unroll
    for (int s = 0; s < MS_SPAN; s++) {
      const uint32_t c = 2u * (uint32_t)(s0 + s) + (uint32_t)half, cc = c < C ? c : 0u;
      a[s] = *reinterpret_cast<const ms_i32x4*>(cc < nchunks ? rowp + cc * 16u : tailp + (cc - nchunks) * 16u);
    }
  };
  // ... until the span is used: zero where the lane has no row or the row no chunk, uint8 bytes as x - 128 elsewhere
  const auto fix_span = [&](ms_i32x4 (&a)[MS_SPAN], bool valid, int s0) {
#pragma unroll
    for (int s = 0; s < MS_SPAN; s++) {
      if (s0 + s < S) {
        const bool ok = valid && 2u * (uint32_t)(s0 + s) + (uint32_t)half < C;
        const int flip = FLIP ? (int)0x80808080u : 0;
#pragma unroll
        for (int k = 0; k < 4; k++) a[s][k] = ok ? a[s][k] ^ flip : 0;
      }
    }
  };
  // the lane's share of its row's term over one span: sum x'^2 (L2) or sum x' (uint8 IP)
  const auto span_term = [&](const ms_i32x4 (&a)[MS_SPAN], int s0) {
    int r = 0;
#pragma unroll
    for (int s = 0; s < MS_SPAN; s++) {
      if (s0 + s < S) {
#pragma unroll
        for (int k = 0; k < 4; k++) r = __builtin_amdgcn_sdot4(a[s][k], L2 ? a[s][k] : 0x01010101, r, false);
      }
    }
    return r;
  };
  [[maybe_unused]] const auto row_of = [&](uint64_t base, uint32_t* id) {  // the lane's row of the tile that starts at candidate `base`
    const uint64_t slot = base + (uint64_t)col;
    const bool valid = slot < hi;
    *id = valid ? (p.cand_ids ? p.cand_ids[slot] : (uint32_t)slot) : 0u;
    return valid;
  };

  // One 32-row tile (candidates base .. base + 31 -- a grouped call: `base` IS the number of its rows, the feeder's nrows(); `a`: its first span as load_span left it, when rows are one span) against
  // every sub-tile of the query tile.
  const auto score_tile = [&](ms_i32x4 (&a)[MS_SPAN], uint32_t id, bool valid, uint64_t base) __attribute__((always_inline)) {
    const uint32_t nrows = GROUPED ? (uint32_t)base : (uint32_t)min((uint64_t)MS_N, hi - base);
    int rterm = 0;  // the row's term, whole in both lanes of the row once its spans are summed
    int rv[16];     // ... and of the sixteen rows this lane's accumulators belong to
    const auto spread_term = [&]() {
      rterm += __shfl_xor(rterm, 32, WAVE);
      if (FLIP && !L2) rterm = (int)((uint32_t)rterm * 128u);
#pragma unroll
      for (int v = 0; v < 16; v++) rv[v] = __shfl(rterm, 8 * (v / 4) + (v % 4) + 4 * half, WAVE);
    };
    if (one_span) {
      fix_span(a, valid, 0);
      if (SIDE) {
        rterm = span_term(a, 0);
        spread_term();
      }
    }
    for (uint32_t t = 0; t < nsub; t++) {
      ms_i32x16 acc = {0};
      const uint4* const qb = qlds + (size_t)t * (uint32_t)S * 64u + lane;
      for (int s0 = 0; s0 < S; s0 += MS_SPAN) {
        if (!one_span) {
          load_span(a, id, s0);
          fix_span(a, valid, s0);
          if (SIDE && t == 0) rterm += span_term(a, s0);
        }
#pragma unroll
        for (int s = 0; s < MS_SPAN; s++) {
          if (s0 + s < S) {
            const uint4 x = qb[(size_t)(s0 + s) * 64u];
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], ms_i32x4{(int)x.x, (int)x.y, (int)x.z, (int)x.w}, acc, 0, 0, 0);
          }
        }
      }
      if (SIDE && !one_span && t == 0) spread_term();
      // the lane's query: its term and its K-th distance so far (an empty slot: +inf; no query in this column: nothing passes)
      const uint32_t qq = t * MS_N + (uint32_t)col;
      const int qt = SIDE ? qterm[qq] : 0;
      const auto kth_dist = [&]() {
        if (qq >= nqb) return -std::numeric_limits<float>::infinity();
        const uint64_t kth = lists[(size_t)qq * K + (K - 1)];
        return kth == SCAN_PAD ? std::numeric_limits<float>::infinity() : __uint_as_float(scan_key_dist_bits(kth));
      };
      float kd = kth_dist();
      if constexpr (RANGE) kd = min(kd, radius);  // a list entry is in range as well
      [[maybe_unused]] uint32_t in_range = 0;  // RANGE: this lane's in-range pairs of the tile, all of one query
#pragma unroll
      for (int v = 0; v < 16; v++) {
        uint32_t s = (uint32_t)acc[v];
        if (L2) s = (uint32_t)rv[v] + (uint32_t)qt - 2u * s;
        else if (FLIP) s += (uint32_t)rv[v] + (uint32_t)qt;
        const float d = D::finish((int)s);
        if constexpr (RANGE) in_range += (d <= radius && qq < nqb && (uint32_t)(8 * (v / 4) + (v % 4) + 4 * half) < nrows) ? 1u : 0u;
        unsigned long long pm = __ballot(d <= kd);  // (ties pass: the key decides)
        while (pm) {
          const int i = __ffsll((long long)pm) - 1;
          pm &= pm - 1;
          const uint32_t r = (uint32_t)(8 * (v / 4) + (v % 4) + 4 * (i >> 5));
          if (r >= nrows) continue;  // (wave-uniform) past the segment's end
          const uint32_t node = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)r);
          const uint64_t key = scan_key((uint32_t)__builtin_amdgcn_readlane(__float_as_int(d), i), node);
          uint64_t* const list = lists + (size_t)(t * MS_N + (uint32_t)(i & 31)) * K;
          if (scan_key_less(key, list[K - 1])) {
            scan_insert(list, K, key, lane);
            if (col == (i & 31)) kd = RANGE ? min(kth_dist(), radius) : kth_dist();
          }
        }
      }
      if constexpr (RANGE) {  // the query's two lanes together; the lower one owns its counter
        if (__ballot(in_range != 0u)) {
          in_range += (uint32_t)__shfl_xor((int)in_range, 32, WAVE);
          if (half == 0 && in_range != 0u) counts[qq] += in_range;
        }
      }
    }
  };

  // Two register sets take turns: while one tile is scored, the next tile's rows are already requested into the other.
  ms_i32x4 a0[MS_SPAN], a1[MS_SPAN];
  uint32_t id0 = 0, id1 = 0;
  bool valid0 = false, valid1 = false;
  if constexpr (GROUPED) {  // the rows are the bits of the tile's filter row over this segment's words (scan_matrix_feed.hpp)
    uint32_t* const queue = reinterpret_cast<uint32_t*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u + 4u));
    MatrixRowFeeder src(queue, gp, gt.row, seg, p.segments, lane);
    const auto request = [&](ms_i32x4 (&a)[MS_SPAN], uint32_t* id, bool* valid, int k) __attribute__((always_inline)) {
      *valid = src.row(k, id);  // (no such tile: no lane has a row, all read row 0)
      if (one_span) load_span(a, *id, 0);
    };
    request(a0, &id0, &valid0, 0);
    while (src.more()) {
      request(a1, &id1, &valid1, 1);
      score_tile(a0, id0, valid0, src.nrows());
      src.advance();
      if (!src.more()) break;
      request(a0, &id0, &valid0, 1);
      score_tile(a1, id1, valid1, src.nrows());
      src.advance();
    }
  } else {
    const auto request = [&](ms_i32x4 (&a)[MS_SPAN], uint32_t* id, bool* valid, uint64_t base) __attribute__((always_inline)) {
      *valid = row_of(base, id);  // (a tile past the segment's end: no lane has a row, all read row 0)
      if (one_span) load_span(a, *id, 0);
    };
    request(a0, &id0, &valid0, lo);
    for (uint64_t base = lo; base < hi; base += 2 * MS_N) {
      request(a1, &id1, &valid1, base + MS_N);
      score_tile(a0, id0, valid0, base);
      if (base + MS_N >= hi) break;
      request(a0, &id0, &valid0, base + 2 * MS_N);
      score_tile(a1, id1, valid1, base + MS_N);
    }
  }
  scan_flush_tile(p, lists, nqb, seg, lane, query_of);
  if constexpr (RANGE) scan_flush_counts(p, counts, nqb, seg, lane, query_of);
}

template <typename T, int METRIC, bool RANGE = false>
constexpr scan_fn exhaustive_scan_matrix_kernel = exhaustive_scan_matrix_any_kernel<T, METRIC, false, RANGE>;
template <typename T, int METRIC, bool RANGE = false>
constexpr scan_grouped_fn exhaustive_scan_matrix_grouped_kernel = exhaustive_scan_matrix_any_kernel<T, METRIC, true, RANGE>;

}  // namespace fnv_dev
