// scan_matrix_f16.hpp -- part of the gfx950 search engine (device code; included by kernel_inst.hip's `scan_mf` units).
// The FLOAT16 MATRIX ENGINE of the exhaustive search ("scan_matrix_float" = 1): exhaustive_scan_matrix_f16_kernel (KSf) takes the
// place of exhaustive_scan_kernel (scan.hpp, step 2) on float16 indexes, for an unfiltered call or one with a single filter.
// The steps before it (node filter, compaction) and after it (the partial lists, exhaustive_merge_kernel) are scan.hpp's.
//
// Why it may.  A float sum re-associated is another float, so a matrix-instruction dot product cannot be the REPORTED distance
// of a float row.  It can be a FILTER: a score that is provably within scan_margin (scan_select.hpp: the
// derivation and its assumptions) of the vector scan's float32 distance discards every pair that cannot reach its query's K-th
// distance -- all but about K ln(n / K) rows per query and segment -- and only the survivors are scored, with exactly the
// vector scan's arithmetic.  Only those exact distances are compared with a list, inserted and reported: every reported
// distance has the vector scan's bits WHATEVER the margin, and a sound margin makes the selection identical too, since the
// order is total (scan_select.hpp) and a dropped pair's exact distance is strictly above a K-th distance already listed.
//
// 1. Prefilter.  C = nchunks + tail_chunks 16-byte chunks of a row take part, S = ceil(C / 2) steps of
//    v_mfma_f32_32x32x16_f16 (a missing last half-step is fed zeros on both sides), P = 16 S elements.  The skeleton is
//    scan_matrix.hpp's: one wavefront per (query tile, row segment); the tile's queries staged ONCE in LDS in operand order --
//    sub-tile t, step s, lane l at uint4 [(t * S + s) * 64 + l] = chunk 2 s + l / 32 of query 32 t + l % 32, one lane's eight
//    halves of the B operand; lane l loads chunk 2 s + l / 32 of row l % 32 of a 32-row tile straight from HBM into the A operand
//    (a table chunk IS the operand; filtered calls gather by cand_ids, split rows read chunks >= nchunks from the side table),
//    two register sets taking turns, requests issued without a branch and fixed up at use.  A row tile stays in registers for
//    every sub-tile when it fits MF_SPAN steps (rows of at most 256 bytes: 128-d); longer rows are re-read span by span and get a
//    tile of one sub-tile from the planner.  The lane pair of a row sums the squares of the chunks it holds (rn), staging does
//    the same per query (qn); each side's share of the margin is formed once, with its norm.  In the 32 x 32 result lane l holds
//    column l % 32 -- one query -- and rows 8 (v / 4) + 4 (l / 32) + v % 4 in registers v = 0 .. 15 (the byte engine's mapping;
//    tests/test_gpu_scan_matrix_f16.py holds it to float64 and to the vector scan).  Per register:
//        score = rn + qn - 2 dot  (L2)   or   1 - dot  (IP);     the pair survives unless  score - margin > kd,
//    kd = the query's K-th EXACT distance, read from its list at every (row tile, sub-tile) -- +inf while the list is not full.
//    The negated compare lets a NaN or infinite score or margin through.  Rows past the segment's end and columns past the
//    tile's last query never survive.  A lane's sixteen survivor bits are all that leaves this path.
// 2. Rescoring.  Survivors of a register are ballotted and scored 64 / G at a time, G = the lanes per vector of the index's
//    row configuration (ScanMatrixFloatParams::group_lanes): lane g of a group takes chunks g, g + G, ... below C -- the side
//    table's chunks included -- through Dist<_Float16, METRIC>::chunk in that order, then lane_sum, group_sum<G> and finish.
//    That is exhaustive_scan_kernel's arithmetic operation for operation (the chunks it adds beyond C are zero on both sides and
//    leave an accumulator as it is).  The query's chunks come back out of the operand-order LDS, the row's chunks are re-read
//    (cache hits).  The exact distance goes into scan_key, is compared with the list's real K-th key and inserted by scan_insert.
// 3. Counters.  A block adds {pairs scored, pairs rescored} to the launch's two counters with one atomic each
//    (fnv_last_replayed_queries reports them); out_ndist stays the candidate count.
//
// Grouped calls ("scan_matrix_grouped" = 1 as well): exhaustive_scan_matrix_f16_grouped_kernel, as scan_matrix.hpp's grouped
// form -- the tile's queries are perm[first ..], its rows the bits of its filter row by way of MatrixRowFeeder
// (scan_matrix_feed.hpp), the id queue behind the query terms in LDS; one kernel template, the ungrouped walk kept as it was.
//
// Not taken by this engine (the call keeps its own): float32 and 1-byte indexes, grouped calls without that option, the scan
// stage of a routed filtered graph search, and shapes whose 32 queries and lists exceed a block's LDS.
#pragma once
#include "scan_matrix_feed.hpp"
namespace fnv_dev {

typedef _Float16 mf_f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t mf_u32x4 __attribute__((ext_vector_type(4)));
typedef float mf_f32x16 __attribute__((ext_vector_type(16)));
constexpr int MF_N = 32;    // the MFMA's N: queries per sub-tile (and its M: rows per row tile)
constexpr int MF_SPAN = 8;  // MFMA steps (two chunks of a row each) a lane keeps in registers: rows of up to 256 bytes whole

// acc + the squares of a chunk's eight values (even elements into .x, odd ones into .y)
__device__ __forceinline__ f32x2 mf_squares(f32x2 acc, const uint4& x) { return Dist<_Float16, FNV_METRIC_IP>::chunk(acc, x, x); }
// the result row of accumulator register v in the lanes of half `half`
__device__ __forceinline__ uint32_t mf_row(int v, int half) { return (uint32_t)(8 * (v >> 2) + (v & 3) + 4 * half); }

// The survivors of one (row tile, sub-tile) -- bit v of `mine`: this lane's query against row mf_row(v, lane / 32) -- scored
// exactly and offered to their lists.  `qsub`: the sub-tile's queries in operand order, `sublists`: its lists, `id`: the row
// tile's node ids (lane l: row l % 32).  Returns how many there were.
// RANGE (scan.hpp, "Range search"): a survivor whose exact key is in range is counted in `subcounts` (the sub-tile's counters; lane 0
// owns them), whether or not it then enters its list; one out of range is neither.
template <int METRIC, int G, bool RANGE = false>
__device__ __forceinline__ uint32_t mf_rescore(const ScanParams& p, const uint4* qsub, uint64_t* sublists, uint32_t mine,
                                               uint32_t id, int lane, [[maybe_unused]] uint32_t* subcounts = nullptr) {
  typedef Dist<_Float16, METRIC> D;
  constexpr int VPW = WAVE / G;
  const uint32_t g = (uint32_t)(lane % G);
  const int grp = lane / G, K = (int)p.K;
  const uint32_t nchunks = p.nchunks, tc = p.tail_chunks;
  uint32_t total = 0;
  for (int v = 0; v < 16; v++) {
    unsigned long long pm = __ballot((mine >> v) & 1u);
    total += (uint32_t)__popcll(pm);
    while (pm) {
      unsigned long long m = pm;  // group `grp` takes the grp-th survivor left
      for (int k = 0; k < grp; k++) m &= m - 1;
      const bool on = m != 0ull;
      const int i = on ? __ffsll((long long)m) - 1 : 0;
      const uint32_t node = (uint32_t)__shfl((int)id, (int)mf_row(v, i >> 5), WAVE), j = (uint32_t)(i & 31);
      f32x2 acc = D::zero();
      if (on) {
        const uint8_t* const rowp = p.vectors + (uint64_t)node * p.row_bytes;
        const uint8_t* const tailp = p.tails + (uint64_t)node * tc * 16u;
        for (uint32_t c = g; c < nchunks + tc; c += G) {
          const uint4 x = qsub[(c >> 1) * 64u + (c & 1u) * 32u + j];
          const uint4 y = *reinterpret_cast<const uint4*>(c < nchunks ? rowp + c * 16u : tailp + (c - nchunks) * 16u);
          acc = D::chunk(acc, x, y);
        }
      }
      const float d = D::finish(group_sum<G>(D::lane_sum(acc, 0)));
      const int cnt = min(__popcll(pm), VPW);
      for (int k = 0; k < cnt; k++) {  // (wave-uniform)
        const uint64_t key = scan_key((uint32_t)__builtin_amdgcn_readlane(__float_as_int(d), k * G),
                                      (uint32_t)__builtin_amdgcn_readlane((int)node, k * G));
        const uint32_t jk = (uint32_t)__builtin_amdgcn_readlane((int)j, k * G);
        uint64_t* const list = sublists + (size_t)jk * K;
        if constexpr (RANGE) {
          if (scan_in_range(key, p.range_bound)) {  // (wave-uniform)
            if (lane == 0) subcounts[jk] += 1u;
            if (scan_key_less(key, list[K - 1])) scan_insert(list, K, key, lane);
          }
        } else {
          if (scan_key_less(key, list[K - 1])) scan_insert(list, K, key, lane);
        }
        pm &= pm - 1;
      }
    }
  }
  return total;
}

// One kernel template for both kinds of call.  GROUPED: the parameter block is the grouped launch's, `gp` points at it.
template <int METRIC, bool GROUPED, bool RANGE = false>
__global__ __launch_bounds__(WAVE) void exhaustive_scan_matrix_f16_any_kernel(const std::conditional_t<GROUPED, GroupedScanParams, ScanMatrixFloatParams> kp) {
  const ScanParams& p = matrix_scan_params(kp);
  [[maybe_unused]] const GroupedScanParams* const gp = matrix_grouped_params(kp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool L2 = METRIC == FNV_METRIC_L2;
  const int lane = threadIdx.x, col = lane & (MF_N - 1), half = lane >> 5;
  const uint32_t tile = blockIdx.x % p.tiles, seg = blockIdx.x / p.tiles;
  GroupTile gt = {0u, 0u, 0u};
  if constexpr (GROUPED) gt = gp->tiles[tile];
  const uint32_t q0 = tile * p.tile_queries;  // (an ungrouped call's first query)
  const uint32_t nqb = GROUPED ? gt.count : min(p.tile_queries, p.nq - q0);
  if (GROUPED && nqb == 0u) return;  // (past the real tiles: the launch is an upper bound)
  const uint32_t nsub = (nqb + MF_N - 1) / MF_N;
  const int K = (int)p.K;
  const uint32_t nchunks = p.nchunks, tc = p.tail_chunks, C = nchunks + tc;
  const int S = (int)((C + 1u) / 2u);
  const uint32_t P = 16u * (uint32_t)S;
  uint4* const qlds = reinterpret_cast<uint4*>(smem);                                                            // [tile / 32][S][64]
  uint64_t* const lists = reinterpret_cast<uint64_t*>(smem + (size_t)p.tile_queries * (uint32_t)S * 32u);        // [tile][K]
  float2* const qterm = reinterpret_cast<float2*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u));  // [tile] {qn, margin term}
  const auto query_of = [&](uint32_t qq) {
    if constexpr (GROUPED) return gp->perm[gt.first + qq];
    else return q0 + qq;
  };

  // RANGE (scan.hpp, "Range search"): the tile's in-range counters, behind everything else, and the radius the prefilter drops by
  [[maybe_unused]] uint32_t* const counts =
      reinterpret_cast<uint32_t*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u + 8u) + (GROUPED ? MATRIX_QUEUE_IDS * 4u : 0u));
  [[maybe_unused]] const float radius = __uint_as_float(scan_key_dist_bits(p.range_bound));
  if constexpr (RANGE) scan_clear_counts(counts, nqb, lane);

  // ---- the tile's queries in operand order (zero beyond dim and beyond the tile), their norms and margin terms, the lists
  for (uint32_t i = lane; i < nsub * (uint32_t)S * 64u; i += WAVE) {
    const uint32_t l = i & 63u, st = i >> 6, s = st % (uint32_t)S, t = st / (uint32_t)S;
    const uint32_t qq = t * MF_N + (l & 31u), c = 2u * s + (l >> 5);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (qq < nqb && c < C) {
      const uint16_t* qsrc = reinterpret_cast<const uint16_t*>(p.queries) + (uint64_t)(GROUPED ? query_of(qq) : q0 + qq) * p.dim;
#pragma unroll
      for (uint32_t e = 0; e < 8u; e++) {
        const uint32_t at = c * 8u + e;
        const uint32_t b = at < p.dim ? qsrc[at] : 0u;
        w[e >> 1] |= b << (16u * (e & 1u));
      }
    }
    qlds[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (uint32_t i = lane; i < nqb * p.K; i += WAVE) lists[i] = SCAN_PAD;
  wave_sync();
  for (uint32_t qq = lane; qq < nsub * MF_N; qq += WAVE) {
    const uint32_t t = qq / MF_N, j = qq % MF_N;
    f32x2 acc = {0.f, 0.f};
    for (uint32_t c = 0; c < 2u * (uint32_t)S; c++) acc = mf_squares(acc, qlds[(t * (uint32_t)S + (c >> 1)) * 64u + (c & 1u) * 32u + j]);
    const float qn = acc.x + acc.y;
    qterm[qq] = make_float2(qn, scan_margin_term(P, qn));
  }
  wave_sync();

  // ---- this block's share of the candidates, 32 rows a step: slots [lo, hi) of the id list or of the live nodes (a grouped
  // call: the bits of the tile's filter row, below)
  const uint64_t ncand = GROUPED ? 0u : p.cand_ids ? (uint64_t)*p.cand_count : p.n_live;
  const uint64_t lo = ncand * seg / p.segments, hi = ncand * (seg + 1) / p.segments;
  const bool one_span = S <= MF_SPAN;
  unsigned long long scored = 0, rescored = 0;  // (wave-uniform) this block's pairs
  // Row `id`'s steps s0 .. s0 + MF_SPAN - 1 (this lane's chunk of each) as they lie in the table.  No branch at all and no use
  // of a loaded value, so the requests stay in flight: a lane without a row reads row 0, a step past the row's last chunk reads
  // chunk 0: legal addresses whose data fix_span discards or no MFMA step takes.
  const auto load_span = [&](mf_u32x4 (&a)[MF_SPAN], uint32_t id, int s0) {
    const uint8_t* const rowp = p.vectors + (uint64_t)id * p.row_bytes;
    const uint8_t* const tailp = p.tails + (uint64_t)id * tc * 16u;
#pragma unroll
    for (int s = 0; s < MF_SPAN; s++) {
      const uint32_t c = 2u * (uint32_t)(s0 + s) + (uint32_t)half, cc = c < C ? c : 0u;
      a[s] = *reinterpret_cast<const mf_u32x4*>(cc < nchunks ? rowp + cc * 16u : tailp + (cc - nchunks) * 16u);
    }
  };
  // ... until the span is used: zero where the lane has no row or the row no chunk
  const auto fix_span = [&](mf_u32x4 (&a)[MF_SPAN], bool valid, int s0) {
#pragma unroll
    for (int s = 0; s < MF_SPAN; s++) {
      if (s0 + s < S) {
        const bool ok = valid && 2u * (uint32_t)(s0 + s) + (uint32_t)half < C;
#pragma unroll
        for (int k = 0; k < 4; k++) a[s][k] = ok ? a[s][k] : 0u;
      }
    }
  };
  // the squares of the lane's chunks of one span, onto r
  const auto span_squares = [&](f32x2 r, const mf_u32x4 (&a)[MF_SPAN], int s0) {
#pragma unroll
    for (int s = 0; s < MF_SPAN; s++) {
      if (s0 + s < S) r = mf_squares(r, make_uint4(a[s][0], a[s][1], a[s][2], a[s][3]));
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
  const auto score_tile = [&](mf_u32x4 (&a)[MF_SPAN], uint32_t id, bool valid, uint64_t base) __attribute__((always_inline)) {
    const uint32_t nrows = GROUPED ? (uint32_t)base : (uint32_t)min((uint64_t)MF_N, hi - base);
    f32x2 rsum = {0.f, 0.f};  // the squares of the lane's chunks of its row
    float rv[16], rt[16];     // the norms and margin terms of the sixteen rows this lane's accumulators belong to
    const auto spread_terms = [&]() {
      float rn = rsum.x + rsum.y;
      rn += __shfl_xor(rn, 32, WAVE);
      const float rm = scan_margin_term(P, rn);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        rv[v] = __shfl(rn, (int)mf_row(v, half), WAVE);
        rt[v] = __shfl(rm, (int)mf_row(v, half), WAVE);
      }
    };
    if (one_span) {
      fix_span(a, valid, 0);
      rsum = span_squares(rsum, a, 0);
      spread_terms();
    }
    for (uint32_t t = 0; t < nsub; t++) {
      mf_f32x16 acc = {0};
      const uint4* const qsub = qlds + (size_t)t * (uint32_t)S * 64u;
      for (int s0 = 0; s0 < S; s0 += MF_SPAN) {
        if (!one_span) {
          load_span(a, id, s0);
          fix_span(a, valid, s0);
          if (t == 0) rsum = span_squares(rsum, a, s0);
        }
#pragma unroll
        for (int s = 0; s < MF_SPAN; s++) {
          if (s0 + s < S) {
            const uint4 x = qsub[(size_t)(s0 + s) * 64u + lane];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(mf_f16x8, a[s]),
                                                         __builtin_bit_cast(mf_f16x8, mf_u32x4{x.x, x.y, x.z, x.w}), acc, 0, 0, 0);
          }
        }
      }
      if (!one_span && t == 0) spread_terms();
      // the lane's query: its norm, its margin term and its K-th exact distance so far (an empty slot: +inf)
      const uint32_t qq = t * MF_N + (uint32_t)col;
      const bool has_query = qq < nqb;
      const float2 qt = qterm[qq];
      float kd = std::numeric_limits<float>::infinity();
      if (has_query) {
        const uint64_t kth = lists[(size_t)qq * K + (K - 1)];
        if (kth != SCAN_PAD) kd = __uint_as_float(scan_key_dist_bits(kth));
      }
      // RANGE: a pair that may lie within the radius is rescored to be counted, even where it cannot enter the list -- so the
      // radius, not the K-th distance, is what a pair is dropped by (scan_select.hpp, where the margin is derived)
      if constexpr (RANGE) kd = radius;
      uint32_t mine = 0;  // bit v: the pair (this lane's query, row mf_row(v, half)) survives
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float score = L2 ? (rv[v] + qt.x) - 2.0f * acc[v] : 1.0f - acc[v];
        const float margin = scan_margin_of_terms(rt[v], qt.y, !L2);
        const bool survives = has_query && mf_row(v, half) < nrows && !(score - margin > kd);  // (a NaN anywhere: survives)
        mine |= (survives ? 1u : 0u) << v;
      }
      scored += (unsigned long long)nrows * min((uint32_t)MF_N, nqb - t * MF_N);
      if (__ballot(mine != 0u)) {  // about K ln(n / K) rows per query, and what the margin adds
        uint64_t* const sublists = lists + (size_t)t * MF_N * K;
        uint32_t n = 0;
        switch (kp.group_lanes) {  // the row configurations of float16 rows (search_types.h, kCfgs)
          case 8: n = mf_rescore<METRIC, 8, RANGE>(p, qsub, sublists, mine, id, lane, counts + t * MF_N); break;
          case 16: n = mf_rescore<METRIC, 16, RANGE>(p, qsub, sublists, mine, id, lane, counts + t * MF_N); break;
          case 32: n = mf_rescore<METRIC, 32, RANGE>(p, qsub, sublists, mine, id, lane, counts + t * MF_N); break;
          default: n = mf_rescore<METRIC, 64, RANGE>(p, qsub, sublists, mine, id, lane, counts + t * MF_N); break;
        }
        rescored += n;
      }
    }
  };

  // Two register sets take turns: while one tile is scored, the next tile's rows are already requested into the other.
  mf_u32x4 a0[MF_SPAN], a1[MF_SPAN];
  uint32_t id0 = 0, id1 = 0;
  bool valid0 = false, valid1 = false;
  if constexpr (GROUPED) {  // the rows are the bits of the tile's filter row over this segment's words (scan_matrix_feed.hpp)
    uint32_t* const queue = reinterpret_cast<uint32_t*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u + 8u));
    MatrixRowFeeder src(queue, gp, gt.row, seg, p.segments, lane);
    const auto request = [&](mf_u32x4 (&a)[MF_SPAN], uint32_t* id, bool* valid, int k) __attribute__((always_inline)) {
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
    const auto request = [&](mf_u32x4 (&a)[MF_SPAN], uint32_t* id, bool* valid, uint64_t base) __attribute__((always_inline)) {
      *valid = row_of(base, id);  // (a tile past the segment's end: no lane has a row, all read row 0)
      if (one_span) load_span(a, *id, 0);
    };
    request(a0, &id0, &valid0, lo);
    for (uint64_t base = lo; base < hi; base += 2 * MF_N) {
      request(a1, &id1, &valid1, base + MF_N);
      score_tile(a0, id0, valid0, base);
      if (base + MF_N >= hi) break;
      request(a0, &id0, &valid0, base + 2 * MF_N);
      score_tile(a1, id1, valid1, base + MF_N);
    }
  }
  if (lane == 0) {
    atomicAdd(kp.counters, scored);
    atomicAdd(kp.counters + 1, rescored);
  }
  scan_flush_tile(p, lists, nqb, seg, lane, query_of);
  if constexpr (RANGE) scan_flush_counts(p, counts, nqb, seg, lane, query_of);
}

template <int METRIC, bool RANGE = false>
constexpr scan_mf_fn exhaustive_scan_matrix_f16_kernel = exhaustive_scan_matrix_f16_any_kernel<METRIC, false, RANGE>;
template <int METRIC, bool RANGE = false>
constexpr scan_grouped_fn exhaustive_scan_matrix_f16_grouped_kernel = exhaustive_scan_matrix_f16_any_kernel<METRIC, true, RANGE>;

}  // namespace fnv_dev
