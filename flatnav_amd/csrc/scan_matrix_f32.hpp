// scan_matrix_f32.hpp -- part of the gfx950 search engine (device code; included by kernel_inst.hip's `scan_mf32` units).
// The FLOAT32 MATRIX ENGINE of the exhaustive search ("scan_matrix_float32" = 1): exhaustive_scan_matrix_f32_kernel (KSf32) takes
// the place of exhaustive_scan_kernel (scan.hpp, step 2) on float32 indexes, for an unfiltered call or one with a single filter.
// The steps before it (node filter, compaction) and after it (the partial lists, exhaustive_merge_kernel) are scan.hpp's.
//
// The method is scan_matrix_f16.hpp's: a matrix-instruction score is a FILTER with a proved margin (scan_select.hpp,
// scan_margin_f32), the survivors are scored again with exactly the vector scan's arithmetic, and only those distances are
// compared with a list, inserted and reported -- every reported distance has the vector scan's bits whatever the margin, and a
// sound margin makes the selection identical too.  What float32 adds: there is no matrix instruction on float32 operands worth
// its rate, so both operands are NARROWED to bfloat16 in registers (v_cvt_pk_bf16_f32, round to nearest even) on their way into
// v_mfma_f32_32x32x16_bf16.  bfloat16 keeps float32's exponent, so no finite value leaves the operand's range but by rounding
// at the very top, which the norms catch; the price is a margin of 2^-7 of the norms (L2), and the table read at twice
// float16's bytes.
//
// 1. Prefilter.  C = nchunks + tail_chunks 16-byte chunks (four floats each) of a row take part, S = ceil(C / 4) steps of the
//    instruction, P = 16 S elements.  One wavefront per (query tile, row segment).
//    Queries: the tile's queries are narrowed ONCE into LDS in operand order -- sub-tile t, step s, lane l at uint4
//    [(t * S + s) * 64 + l] = elements 16 s + 8 (l / 32) ... + 7 of query 32 t + l % 32 as eight bfloat16, zero beyond dim and
//    beyond the tile: 32 bytes per step and query, float16's footprint.  qn is an fma chain over the query's float32 values.
//    Rows: lane l (row l % 32 of a 32-row tile, half l / 32) holds the same eight k-elements of every step: chunks
//    4 s + 2 (l / 32) and the one after it, 32 contiguous bytes, two 16-byte requests straight from HBM (filtered calls gather by
//    cand_ids; a chunk >= nchunks comes from the side table; a chunk at or past C, and a lane without a row, re-reads chunk 0 /
//    row 0 -- legal addresses whose data is zeroed at use).  TWO register sets: `raw`, the float32 chunks of the NEXT unit of
//    work as the loads left them (8 steps x 8 registers, requested without a branch or a use, so they stay in flight while the
//    current unit is scored), and `a`, the CURRENT unit narrowed (8 steps x 4 registers).  At a unit's start raw is fixed up,
//    summed into the row norm (float32 fma chain over the original values, joined across the lane pair), narrowed into `a`, and
//    at once requested again for the unit after.  A unit is a whole row tile when the row fits MF32_SPAN steps (512 bytes:
//    128-d) -- `a` then serves every sub-tile of the query tile -- and one span of a row tile otherwise (the planner gives such
//    rows a tile of one sub-tile, so no row is read twice by a block).  In the 32 x 32 result lane l holds column l % 32 -- one
//    query -- and rows 8 (v / 4) + 4 (l / 32) + v % 4 in registers v = 0 .. 15.  Per register:
//        score = (rn + qn) - 2 dot  (L2)   or   1 - dot  (IP);     the pair survives unless  kd < score - margin < +inf,
//    kd = the query's K-th EXACT distance, read from its list at every (row tile, sub-tile) -- +inf while the list is not full.
//    A NaN or an infinity anywhere -- a norm that overflowed, an element that narrowed to bfloat16 infinity, a NaN row -- lets
//    the pair through (scan_select.hpp (f), (g)).  Rows past the segment's end and columns past the tile's last query never
//    survive.  A lane's sixteen survivor bits are all that leaves this path.
// 2. Rescoring.  Survivors of a register are ballotted and scored 64 / G at a time, G = the lanes per vector of the index's
//    row configuration: lane g of a group takes chunks g, g + G, ... below C through Dist<float, METRIC>::chunk in that order,
//    then lane_sum, group_sum<G> and finish -- exhaustive_scan_kernel's arithmetic operation for operation.  The float32 query
//    is NOT kept in LDS (that would take 856 instead of 344 bytes per query at 128-d and halve the tile, doubling the table's HBM
//    reads): the survivor's query chunks are read from p.queries, which staging has just read (cache hits; about one pair in a
//    thousand gets here on real data), elements at or past dim zero.
// 3. Counters.  {pairs scored, pairs rescored}, one atomic each per block; out_ndist stays the candidate count.
//
// Grouped calls ("scan_matrix_grouped" = 1 as well): exhaustive_scan_matrix_f32_grouped_kernel, as scan_matrix.hpp's grouped
// form -- the tile's queries are perm[first ..] (rescoring finds a survivor's float32 query through perm as well), its rows the
// bits of its filter row by way of MatrixRowFeeder (scan_matrix_feed.hpp), the id queue behind the query terms in LDS; one
// kernel template, the ungrouped staging and walk kept as they were (a grouped lane looks its query up in perm once per sub-tile).
//
// Not taken by this engine (the call keeps its own): other element types, grouped calls without that option, the scan stage of
// a routed filtered graph search, and shapes whose 32 queries and lists exceed a block's LDS.
#pragma once
#include "scan_matrix_feed.hpp"
namespace fnv_dev {

typedef __bf16 mf32_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mf32_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t mf32_u32x4 __attribute__((ext_vector_type(4)));
typedef float mf32_f32x16 __attribute__((ext_vector_type(16)));
constexpr int MF32_N = 32;    // the MFMA's N: queries per sub-tile (and its M: rows per row tile)
constexpr int MF32_SPAN = 8;  // MFMA steps (four chunks of a row each) a lane keeps in registers: rows of up to 512 bytes whole

// two float32 values -> two bfloat16 (round to nearest even), the first in the low half: one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t mf32_narrow2(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{__uint_as_float(a), __uint_as_float(b)}, mf32_bf16x2));
}
// two chunks -> eight bfloat16 in element order: one lane's share of an operand
__device__ __forceinline__ mf32_u32x4 mf32_narrow8(const mf32_u32x4& lo, const mf32_u32x4& hi) {
  return mf32_u32x4{mf32_narrow2(lo[0], lo[1]), mf32_narrow2(lo[2], lo[3]), mf32_narrow2(hi[0], hi[1]), mf32_narrow2(hi[2], hi[3])};
}
// acc + the squares of a chunk's four float32 values (one rounding each)
__device__ __forceinline__ f32x2 mf32_squares(f32x2 acc, const mf32_u32x4& x) {
  const uint4 v = make_uint4(x[0], x[1], x[2], x[3]);
  return Dist<float, FNV_METRIC_IP>::chunk(acc, v, v);
}
// the result row of accumulator register v in the lanes of half `half`
__device__ __forceinline__ uint32_t mf32_row(int v, int half) { return (uint32_t)(8 * (v >> 2) + (v & 3) + 4 * half); }

// The survivors of one (row tile, sub-tile) -- bit v of `mine`: this lane's query against row mf32_row(v, lane / 32) -- scored
// exactly and offered to their lists.  `query_at(j)`: the float32 query of the sub-tile's column j in p.queries, `sublists`: its
// lists, `id`: the row tile's node ids (lane l: row l % 32).  Returns how many there were.
// RANGE (scan.hpp, "Range search"): a survivor whose exact key is in range is counted in `subcounts` (the sub-tile's counters; lane 0
// owns them), whether or not it then enters its list; one out of range is neither.
template <int METRIC, int G, bool RANGE = false, typename F>
__device__ __forceinline__ uint32_t mf32_rescore(const ScanParams& p, F query_at, uint64_t* sublists, uint32_t mine, uint32_t id, int lane,
                                                 [[maybe_unused]] uint32_t* subcounts = nullptr) {
  typedef Dist<float, METRIC> D;
  constexpr int VPW = WAVE / G;
  const uint32_t g = (uint32_t)(lane % G);
  const int grp = lane / G, K = (int)p.K;
  const uint32_t nchunks = p.nchunks, tc = p.tail_chunks, dim = p.dim;
  uint32_t total = 0;
  for (int v = 0; v < 16; v++) {
    unsigned long long pm = __ballot((mine >> v) & 1u);
    total += (uint32_t)__popcll(pm);
    while (pm) {
      unsigned long long m = pm;  // group `grp` takes the grp-th survivor left
      for (int k = 0; k < grp; k++) m &= m - 1;
      const bool on = m != 0ull;
      const int i = on ? __ffsll((long long)m) - 1 : 0;
      const uint32_t node = (uint32_t)__shfl((int)id, (int)mf32_row(v, i >> 5), WAVE), j = (uint32_t)(i & 31);
      f32x2 acc = D::zero();
      if (on) {
        const uint8_t* const rowp = p.vectors + (uint64_t)node * p.row_bytes;
        const uint8_t* const tailp = p.tails + (uint64_t)node * tc * 16u;
        const float* const qp = query_at(j);  // (a query row is aligned to its elements only)
        for (uint32_t c = g; c < nchunks + tc; c += G) {
          uint32_t w[4];
#pragma unroll
          for (uint32_t e = 0; e < 4u; e++) w[e] = c * 4u + e < dim ? __float_as_uint(qp[c * 4u + e]) : 0u;
          const uint4 x = make_uint4(w[0], w[1], w[2], w[3]);
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

// (two wavefronts per SIMD: 256 registers each -- raw 64, narrowed 32, accumulators 16, row terms 32)
// One kernel template for both kinds of call.  GROUPED: the parameter block is the grouped launch's, `gp` points at it.
template <int METRIC, bool GROUPED, bool RANGE = false>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2))) void exhaustive_scan_matrix_f32_any_kernel(
    const std::conditional_t<GROUPED, GroupedScanParams, ScanMatrixFloatParams> kp) {
  const ScanParams& p = matrix_scan_params(kp);
  [[maybe_unused]] const GroupedScanParams* const gp = matrix_grouped_params(kp);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool L2 = METRIC == FNV_METRIC_L2;
  const int lane = threadIdx.x, col = lane & (MF32_N - 1), half = lane >> 5;
  const uint32_t tile = blockIdx.x % p.tiles, seg = blockIdx.x / p.tiles;
  GroupTile gt = {0u, 0u, 0u};
  if constexpr (GROUPED) gt = gp->tiles[tile];
  const uint32_t q0 = tile * p.tile_queries;  // (an ungrouped call's first query)
  const uint32_t nqb = GROUPED ? gt.count : min(p.tile_queries, p.nq - q0);
  if (GROUPED && nqb == 0u) return;  // (past the real tiles: the launch is an upper bound)
  const uint32_t nsub = (nqb + MF32_N - 1) / MF32_N;
  const int K = (int)p.K;
  const uint32_t nchunks = p.nchunks, tc = p.tail_chunks, C = nchunks + tc, dim = p.dim;
  const int S = (int)((C + 3u) / 4u);
  const uint32_t P = 16u * (uint32_t)S;
  uint4* const qlds = reinterpret_cast<uint4*>(smem);                                                            // [tile / 32][S][64]
  uint64_t* const lists = reinterpret_cast<uint64_t*>(smem + (size_t)p.tile_queries * (uint32_t)S * 32u);        // [tile][K]
  float2* const qterm = reinterpret_cast<float2*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u));  // [tile] {qn, margin term}
  const float* const queries = reinterpret_cast<const float*>(p.queries) + (uint64_t)q0 * dim;  // the tile's first query
  const auto query_of = [&](uint32_t qq) {
    if constexpr (GROUPED) return gp->perm[gt.first + qq];
    else return q0 + qq;
  };
  // the float32 query of tile slot qq (a grouped call: through the permutation)
  const auto query_ptr = [&](uint32_t qq) {
    if constexpr (GROUPED) return reinterpret_cast<const float*>(p.queries) + (uint64_t)gp->perm[gt.first + qq] * dim;
    else return queries + (uint64_t)qq * dim;
  };

  // RANGE (scan.hpp, "Range search"): the tile's in-range counters, behind everything else, and the radius the prefilter drops by
  [[maybe_unused]] uint32_t* const counts =
      reinterpret_cast<uint32_t*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u + 8u) + (GROUPED ? MATRIX_QUEUE_IDS * 4u : 0u));
  [[maybe_unused]] const float radius = __uint_as_float(scan_key_dist_bits(p.range_bound));
  if constexpr (RANGE) scan_clear_counts(counts, nqb, lane);

  // ---- the tile's queries narrowed into operand order (zero beyond dim and beyond the tile), their norms and margin terms
  // from the float32 values, the lists
  if constexpr (GROUPED) {  // (a lane stages ONE query per sub-tile: its place in the permutation is looked up once)
    for (uint32_t t = 0; t < nsub; t++) {
      const uint32_t qq = t * MF32_N + (uint32_t)col;
      const float* const qsrc = query_ptr(qq < nqb ? qq : 0u);
      for (uint32_t s = 0; s < (uint32_t)S; s++) {
        const uint32_t e0 = 16u * s + 8u * (uint32_t)half;
        uint32_t w[8];
#pragma unroll
        for (uint32_t e = 0; e < 8u; e++) w[e] = qq < nqb && e0 + e < dim ? __float_as_uint(qsrc[e0 + e]) : 0u;
        const mf32_u32x4 x = mf32_narrow8(mf32_u32x4{w[0], w[1], w[2], w[3]}, mf32_u32x4{w[4], w[5], w[6], w[7]});
        qlds[(t * (uint32_t)S + s) * 64u + (uint32_t)lane] = make_uint4(x[0], x[1], x[2], x[3]);
      }
    }
  } else {
    for (uint32_t i = lane; i < nsub * (uint32_t)S * 64u; i += WAVE) {
      const uint32_t l = i & 63u, st = i >> 6, s = st % (uint32_t)S, t = st / (uint32_t)S;
      const uint32_t qq = t * MF32_N + (l & 31u), e0 = 16u * s + 8u * (l >> 5);
      uint32_t w[8];
#pragma unroll
      for (uint32_t e = 0; e < 8u; e++) w[e] = qq < nqb && e0 + e < dim ? __float_as_uint(queries[(uint64_t)qq * dim + e0 + e]) : 0u;
      const mf32_u32x4 x = mf32_narrow8(mf32_u32x4{w[0], w[1], w[2], w[3]}, mf32_u32x4{w[4], w[5], w[6], w[7]});
      qlds[i] = make_uint4(x[0], x[1], x[2], x[3]);
    }
  }
  for (uint32_t i = lane; i < nqb * p.K; i += WAVE) lists[i] = SCAN_PAD;
  for (uint32_t qq = lane; qq < nsub * MF32_N; qq += WAVE) {
    float qn = 0.f;
    if (qq < nqb) {
      [[maybe_unused]] const float* const qsrc = query_ptr(qq);
      for (uint32_t e = 0; e < dim; e++) {
        const float x = GROUPED ? qsrc[e] : queries[(uint64_t)qq * dim + e];
        qn = __builtin_fmaf(x, x, qn);
      }
    }
    qterm[qq] = make_float2(qn, scan_margin_f32_term(P, qn, !L2));
  }
  wave_sync();

  // ---- this block's share of the candidates, 32 rows a step
  const uint64_t ncand = GROUPED ? 0u : p.cand_ids ? (uint64_t)*p.cand_count : p.n_live;
  const uint64_t lo = ncand * seg / p.segments, hi = ncand * (seg + 1) / p.segments;
  const bool one_span = S <= MF32_SPAN;
  unsigned long long scored = 0, rescored = 0;  // (wave-uniform) this block's pairs
  // Row `id`'s steps s0 .. s0 + MF32_SPAN - 1 (this lane's two chunks of each) as they lie in the table.  No branch at all and
  // no use of a loaded value, so the requests stay in flight: a lane without a row reads row 0, a chunk at or past C reads chunk
  // 0: legal addresses whose data narrow_span discards or no MFMA step takes.
  const auto load_span = [&](mf32_u32x4 (&r)[MF32_SPAN][2], uint32_t id, int s0) {
    const uint8_t* const rowp = p.vectors + (uint64_t)id * p.row_bytes;
    const uint8_t* const tailp = p.tails + (uint64_t)id * tc * 16u;
#pragma unroll
    for (int s = 0; s < MF32_SPAN; s++) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t c = 4u * (uint32_t)(s0 + s) + 2u * (uint32_t)half + (uint32_t)h, cc = c < C ? c : 0u;
        r[s][h] = *reinterpret_cast<const mf32_u32x4*>(cc < nchunks ? rowp + cc * 16u : tailp + (cc - nchunks) * 16u);
      }
    }
  };
  // ... until the span is used: zero where the lane has no row or the row no chunk, the squares of the float32 values onto
  // `rsum`, the values narrowed into `a`
  const auto narrow_span = [&](mf32_u32x4 (&a)[MF32_SPAN], f32x2& rsum, const mf32_u32x4 (&r)[MF32_SPAN][2], bool valid, int s0) {
#pragma unroll
    for (int s = 0; s < MF32_SPAN; s++) {
      if (s0 + s < S) {
        mf32_u32x4 x[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const bool ok = valid && 4u * (uint32_t)(s0 + s) + 2u * (uint32_t)half + (uint32_t)h < C;
#pragma unroll
          for (int k = 0; k < 4; k++) x[h][k] = ok ? r[s][h][k] : 0u;
          rsum = mf32_squares(rsum, x[h]);
        }
        a[s] = mf32_narrow8(x[0], x[1]);
      }
    }
  };
  [[maybe_unused]] const auto row_of = [&](uint64_t base, uint32_t* id) {  // the lane's row of the tile that starts at candidate `base`
    const uint64_t slot = base + (uint64_t)col;
    const bool valid = slot < hi;
    *id = valid ? (p.cand_ids ? p.cand_ids[slot] : (uint32_t)slot) : 0u;
    return valid;
  };

  mf32_u32x4 raw[MF32_SPAN][2], a[MF32_SPAN];
  uint32_t next_id = 0;
  // The walk over the 32-row tiles: candidates base .. base + 31 of [lo, hi), or -- a grouped call -- what the feeder hands out
  // from the bits of the tile's filter row over this segment's words (scan_matrix_feed.hpp; its queue lies behind the query terms).
  uint32_t* const queue = reinterpret_cast<uint32_t*>(smem + (size_t)p.tile_queries * ((uint32_t)S * 32u + p.K * 8u + 8u));
  std::conditional_t<GROUPED, MatrixRowFeeder, MatrixNoFeeder> src(queue, gp, gt.row, seg, p.segments, lane);
  const auto next_row = [&](uint64_t base, uint32_t* id) {  // this lane's row of the tile after the current one
    if constexpr (GROUPED) return src.row(1, id);
    else return row_of(base + MF32_N, id);
  };
  bool next_valid = GROUPED ? src.row(0, &next_id) : row_of(lo, &next_id);
  load_span(raw, next_id, 0);
  for (uint64_t base = lo; GROUPED ? src.more() : base < hi; base += MF32_N, src.advance()) {
    const uint32_t id = next_id;
    const bool valid = next_valid;
    const uint32_t nrows = GROUPED ? src.nrows() : (uint32_t)min((uint64_t)MF32_N, hi - base);
    f32x2 rsum = {0.f, 0.f};  // the squares of the lane's chunks of its row
    float rv[16], rt[16];     // the norms and margin terms of the sixteen rows this lane's accumulators belong to
    for (uint32_t t = 0; t < nsub; t++) {
      mf32_f32x16 acc = {0};
      const uint4* const qsub = qlds + (size_t)t * (uint32_t)S * 64u;
      for (int s0 = 0; s0 < S; s0 += MF32_SPAN) {
        if (t == 0 || !one_span) {  // (wave-uniform) a new unit: `raw` becomes `a`, and the unit after it is requested
          f32x2 sq = rsum;
          narrow_span(a, sq, raw, valid, s0);
          if (t == 0) rsum = sq;
          const bool same_rows = !one_span && (s0 + MF32_SPAN < S || t + 1 < nsub);
          if (!same_rows) next_valid = next_row(base, &next_id);  // (past the segment's end: no lane has a row, all read row 0)
          load_span(raw, same_rows ? id : next_id, s0 + MF32_SPAN < S ? s0 + MF32_SPAN : 0);
        }
#pragma unroll
        for (int s = 0; s < MF32_SPAN; s++) {
          if (s0 + s < S) {
            const uint4 x = qsub[(size_t)(s0 + s) * 64u + lane];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mf32_bf16x8, a[s]),
                                                          __builtin_bit_cast(mf32_bf16x8, mf32_u32x4{x.x, x.y, x.z, x.w}), acc, 0, 0, 0);
          }
        }
      }
      if (t == 0) {  // the rows' norms and margin terms, once per row tile
        float rn = rsum.x + rsum.y;
        rn += __shfl_xor(rn, 32, WAVE);
        const float rm = scan_margin_f32_term(P, rn, !L2);
#pragma unroll
        for (int v = 0; v < 16; v++) {
          rv[v] = __shfl(rn, (int)mf32_row(v, half), WAVE);
          rt[v] = __shfl(rm, (int)mf32_row(v, half), WAVE);
        }
      }
      // the lane's query: its norm, its margin term and its K-th exact distance so far (an empty slot: +inf)
      const uint32_t qq = t * MF32_N + (uint32_t)col;
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
      uint32_t mine = 0;  // bit v: the pair (this lane's query, row mf32_row(v, half)) survives
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float score = L2 ? (rv[v] + qt.x) - 2.0f * acc[v] : 1.0f - acc[v];
        const float bound = score - scan_margin_of_terms(rt[v], qt.y, !L2);
        const bool drop = bound > kd && bound <= std::numeric_limits<float>::max();  // (a NaN or an infinity anywhere: survives)
        const bool survives = has_query && mf32_row(v, half) < nrows && !drop;
        mine |= (survives ? 1u : 0u) << v;
      }
      scored += (unsigned long long)nrows * min((uint32_t)MF32_N, nqb - t * MF32_N);
      if (__ballot(mine != 0u)) {  // about K ln(n / K) rows per query, and what the margin adds
        uint64_t* const sublists = lists + (size_t)t * MF32_N * K;
        [[maybe_unused]] const float* const qfirst = queries + (uint64_t)t * MF32_N * dim;
        const auto query_at = [&](uint32_t j) {
          if constexpr (GROUPED) return query_ptr(t * MF32_N + j);
          else return qfirst + (uint64_t)j * dim;
        };
        uint32_t n = 0;
        switch (kp.group_lanes) {  // the row configurations of float32 rows (search_types.h, kCfgs)
          case 8: n = mf32_rescore<METRIC, 8, RANGE>(p, query_at, sublists, mine, id, lane, counts + t * MF32_N); break;
          case 16: n = mf32_rescore<METRIC, 16, RANGE>(p, query_at, sublists, mine, id, lane, counts + t * MF32_N); break;
          case 32: n = mf32_rescore<METRIC, 32, RANGE>(p, query_at, sublists, mine, id, lane, counts + t * MF32_N); break;
          default: n = mf32_rescore<METRIC, 64, RANGE>(p, query_at, sublists, mine, id, lane, counts + t * MF32_N); break;
        }
        rescored += n;
      }
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
constexpr scan_mf_fn exhaustive_scan_matrix_f32_kernel = exhaustive_scan_matrix_f32_any_kernel<METRIC, false, RANGE>;
template <int METRIC, bool RANGE = false>
constexpr scan_grouped_fn exhaustive_scan_matrix_f32_grouped_kernel = exhaustive_scan_matrix_f32_any_kernel<METRIC, true, RANGE>;

}  // namespace fnv_dev
