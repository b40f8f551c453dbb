// scan_matrix_block.hpp -- part of the gfx950 search engine (device code; included by kernel_inst.hip's `scan_mb` units and launch.hip).
// The BLOCK FORM of the two float matrix engines of the exhaustive search ("scan_matrix_block" = 1 on top of "scan_matrix_float" /
// "scan_matrix_float32"): exhaustive_scan_matrix_block_kernel takes the place of exhaustive_scan_matrix_f16_kernel /
// exhaustive_scan_matrix_f32_kernel for an ungrouped call with ONE FILTER on rows of at most 8 MFMA steps (float16: 256 bytes,
// float32: 512 bytes: 128-d), where the planner gives it the call (launch_plan.hpp, scan_block_shape).  The method, the margins
// and every reported byte are those engines' (scan_matrix_f16.hpp, scan_matrix_f32.hpp, scan_select.hpp); what changes is who
// reads the table.
//
// Those engines run one wavefront per (query tile, row segment) and every wavefront streams its own copy of the rows from HBM, so
// the table is read nq / tile times and the tile is bounded by ONE wavefront's LDS budget.  Here a workgroup of W <= 4 wavefronts
// takes one (query tile, row segment): every 32-row tile comes from HBM ONCE per block into LDS, and each wavefront scores it
// against its OWN queries -- the tile is W times as wide for the same reads.
//
// 1. Work split.  The tile's 32-query sub-tiles are dealt out in runs: wavefront w owns sub-tiles w * wave_subtiles ... of the tile
//    (none where nq ended).  For its own queries it keeps, in its own part of LDS, what the wave engines keep for a whole tile and
//    in their layout: the queries in operand order [sub-tile][S][64] uint4, the K-entry lists, the {norm, margin term} pairs.
//    No list is touched by two wavefronts: scan_insert and scan_flush_tile stay wave-local.
// 2. Shared rows.  Row tile i (candidates 32 i ... of the segment's share of cand_ids) is LOADED by wavefront i % W: lane l
//    requests its chunks of row l % 32 as the wave engines do (float32 split rows read the side table; no branch on loaded data,
//    absent rows and chunks read legal addresses), and keeps the requests in flight while it scores -- a wavefront's next tile,
//    W tiles ahead, is requested as soon as it has handed one over.  Handing over: the loader zeroes what is absent, sums the
//    squares into the rows' norms (float32 fma chains over the original values), narrows float32 to bfloat16
//    (v_cvt_pk_bf16_f32) and writes the tile into a ring buffer in OPERAND ORDER, [step][lane] uint4 -- consecutive lanes 16
//    consecutive bytes, so both its ds_write_b128 and every reader's ds_read_b128 are free of bank conflicts -- with the 32
//    {norm, margin term} pairs and the node ids.  All of that is done once per row, not once per wavefront.
// 3. Scoring.  Every wavefront reads the tile's A operand from the ring into registers ONCE and, per sub-tile of its own, issues
//    v_mfma_f32_32x32x16_f16 / _bf16 against the B operands, then runs the wave engines' epilogue on the 32 x 32 accumulator --
//    the same  score - margin > kd  test with the element type's own margin -- and their mf_rescore / mf32_rescore, unchanged.
// 4. The ring.  Tile u lies in buffer u % 2.  In step u every wavefront scores tile u, then the loader of tile u + 1 hands it
//    over into the other buffer, then ONE block barrier.  That barrier is the only block-wide synchronisation of the walk: it
//    makes tile u + 1 visible and says that nobody reads tile u any more.  Its loop runs over the segment's tiles, a count formed
//    from the segment's bounds alone, so every wavefront -- one without queries, one that has just rescored -- reaches every
//    barrier.  A wavefront that rescores keeps the others waiting at the step's barrier.
// 5. Counters.  The wavefronts' {pairs scored, pairs rescored} are added up in the ring's memory after the walk: one atomic pair
//    per block.
//
// Tried, measured slower than the wave engines and REMOVED (profiles/scan_matrix_block.md): rows beyond 8 steps walked span by
// span through the ring with the accumulators kept (768-d: 0.63 - 0.90 x), and unfiltered calls (0.89 - 0.92 x at 128-d).
#pragma once
#include "scan_matrix_f16.hpp"
#include "scan_matrix_f32.hpp"
namespace fnv_dev {

constexpr int MB_STEPS = (int)kScanBlockSpanSteps;  // MFMA steps of a row at most: a tile's A operand stays in registers

// (two wavefronts per SIMD: 256 registers each)
template <typename T, int METRIC>
__global__ __launch_bounds__(WAVE* kScanBlockMaxWaves) __attribute__((amdgpu_waves_per_eu(2))) void exhaustive_scan_matrix_block_kernel(
    const ScanMatrixBlockParams kp) {
  const ScanParams& p = kp;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool F32 = std::is_same<T, float>::value, L2 = METRIC == FNV_METRIC_L2;
  constexpr uint32_t CPS = F32 ? 4u : 2u;  // chunks per MFMA step (sixteen elements)
  constexpr int NH = F32 ? 2 : 1;          // 16-byte requests per lane and step
  const int lane = (int)(threadIdx.x & (WAVE - 1)), col = lane & (MF_N - 1), half = lane >> 5;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const uint32_t W = kp.waves, wsub = kp.wave_subtiles;
  const uint32_t tile = blockIdx.x % p.tiles, seg = blockIdx.x / p.tiles;
  const uint32_t wq = wsub * MF_N;                                   // queries a wavefront owns at most
  const uint32_t tq0 = tile * p.tile_queries;                        // the tile's first query
  const uint32_t nqt = min(p.tile_queries, p.nq - tq0);              // ... and how many it has
  const uint32_t nqw = nqt > wave * wq ? min(wq, nqt - wave * wq) : 0u;  // this wavefront's queries: q0 ... q0 + nqw - 1
  const uint32_t q0 = tq0 + wave * wq;
  const uint32_t nsub = (nqw + MF_N - 1) / MF_N;
  const int K = (int)p.K;
  // (a float16 row with a side table has thirteen steps or more: it never gets here)
  const uint32_t nchunks = p.nchunks, tc = F32 ? p.tail_chunks : 0u, C = nchunks + tc, dim = p.dim;
  const int S = (int)((C + CPS - 1u) / CPS);  // <= MB_STEPS (the planner)
  const uint32_t P = 16u * (uint32_t)S;
  const uint32_t per_query = (uint32_t)S * 32u + p.K * 8u + 8u;
  unsigned char* const mine_lds = smem + (size_t)wave * wq * per_query;                            // this wavefront's part
  uint4* const qlds = reinterpret_cast<uint4*>(mine_lds);                                          // [wsub][S][64]
  uint64_t* const lists = reinterpret_cast<uint64_t*>(mine_lds + (size_t)wq * (uint32_t)S * 32u);  // [wq][K]
  float2* const qterm = reinterpret_cast<float2*>(mine_lds + (size_t)wq * ((uint32_t)S * 32u + p.K * 8u));  // [wq] {qn, margin term}
  unsigned char* const ring = smem + (size_t)p.tile_queries * per_query;
  const uint32_t buffer_bytes = scan_block_buffer_bytes((uint32_t)S);
  const auto ring_data = [&](uint64_t u) { return reinterpret_cast<uint4*>(ring + (size_t)(u % kScanBlockRing) * buffer_bytes); };  // [S][64]
  const auto ring_terms = [&](uint64_t u) { return reinterpret_cast<float2*>(ring + (size_t)(u % kScanBlockRing) * buffer_bytes + (uint32_t)S * 1024u); };  // [32]
  const auto ring_ids = [&](uint64_t u) { return reinterpret_cast<uint32_t*>(ring + (size_t)(u % kScanBlockRing) * buffer_bytes + (uint32_t)S * 1024u + 256u); };  // [32]
  const auto query_of = [&](uint32_t qq) { return q0 + qq; };
  const auto row_term = [&](float n) {
    if constexpr (F32) return scan_margin_f32_term(P, n, !L2);
    else return scan_margin_term(P, n);
  };

  // ---- this wavefront's queries in operand order (zero beyond dim and beyond its last query), their norms and margin terms,
  // its lists: scan_matrix_f16.hpp's / scan_matrix_f32.hpp's staging on q0 ... (a wavefront without queries stages nothing)
  [[maybe_unused]] const float* const queries32 = reinterpret_cast<const float*>(p.queries) + (uint64_t)q0 * dim;
  for (uint32_t i = lane; i < nsub * (uint32_t)S * 64u; i += WAVE) {
    const uint32_t l = i & 63u, st = i >> 6, s = st % (uint32_t)S, t = st / (uint32_t)S;
    const uint32_t qq = t * MF_N + (l & 31u);
    if constexpr (F32) {
      const uint32_t e0 = 16u * s + 8u * (l >> 5);
      uint32_t w[8];
#pragma unroll
      for (uint32_t e = 0; e < 8u; e++) w[e] = qq < nqw && e0 + e < dim ? __float_as_uint(queries32[(uint64_t)qq * dim + e0 + e]) : 0u;
      const mf32_u32x4 x = mf32_narrow8(mf32_u32x4{w[0], w[1], w[2], w[3]}, mf32_u32x4{w[4], w[5], w[6], w[7]});
      qlds[i] = make_uint4(x[0], x[1], x[2], x[3]);
    } else {
      const uint32_t c = 2u * s + (l >> 5);
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (qq < nqw && c < C) {
        const uint16_t* qsrc = reinterpret_cast<const uint16_t*>(p.queries) + (uint64_t)(q0 + qq) * dim;
#pragma unroll
        for (uint32_t e = 0; e < 8u; e++) {
          const uint32_t at = c * 8u + e;
          const uint32_t b = at < dim ? qsrc[at] : 0u;
          w[e >> 1] |= b << (16u * (e & 1u));
        }
      }
      qlds[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  for (uint32_t i = lane; i < nqw * p.K; i += WAVE) lists[i] = SCAN_PAD;
  wave_sync();
  for (uint32_t qq = lane; qq < nsub * MF_N; qq += WAVE) {
    float qn = 0.f;
    if constexpr (F32) {
      if (qq < nqw)
        for (uint32_t e = 0; e < dim; e++) {
          const float x = queries32[(uint64_t)qq * dim + e];
          qn = __builtin_fmaf(x, x, qn);
        }
    } else {
      const uint32_t t = qq / MF_N, j = qq % MF_N;
      f32x2 acc = {0.f, 0.f};
      for (uint32_t c = 0; c < 2u * (uint32_t)S; c++) acc = mf_squares(acc, qlds[(t * (uint32_t)S + (c >> 1)) * 64u + (c & 1u) * 32u + j]);
      qn = acc.x + acc.y;
    }
    qterm[qq] = make_float2(qn, row_term(qn));
  }
  wave_sync();

  // ---- the block's share of the candidates: slots [lo, hi) of the id list, 32 rows a tile.  Everything here is the same in
  // every wavefront of the block: the walk's barrier stands on it.
  const uint64_t ncand = (uint64_t)*p.cand_count;
  const uint64_t lo = ncand * seg / p.segments, hi = ncand * (seg + 1) / p.segments;
  const uint64_t tiles = (hi - lo + MF_N - 1) / MF_N;

  // ---- loading.  This wavefront's next row tile, its requests in `raw`.
  mf_u32x4 raw[MB_STEPS][NH];
  uint64_t my_tile = wave;
  uint32_t my_id = 0;
  bool my_valid = false;
  // The requests of my_tile: no branch on loaded data and no use of it, so they stay in flight.  A lane without a row reads row
  // 0, a chunk at or past C reads chunk 0: legal addresses whose data hand_over discards or no MFMA step takes.
  const auto request = [&]() __attribute__((always_inline)) {
    if (my_tile >= tiles) return;  // (wave-uniform)
    const uint64_t slot = lo + my_tile * MF_N + (uint64_t)col;
    my_valid = slot < hi;
    my_id = my_valid ? p.cand_ids[slot] : 0u;
    const uint8_t* const rowp = p.vectors + (uint64_t)my_id * p.row_bytes;
    const uint8_t* const tailp = p.tails + (uint64_t)my_id * tc * 16u;
#pragma unroll
    for (int s = 0; s < MB_STEPS; s++) {
#pragma unroll
      for (int h = 0; h < NH; h++) {
        const uint32_t c = CPS * (uint32_t)s + (CPS / 2u) * (uint32_t)half + (uint32_t)h, cc = c < C ? c : 0u;
        raw[s][h] = *reinterpret_cast<const mf_u32x4*>(cc < nchunks ? rowp + cc * 16u : tailp + (cc - nchunks) * 16u);
      }
    }
  };
  // my_tile into its ring buffer (the caller knows the buffer is free), then on to this wavefront's next tile and its requests
  const auto hand_over = [&]() __attribute__((always_inline)) {
    uint4* const data = ring_data(my_tile);
    f32x2 squares = {0.f, 0.f};  // the squares of the lane's chunks of its row
#pragma unroll
    for (int s = 0; s < MB_STEPS; s++) {
      if (s < S) {
        mf_u32x4 x[NH];
#pragma unroll
        for (int h = 0; h < NH; h++) {
          const bool ok = my_valid && CPS * (uint32_t)s + (CPS / 2u) * (uint32_t)half + (uint32_t)h < C;
#pragma unroll
          for (int k = 0; k < 4; k++) x[h][k] = ok ? raw[s][h][k] : 0u;
          if constexpr (F32) squares = mf32_squares(squares, x[h]);
          else squares = mf_squares(squares, make_uint4(x[h][0], x[h][1], x[h][2], x[h][3]));
        }
        mf_u32x4 a;
        if constexpr (F32) a = mf32_narrow8(x[0], x[NH - 1]);
        else a = x[0];
        data[s * WAVE + lane] = make_uint4(a[0], a[1], a[2], a[3]);
      }
    }
    float rn = squares.x + squares.y;  // the row's norm and its share of the margin, once
    rn += __shfl_xor(rn, 32, WAVE);
    if (half == 0) {
      ring_terms(my_tile)[col] = make_float2(rn, row_term(rn));
      ring_ids(my_tile)[col] = my_id;
    }
    my_tile += W;
    request();
  };

  // ---- scoring: this wavefront's sub-tiles against row tile u
  unsigned long long scored = 0, rescored = 0;  // (wave-uniform) this wavefront's pairs
  const auto score_tile = [&](uint64_t u) __attribute__((always_inline)) {
    if (nsub == 0u) return;  // (wave-uniform; the barrier is the caller's)
    const uint4* const data = ring_data(u);
    mf_u32x4 a[MB_STEPS];
#pragma unroll
    for (int s = 0; s < MB_STEPS; s++) {
      if (s < S) {
        const uint4 x = data[s * WAVE + lane];
        a[s] = mf_u32x4{x.x, x.y, x.z, x.w};
      }
    }
    const uint32_t nrows = (uint32_t)min((uint64_t)MF_N, hi - (lo + u * MF_N));
    const float2* const terms = ring_terms(u);
    const uint32_t id = ring_ids(u)[col];
    float rv[16], rt[16];  // the norms and margin terms of the sixteen rows this lane's accumulators belong to
#pragma unroll
    for (int v = 0; v < 16; v++) {
      const float2 r = terms[mf_row(v, half)];
      rv[v] = r.x;
      rt[v] = r.y;
    }
    for (uint32_t t = 0; t < nsub; t++) {
      mf_f32x16 acc = {0};
      const uint4* const qsub = qlds + (size_t)t * (uint32_t)S * 64u;
#pragma unroll
      for (int s = 0; s < MB_STEPS; s++) {
        if (s < S) {
          const uint4 x = qsub[(size_t)s * 64u + lane];
          const mf_u32x4 b = mf_u32x4{x.x, x.y, x.z, x.w};
          if constexpr (F32)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mf32_bf16x8, a[s]), __builtin_bit_cast(mf32_bf16x8, b), acc, 0, 0, 0);
          else
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(mf_f16x8, a[s]), __builtin_bit_cast(mf_f16x8, b), acc, 0, 0, 0);
        }
      }
      // the lane's query: its norm, its margin term and its K-th exact distance so far (an empty slot: +inf)
      const uint32_t qq = t * MF_N + (uint32_t)col;
      const bool has_query = qq < nqw;
      const float2 qt = qterm[qq];
      float kd = std::numeric_limits<float>::infinity();
      if (has_query) {
        const uint64_t kth = lists[(size_t)qq * K + (K - 1)];
        if (kth != SCAN_PAD) kd = __uint_as_float(scan_key_dist_bits(kth));
      }
      uint32_t mine = 0;  // bit v: the pair (this lane's query, row mf_row(v, half)) survives
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const float score = L2 ? (rv[v] + qt.x) - 2.0f * acc[v] : 1.0f - acc[v];
        const float bound = score - scan_margin_of_terms(rt[v], qt.y, !L2);
        bool drop = bound > kd;  // (a NaN anywhere: survives)
        if constexpr (F32) drop = drop && bound <= std::numeric_limits<float>::max();  // (float32: an infinity as well)
        const bool survives = has_query && mf_row(v, half) < nrows && !drop;
        mine |= (survives ? 1u : 0u) << v;
      }
      scored += (unsigned long long)nrows * min((uint32_t)MF_N, nqw - t * MF_N);
      if (__ballot(mine != 0u)) {  // about K ln(n / K) rows per query, and what the margin adds
        uint64_t* const sublists = lists + (size_t)t * MF_N * K;
        uint32_t n = 0;
        if constexpr (F32) {
          const float* const qfirst = queries32 + (uint64_t)t * MF_N * dim;
          const auto query_at = [&](uint32_t j) { return qfirst + (uint64_t)j * dim; };
          switch (kp.group_lanes) {  // the row configurations of float32 rows (search_types.h, kCfgs)
            case 8: n = mf32_rescore<METRIC, 8>(p, query_at, sublists, mine, id, lane); break;
            case 16: n = mf32_rescore<METRIC, 16>(p, query_at, sublists, mine, id, lane); break;
            case 32: n = mf32_rescore<METRIC, 32>(p, query_at, sublists, mine, id, lane); break;
            default: n = mf32_rescore<METRIC, 64>(p, query_at, sublists, mine, id, lane); break;
          }
        } else {
          switch (kp.group_lanes) {  // the row configurations of float16 rows
            case 8: n = mf_rescore<METRIC, 8>(p, qsub, sublists, mine, id, lane); break;
            case 16: n = mf_rescore<METRIC, 16>(p, qsub, sublists, mine, id, lane); break;
            case 32: n = mf_rescore<METRIC, 32>(p, qsub, sublists, mine, id, lane); break;
            default: n = mf_rescore<METRIC, 64>(p, qsub, sublists, mine, id, lane); break;
          }
        }
        rescored += n;
      }
    }
  };

  // ---- the walk.  Every wavefront has its first tile under way; tile 0 is handed over before the first barrier.  `tiles`, and
  // with it every trip of this loop and every barrier, is the same in all wavefronts of the block.
  request();
  if (wave == 0u && tiles != 0u) hand_over();
  __syncthreads();
  for (uint64_t u = 0; u < tiles; u++) {
    score_tile(u);
    if (my_tile == u + 1u && my_tile < tiles) hand_over();  // (wave-uniform) into the buffer tile u - 1 has left
    __syncthreads();
  }

  // ---- the block's counters (the ring is free: the last barrier is behind every read of it), this wavefront's lists
  unsigned long long* const pairs = reinterpret_cast<unsigned long long*>(ring);  // [W][2]
  if (lane == 0) {
    pairs[2u * wave] = scored;
    pairs[2u * wave + 1u] = rescored;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0, b = 0;
    for (uint32_t w = 0; w < W; w++) {
      a += pairs[2u * w];
      b += pairs[2u * w + 1u];
    }
    atomicAdd(kp.counters, a);
    atomicAdd(kp.counters + 1, b);
  }
  scan_flush_tile(p, lists, nqw, seg, lane, query_of);
}

}  // namespace fnv_dev
