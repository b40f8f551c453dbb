// scan.hpp -- part of the gfx950 search engine (device code; included by kernel_inst.hip's `scan` units and by launch.hip).
// The EXHAUSTIVE search (fnv_search_batch_exhaustive): the exact K nearest among the live nodes, or among the allowed ones.
//
//   1. filtered calls: node_filter_kernel (launch.hip) turns the label bitmap into a node bitmap, exhaustive_compact_kernel
//      turns that into the list of allowed node ids (any order: the selection's order is total, scan_select.hpp).
//   2. exhaustive_scan_kernel, one wavefront per (query tile, row segment): the tile's queries are staged in LDS
//      (scan_stage_tile), a lane group loads the chunks of PU rows into registers ONCE and scores them against every query of
//      the tile -- the row traffic of a launch is  ceil(nq / tile) * candidates * row_bytes  instead of
//      nq * candidates * row_bytes.  Per (query, row) the arithmetic is batch_dists' (distance.hpp): lane g of the row's group
//      accumulates chunks g, g + G, ... in that order with Dist<T, METRIC>, group_sum adds the lanes -- so a distance has the
//      bits the graph search reports for the same pair.  Every query keeps a sorted list of its K best keys in LDS; a row that
//      does not beat the K-th is dropped by one compare, one that does (about K ln(n / K) per query) is inserted by the whole
//      wave.  The lists go out per segment (scan_flush_tile).
//   3. exhaustive_merge_kernel, one wavefront per query: the segments' lists merged by rank (scan_select.hpp), keys back to
//      (distance, label), padding, counters.
// With one filter per query (fnv_search_batch_exhaustive_grouped) step 2 is exhaustive_scan_grouped_kernel: the same staging
// and flushing around a walk of the tile's filter row; its batches are scored by scan_score_batch, a copy of step 2's loop.
// A routed filtered graph search (scan_select.hpp, "filter routing") runs that grouped form as its second stage, on the queries
// whose route word is set: route_queries_kernel, group_rows_routed_kernel and exhaustive_merge_routed_kernel below.
#pragma once
#include "distance.hpp"
#include "heaps.hpp"
#include "scan_select.hpp"
namespace fnv_dev {

// key into the sorted list[0, K) (wave-uniform arguments; the caller has checked key < list[K - 1]): the last entry falls out
__device__ __forceinline__ void scan_insert(uint64_t* list, int K, uint64_t key, int lane) {
  const int pos = (int)scan_lower_bound(list, (uint32_t)K, key);
  for (int top = K - 1; top > pos; top -= WAVE) {  // entries (max(pos, top - 64), top] move up by one, the highest first
    const int j = top - lane;
    const bool act = j > pos;
    uint64_t e = 0;
    if (act) e = list[j - 1];
    wave_sync();
    if (act) list[j] = e;
    wave_sync();
  }
  if (lane == 0) list[pos] = key;
  wave_sync();
}

// The tile's queries into LDS, zero padded to q_chunks, and every list empty.  query_of(qq): the global query of tile slot qq.
template <typename T, typename F>
__device__ __forceinline__ void scan_stage_tile(const ScanParams& p, uint4* qlds, uint64_t* lists, uint32_t nqb, int lane, F query_of) {
  const int padded = (int)(p.q_chunks * 16u / sizeof(T));
  const int dim = (int)p.dim;
  for (uint32_t qq = 0; qq < nqb; qq++) {
    const T* qsrc = reinterpret_cast<const T*>(p.queries) + (uint64_t)query_of(qq) * p.dim;
    T* qdst = reinterpret_cast<T*>(qlds + (size_t)qq * p.q_chunks);
    for (int i = lane; i < padded; i += WAVE) qdst[i] = i < dim ? qsrc[i] : T(0);
  }
  for (uint32_t i = lane; i < nqb * p.K; i += WAVE) lists[i] = SCAN_PAD;
  wave_sync();
}
// ... and the tile's lists out to the partial lists of segment `seg`
template <typename F>
__device__ __forceinline__ void scan_flush_tile(const ScanParams& p, const uint64_t* lists, uint32_t nqb, uint32_t seg, int lane, F query_of) {
  wave_sync();
  for (uint32_t i = lane; i < nqb * p.K; i += WAVE) {
    const uint32_t qq = i / p.K, k = i % p.K;
    p.partial[((uint64_t)query_of(qq) * p.segments + seg) * (uint64_t)p.K + k] = lists[i];
  }
}

// One wavefront per (query tile, row segment): the tile's queries staged, the segment's candidates -- the live nodes, or the
// compacted ids of the allowed ones -- scored VPW * PU at a time, by the kernel's own loop (see scan_score_batch below).
template <typename T, int METRIC, int G, int CU, bool FULL>
__global__ __launch_bounds__(WAVE) void exhaustive_scan_kernel(const ScanParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int PU = passes<G, CU>();
  constexpr int VPW = WAVE / G;
  constexpr int SPAN = G * CU;
  constexpr bool TAIL = row_has_tail<G, CU, FULL>();
  typedef Dist<T, METRIC> D;
  typedef typename D::acc_t acc_t;
  const int lane = threadIdx.x, g = lane % G, v = lane / G;
  const uint32_t tile = blockIdx.x % p.tiles, seg = blockIdx.x / p.tiles;
  const uint32_t q0 = tile * p.tile_queries;
  const uint32_t nqb = min(p.tile_queries, p.nq - q0);
  uint4* const qlds = reinterpret_cast<uint4*>(smem);                                                     // [tile][q_chunks]
  uint64_t* const lists = reinterpret_cast<uint64_t*>(smem + (size_t)p.tile_queries * p.q_chunks * 16u);  // [tile][K]
  const int K = (int)p.K;
  const uint32_t q_chunks = p.q_chunks;
  const int nchunks = (int)p.nchunks;
  const auto query_of = [&](uint32_t qq) { return q0 + qq; };
  scan_stage_tile<T>(p, qlds, lists, nqb, lane, query_of);

  // this block's share of the candidates
  const uint64_t ncand = p.cand_ids ? (uint64_t)*p.cand_count : p.n_live;
  const uint64_t lo = ncand * seg / p.segments, hi = ncand * (seg + 1) / p.segments;
  const bool one_span = nchunks <= SPAN;  // (every row configuration but rows beyond 4 KB)
  const uint32_t tc = p.tail_chunks;

  for (uint64_t base = lo; base < hi; base += VPW * PU) {
    uint32_t id[PU];
    bool val[PU];
    const uint8_t* rowp[PU];
#pragma unroll
    for (int pu = 0; pu < PU; pu++) {  // lanes past the end re-read the last candidate; their results are ignored
      const uint64_t slot = base + (uint64_t)(pu * VPW + v);
      val[pu] = slot < hi;
      const uint64_t idx = val[pu] ? slot : hi - 1;
      id[pu] = p.cand_ids ? p.cand_ids[idx] : (uint32_t)idx;
      rowp[pu] = p.vectors + (uint64_t)id[pu] * p.row_bytes;
    }
    uint4 y[PU][CU], yt[PU];
    // lane g's chunks c0 + g, c0 + G + g, ... of every row of the batch; zero beyond the row (the staged query is zero there too)
    auto load_span = [&](int c0) {
#pragma unroll
      for (int pu = 0; pu < PU; pu++) {
#pragma unroll
        for (int cu = 0; cu < CU; cu++) {
          const int c = c0 + cu * G + g;
          y[pu][cu] = make_uint4(0u, 0u, 0u, 0u);
          if (FULL || TAIL || c < nchunks) y[pu][cu] = *reinterpret_cast<const uint4*>(rowp[pu] + (uint32_t)c * 16u);
        }
      }
    };
    if (one_span) load_span(0);
    if constexpr (TAIL) {  // split rows: chunk 24 + g from the side table
#pragma unroll
      for (int pu = 0; pu < PU; pu++) {
        yt[pu] = make_uint4(0u, 0u, 0u, 0u);
        if ((uint32_t)g < tc) yt[pu] = *reinterpret_cast<const uint4*>(p.tails + ((uint64_t)id[pu] * tc + (uint32_t)g) * 16u);
      }
    }

    for (uint32_t qq = 0; qq < nqb; qq++) {
      const uint4* qv = qlds + (size_t)qq * q_chunks;
      acc_t acc[PU];
      typename D::qacc_t qacc = D::qzero();
#pragma unroll
      for (int pu = 0; pu < PU; pu++) acc[pu] = D::zero();
      for (int c0 = 0; c0 < nchunks; c0 += SPAN) {
        if (!one_span) load_span(c0);
#pragma unroll
        for (int cu = 0; cu < CU; cu++) {
          const uint4 x = qv[c0 + cu * G + g];
          qacc = D::qchunk(qacc, x);
#pragma unroll
          for (int pu = 0; pu < PU; pu++) acc[pu] = D::chunk(acc[pu], x, y[pu][cu]);
        }
      }
      if constexpr (TAIL) {
        const uint4 xt = qv[SPAN + g];
        qacc = D::qchunk(qacc, xt);
#pragma unroll
        for (int pu = 0; pu < PU; pu++) acc[pu] = D::chunk(acc[pu], xt, yt[pu]);
      }
      uint64_t* const list = lists + (size_t)qq * K;
      uint64_t kth = list[K - 1];  // one address for the wave: a broadcast read
#pragma unroll
      for (int pu = 0; pu < PU; pu++) {
        const float d = D::finish(group_sum<G>(D::lane_sum(acc[pu], qacc)));
        const uint64_t key = scan_key(__float_as_uint(d), id[pu]);
        unsigned long long pm = __ballot(g == 0 && val[pu] && scan_key_less(key, kth));
        while (pm) {  // rare: about K ln(n / K) rows per query ever get here
          const int i = __ffsll((long long)pm) - 1;
          pm &= pm - 1;
          const uint64_t k = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), i) << 32) |
                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, i);
          if (scan_key_less(k, kth)) {
            scan_insert(list, K, k, lane);
            kth = list[K - 1];
          }
        }
      }
    }
  }
  scan_flush_tile(p, lists, nqb, seg, lane, query_of);
}

// ---- grouped filters: one allowed set per query (fnv_search_batch_exhaustive_grouped) --------------------------------------
// One batch of VPW * PU queued node ids against the tile's nqb staged queries: exhaustive_scan_kernel's loop body -- the same
// loads, the same per-lane chunk order, group_sum, scan_key and scan_insert, so a distance has the same bits -- with the ids
// taken from ids[0, nvalid) (LDS) instead of a compacted list; slots from nvalid on repeat the last valid id with val = false.
// (A copy, not a shared body: with the body shared, the plain scan's small launches -- a hundred queries on 1 % of the rows --
// measured 0.7 % slower, profiles/exhaustive.md.  Only the GPU tests hold the two bodies to the same bits: ANY change to the
// scoring of either must be made in both.)
template <typename T, int METRIC, int G, int CU, bool FULL>
__device__ __forceinline__ void scan_score_batch(const ScanParams& p, const uint4* qlds, uint64_t* lists, uint32_t nqb,
                                                 const uint32_t* ids, uint32_t nvalid, int lane) {
  constexpr int PU = passes<G, CU>();
  constexpr int VPW = WAVE / G;
  constexpr int SPAN = G * CU;
  constexpr bool TAIL = row_has_tail<G, CU, FULL>();
  typedef Dist<T, METRIC> D;
  typedef typename D::acc_t acc_t;
  const int g = lane % G, v = lane / G;
  const int K = (int)p.K;
  const uint32_t q_chunks = p.q_chunks;
  const int nchunks = (int)p.nchunks;
  const bool one_span = nchunks <= SPAN;
  const uint32_t tc = p.tail_chunks;
  uint32_t id[PU];
  bool val[PU];
  const uint8_t* rowp[PU];
#pragma unroll
  for (int pu = 0; pu < PU; pu++) {
    const uint32_t slot = (uint32_t)(pu * VPW + v);
    val[pu] = slot < nvalid;
    id[pu] = ids[val[pu] ? slot : nvalid - 1u];
    rowp[pu] = p.vectors + (uint64_t)id[pu] * p.row_bytes;
  }
  uint4 y[PU][CU], yt[PU];
  auto load_span = [&](int c0) {
#pragma unroll
    for (int pu = 0; pu < PU; pu++) {
#pragma unroll
      for (int cu = 0; cu < CU; cu++) {
        const int c = c0 + cu * G + g;
        y[pu][cu] = make_uint4(0u, 0u, 0u, 0u);
        if (FULL || TAIL || c < nchunks) y[pu][cu] = *reinterpret_cast<const uint4*>(rowp[pu] + (uint32_t)c * 16u);
      }
    }
  };
  if (one_span) load_span(0);
  if constexpr (TAIL) {
#pragma unroll
    for (int pu = 0; pu < PU; pu++) {
      yt[pu] = make_uint4(0u, 0u, 0u, 0u);
      if ((uint32_t)g < tc) yt[pu] = *reinterpret_cast<const uint4*>(p.tails + ((uint64_t)id[pu] * tc + (uint32_t)g) * 16u);
    }
  }
  for (uint32_t qq = 0; qq < nqb; qq++) {
    const uint4* qv = qlds + (size_t)qq * q_chunks;
    acc_t acc[PU];
    typename D::qacc_t qacc = D::qzero();
#pragma unroll
    for (int pu = 0; pu < PU; pu++) acc[pu] = D::zero();
    for (int c0 = 0; c0 < nchunks; c0 += SPAN) {
      if (!one_span) load_span(c0);
#pragma unroll
      for (int cu = 0; cu < CU; cu++) {
        const uint4 x = qv[c0 + cu * G + g];
        qacc = D::qchunk(qacc, x);
#pragma unroll
        for (int pu = 0; pu < PU; pu++) acc[pu] = D::chunk(acc[pu], x, y[pu][cu]);
      }
    }
    if constexpr (TAIL) {
      const uint4 xt = qv[SPAN + g];
      qacc = D::qchunk(qacc, xt);
#pragma unroll
      for (int pu = 0; pu < PU; pu++) acc[pu] = D::chunk(acc[pu], xt, yt[pu]);
    }
    uint64_t* const list = lists + (size_t)qq * K;
    uint64_t kth = list[K - 1];
#pragma unroll
    for (int pu = 0; pu < PU; pu++) {
      const float d = D::finish(group_sum<G>(D::lane_sum(acc[pu], qacc)));
      const uint64_t key = scan_key(__float_as_uint(d), id[pu]);
      unsigned long long pm = __ballot(g == 0 && val[pu] && scan_key_less(key, kth));
      while (pm) {
        const int i = __ffsll((long long)pm) - 1;
        pm &= pm - 1;
        const uint64_t k = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), i) << 32) |
                           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, i);
        if (scan_key_less(k, kth)) {
          scan_insert(list, K, k, lane);
          kth = list[K - 1];
        }
      }
    }
  }
}

// One wavefront per (tile descriptor, row segment).  The tile's queries all use one filter row; the block walks that row's
// words over its segment of [0, live_words), 64 words a step, and turns set bits into node ids in an LDS queue: a wave prefix
// over the words' popcounts gives every lane the place of its word's ids, the words that fit the queue's free room (a prefix of
// the lanes) are appended, full batches are scored, what is left moves to the queue's front, until the step's words are used
// up.  The last short batch is scored after the last word.  Which batch a node falls into never shows: the order is total.
// LDS: the plain scan's [tile][q_chunks] queries and [tile][K] lists, then SCAN_QUEUE_IDS ids.
template <typename T, int METRIC, int G, int CU, bool FULL>
__global__ __launch_bounds__(WAVE) void exhaustive_scan_grouped_kernel(const GroupedScanParams gp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t BATCH = (uint32_t)(passes<G, CU>() * (WAVE / G));
  static_assert(BATCH - 1u + 32u <= SCAN_QUEUE_IDS && BATCH <= (uint32_t)WAVE, "a word always fits behind the leftovers");
  const ScanParams& p = gp.s;
  const int lane = threadIdx.x;
  const uint32_t seg = blockIdx.x / p.tiles;
  const GroupTile t = gp.tiles[blockIdx.x % p.tiles];
  const uint32_t nqb = t.count;
  if (nqb == 0u) return;  // (past the real tiles: the launch is an upper bound)
  uint4* const qlds = reinterpret_cast<uint4*>(smem);
  uint64_t* const lists = reinterpret_cast<uint64_t*>(smem + (size_t)p.tile_queries * p.q_chunks * 16u);
  uint32_t* const queue = reinterpret_cast<uint32_t*>(lists + (size_t)p.tile_queries * p.K);
  const uint32_t* const perm = gp.perm + t.first;
  const auto query_of = [&](uint32_t qq) { return perm[qq]; };
  scan_stage_tile<T>(p, qlds, lists, nqb, lane, query_of);
  const uint32_t* const bits = gp.node_bits + (uint64_t)t.row * gp.row_words;
  const uint32_t wlo = (uint32_t)((uint64_t)gp.live_words * seg / p.segments);
  const uint32_t whi = (uint32_t)((uint64_t)gp.live_words * (seg + 1) / p.segments);
  uint32_t count = 0;  // ids in the queue (wave-uniform)
  for (uint32_t w0 = wlo; w0 < whi; w0 += WAVE) {
    const uint32_t w = w0 + (uint32_t)lane;
    uint32_t word = w < whi ? bits[w] : 0u;
    while (__ballot(word != 0u)) {
      const uint32_t pc = (uint32_t)__popc(word);
      uint32_t incl = pc;  // ids of lanes [0, lane]
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, WAVE);
        if (lane >= off) incl += up;
      }
      const bool fits = count + incl <= SCAN_QUEUE_IDS;  // (incl never decreases along the lanes: a prefix of them)
      const int nfit = __popcll(__ballot(fits));          // >= 1 word with ids: count < BATCH here
      if (fits) {
        uint32_t at = count + incl - pc;
        while (word) {
          queue[at++] = w * 32u + (uint32_t)(__ffs((int)word) - 1);
          word &= word - 1u;
        }
      }
      count += (uint32_t)__shfl((int)incl, nfit - 1, WAVE);
      wave_sync();
      uint32_t head = 0;
      for (; count - head >= BATCH; head += BATCH)
        scan_score_batch<T, METRIC, G, CU, FULL>(p, qlds, lists, nqb, queue + head, BATCH, lane);
      if (head) {  // the leftovers (fewer than a batch) to the front
        const uint32_t rem = count - head;
        uint32_t keep = 0;
        if ((uint32_t)lane < rem) keep = queue[head + lane];
        wave_sync();
        if ((uint32_t)lane < rem) queue[lane] = keep;
        wave_sync();
        count = rem;
      }
    }
  }
  if (count) scan_score_batch<T, METRIC, G, CU, FULL>(p, qlds, lists, nqb, queue, count, lane);
  scan_flush_tile(p, lists, nqb, seg, lane, query_of);
}

#ifndef FNV_INST_FAMILY  // (the kernels below are not templates: launch.hip alone emits them, not kernel_inst.hip's units)
// The allowed node ids of a node bitmap (bit i & 31 of word i >> 5), compacted wave by wave: the order is whatever the
// atomics make it, which the selection does not see.  *count must be zero at launch; ids holds n_live entries.
static __global__ __launch_bounds__(256) void exhaustive_compact_kernel(const uint32_t* node_bits, uint64_t n_live, uint32_t* ids,
                                                                        uint32_t* count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < n_live && ((node_bits[i >> 5] >> (i & 31)) & 1u);
  const unsigned long long m = __ballot(ok);
  if (m == 0ull) return;
  const int lane = (int)(threadIdx.x & (WAVE - 1));
  uint32_t first = 0;
  if (lane == __ffsll((long long)m) - 1) first = atomicAdd(count, (uint32_t)__popcll(m));
  first = (uint32_t)__shfl((int)first, __ffsll((long long)m) - 1, WAVE);
  if (ok) ids[first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;
}

// One wavefront per query: its `segments` sorted lists -> the K first of their union -> the caller's arrays.
// LDS: three lists of K keys.  `candidates()`: how many the query had (out_count / out_ndist), read once the lists are merged.
template <typename F>
__device__ __forceinline__ void scan_merge_query(const ScanParams& p, unsigned char* smem, F candidates) {
  const int lane = threadIdx.x;
  const uint32_t q = blockIdx.x, K = p.K;
  uint64_t* a = reinterpret_cast<uint64_t*>(smem);
  uint64_t* b = a + K;
  uint64_t* const c = b + K;
  const uint64_t* part = p.partial + (uint64_t)q * p.segments * K;
  for (uint32_t i = lane; i < K; i += WAVE) a[i] = part[i];
  wave_sync();
  for (uint32_t s = 1; s < p.segments; s++) {
    const uint64_t* src = part + (uint64_t)s * K;
    if (!scan_key_less(src[0], a[K - 1])) continue;  // (wave-uniform) nothing of this segment ranks before the K-th so far
    for (uint32_t i = lane; i < K; i += WAVE) c[i] = src[i];
    wave_sync();
    for (uint32_t i = lane; i < K; i += WAVE) {
      const uint64_t ka = a[i], kc = c[i];
      const uint32_t pa = scan_merge_pos_a(i, ka, c, K), pc = scan_merge_pos_b(i, kc, a, K);
      if (pa < K) b[pa] = ka;
      if (pc < K) b[pc] = kc;
    }
    wave_sync();
    uint64_t* t = a;
    a = b;
    b = t;
  }
  const uint64_t ncand = candidates();
  for (uint32_t k = lane; k < K; k += WAVE) {
    const uint64_t key = a[k];
    float od = std::numeric_limits<float>::infinity();
    int32_t ol = -1;
    if (key != SCAN_PAD) {
      od = __uint_as_float(scan_key_dist_bits(key));
      const uint32_t node = scan_key_node(key);
      ol = p.labels ? p.labels[node] : (int32_t)node;
    }
    p.out_dist[(uint64_t)q * K + k] = od;
    p.out_labels[(uint64_t)q * K + k] = ol;
  }
  if (lane == 0) {
    if (p.out_count) p.out_count[q] = (int32_t)(ncand < (uint64_t)K ? ncand : (uint64_t)K);
    if (p.out_ndist) p.out_ndist[q] = ncand;
  }
}
static __global__ __launch_bounds__(WAVE) void exhaustive_merge_kernel(const ScanParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  scan_merge_query(p, smem, [&] { return p.cand_ids ? (uint64_t)*p.cand_count : p.n_live; });
}
// ... of a grouped launch: the candidates of a query are the nodes set in its filter row.
static __global__ __launch_bounds__(WAVE) void exhaustive_merge_grouped_kernel(const GroupedScanParams gp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  scan_merge_query(gp.s, smem, [&] { return (uint64_t)gp.row_count[gp.query_row[blockIdx.x]]; });
}
// ... of a routed filtered graph search (scan_select.hpp, "filter routing"): one block per query of the call; only a query whose
// route word is set has partial lists, and its n_hops = 0 tells its row from a graph search's.
static __global__ __launch_bounds__(WAVE) void exhaustive_merge_routed_kernel(const GroupedScanParams gp, const uint32_t* route,
                                                                              uint64_t* out_nhops) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (route[blockIdx.x] == ROUTE_GRAPH) return;  // (uniform over the block)
  scan_merge_query(gp.s, smem, [&] { return (uint64_t)gp.row_count[gp.query_row[blockIdx.x]]; });
  if (threadIdx.x == 0 && out_nhops) out_nhops[blockIdx.x] = 0ull;
}

// Grouping of a grouped launch's queries by filter row, in four small steps (rows = n_filters + 2; every array uint32):
//   group_rows_kernel     query_row[q] = filter_row(query_filter[q]), counts[row]++          (counts zero at launch)
//   group_prefix_kernel   slot_start / tile_start [rows + 1]: exclusive prefixes of the counts and of ceil(count / tile)
//   group_scatter_kernel  perm: the query indices, contiguous per row, in whatever order the atomics leave inside a row
//                         (results go out at the original query index)                          (cursor zero at launch)
//   group_tiles_kernel    the `bound` tile descriptors (scan_select.hpp, group_tile_at)
// A routed filtered graph search groups the queries its scan stage answers and no others: group_rows_routed_kernel takes the
// first step's place (query_row[q] = GROUP_NO_ROW for the rest, which group_scatter_kernel passes over), the others run as they are.
static __global__ __launch_bounds__(256) void group_rows_kernel(const int32_t* query_filter, uint32_t nq, uint32_t n_filters,
                                                                uint32_t* query_row, uint32_t* counts) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint32_t r = filter_row(query_filter[q], n_filters);
  query_row[q] = r;
  atomicAdd(counts + r, 1u);
}
static __global__ __launch_bounds__(256) void group_rows_routed_kernel(const int32_t* query_filter, const uint32_t* route, uint32_t nq,
                                                                       uint32_t n_filters, uint32_t* query_row, uint32_t* counts) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint32_t r = routed_group_row(query_filter, q, n_filters, route);
  query_row[q] = r;
  if (r != GROUP_NO_ROW) atomicAdd(counts + r, 1u);
}
// The route words of a routed launch before its search kernel runs (row_count: node_filter_table_kernel's popcounts), and behind
// them, at [nq], whether the search kernel hands a query whose candidates heap overflows to the scan.
static __global__ __launch_bounds__(256) void route_queries_kernel(const int32_t* query_filter, uint32_t nq, uint32_t n_filters,
                                                                   const uint32_t* row_count, uint64_t scan_max, uint32_t on_overflow,
                                                                   uint32_t* route) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) route[q] = route_at_launch(query_filter, q, n_filters, row_count, scan_max);
  else if (q == nq) route[nq] = on_overflow;
}
static __global__ __launch_bounds__(256) void group_prefix_kernel(const uint32_t* counts, uint32_t rows, uint32_t tile,
                                                                  uint32_t* slot_start, uint32_t* tile_start) {
  __shared__ uint32_t sc[256], st[256];
  const uint32_t tid = threadIdx.x;
  uint32_t carry_c = 0, carry_t = 0;
  for (uint32_t base = 0; base < rows; base += 256u) {  // one block: 256 rows a step, Hillis-Steele inside it
    const uint32_t g = base + tid;
    const uint32_t c = g < rows ? counts[g] : 0u, t = (c + tile - 1u) / tile;
    sc[tid] = c;
    st[tid] = t;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {
      const uint32_t ac = tid >= off ? sc[tid - off] : 0u, at = tid >= off ? st[tid - off] : 0u;
      __syncthreads();
      sc[tid] += ac;
      st[tid] += at;
      __syncthreads();
    }
    if (g < rows) {
      slot_start[g] = carry_c + sc[tid] - c;
      tile_start[g] = carry_t + st[tid] - t;
    }
    carry_c += sc[255];
    carry_t += st[255];
    __syncthreads();
  }
  if (tid == 0) {
    slot_start[rows] = carry_c;
    tile_start[rows] = carry_t;
  }
}
static __global__ __launch_bounds__(256) void group_scatter_kernel(const uint32_t* query_row, uint32_t nq, const uint32_t* slot_start,
                                                                   uint32_t* cursor, uint32_t* perm) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint32_t r = query_row[q];
  if (r == GROUP_NO_ROW) return;  // (routed launches: not a query of the scan stage)
  perm[slot_start[r] + atomicAdd(cursor + r, 1u)] = q;
}
static __global__ __launch_bounds__(256) void group_tiles_kernel(const uint32_t* slot_start, const uint32_t* tile_start, uint32_t rows,
                                                                 uint32_t tile, uint32_t bound, GroupTile* tiles) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < bound) tiles[d] = group_tile_at(d, slot_start, tile_start, rows, tile);
}

#endif  // FNV_INST_FAMILY

}  // namespace fnv_dev
