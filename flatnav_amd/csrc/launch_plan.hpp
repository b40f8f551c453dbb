// launch_plan.hpp -- part of the gfx950 search engine: the launch planner, in plain C++ (no HIP header; compiles with g++).
// Everything the host decides about a search launch by arithmetic alone: the row layout, the visited-table geometry and the
// LDS layout of a query slot, the table-size ladder and its occupancy trade, the choice of kernel family and variant, one
// graph-search launch whole (shape_search: the function launch.hip launches by and the CPU test reports), K0's tile, the
// per-slot workspace, the exhaustive scan's tiles, segments, grouping arrays, routing and byte counts, the layouts fnv_tune
// tries -- and, in measurements.hpp (included below), what the adaptive choice has measured and how fnv_tune decides.  It deals in counts and option values, never in pointers.  The host units (runtime.hpp) own the HIP runtime (kernel
// pointers, occupancy queries, LDS limits, events, buffers) and hand the planner what it needs of it as a `Runtime` object:
//   int occupancy(int mode, uint32_t lds)                workgroups of MODE_*'s kernel one CU holds with `lds` bytes each (0: error)
//   const char* raise_lds_limit(int mode, uint32_t lds)  that kernel may be launched with `lds` bytes: null, or the runtime's error
// A plan that fails returns its code and says why in `err`.
// tests/test_launch_plan.py runs this header on the CPU (tests/launch_plan_harness.cpp) over far more shapes than a GPU
// suite visits.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/flatnav_hip.h"
#include "measurements.hpp"
#include "scan_select.hpp"
#include "search_types.h"

namespace fnv_dev {

inline size_t dtype_size(int dt) {
  switch (dt) {
    case FNV_DTYPE_FLOAT32: return 4;
    case FNV_DTYPE_FLOAT16: return 2;
    case FNV_DTYPE_UINT8:
    case FNV_DTYPE_INT8: return 1;
    default: return 0;
  }
}

// Everything fnv_set_option can change: one block, so that views and replicas start as exact copies of their source.
struct IndexOptions {
  int64_t visited_factor = 27, visited_slots = 0, visited_floor = 2048, occupancy_target = 13, occupancy_roomy = 9, cand_factor = 2,
          cand_slots = 0, spill_entries = 16384, blocks_per_cu = 0, visited_wide = 0,
          entry_kernel = 0, output_node_ids = 0, visited_tag_bits = 0, sorted_beam = 2,
          sorted_beam_min = 1, sorted_cand_lds = 2, sorted_tail_exact_pct = -1, beam_registers = 1,
          sorted_variant = -1, tune_layout = 1, shadow_exact = 1, tie_replay = 1, tie_log_entries = 0, visited_direct = 1,
          host_zero_copy = 1 << 20;  // (every call that fits the pinned staging buffer)
  int64_t half_rows = 1;  // searches read the half-width mirror of a float32 table while one is live (half_rows.hpp)
  int64_t overflow_list = -1;  // -1: automatic (a list in HBM only when the bitmap is larger than 512 KB)
  int64_t scan_segment_rows = 0;  // exhaustive search: candidate rows per block's segment (0: automatic)
  // Filter routing (filtered graph searches; scan_select.hpp): a query whose filter allows at most filter_scan_max live nodes
  // (0: off), or whose candidates heap overflows (filter_scan_on_overflow != 0), is answered by the exhaustive scan.
  int64_t filter_scan_max = 0, filter_scan_on_overflow = 0;
};

// What the planner reads of an index (fnv_index_s inherits it): the options, the table geometry, the device's size.
struct PlanInputs : IndexOptions {
  int dtype = FNV_DTYPE_FLOAT32;
  uint32_t M = 0, dim = 0, row_bytes = 0;
  uint32_t tail_bytes = 0;  // split rows (distance.hpp, row_layout below): bytes per row in the side table that follows the main
                            // table in d_vectors' allocation ([capacity][row_bytes] main, then [capacity][tail_bytes]); 0: one table
  uint64_t capacity = 0;  // rows the device buffers hold (>= n_nodes; grows never)
  uint64_t parent_capacity = 0;  // a view: its source's capacity (0: not a view)
  int num_cus = 0;
};

// Row stride of the vector table.  Rows are 16-byte chunks; when rounding the stride up to whole 128-byte lines costs
// at most FLATNAV_ROW_PAD_PCT (default 30) per cent of padding it is done: a 100-d float32 row (400 bytes) at a
// 16-byte stride straddles 4-5 lines (4.0 on average = the 512 bytes the padded row occupies anyway), takes the clamped
// non-FULL distance path and costs the gather ~20 % of its rate (tools/gather_bench.hip: 5.9 vs 7.1 TB/s of row bytes);
// at a 512-byte stride it is exactly four lines and whole 8-lane x 4-chunk spans.  The padding is zero in rows and in
// the staged query, so every distance keeps its bits (zeros add nothing to either partial sum).
inline uint32_t row_stride_bytes(uint32_t dim, int data_type) {
  const uint64_t rb16 = ((uint64_t)dim * dtype_size(data_type) + 15) / 16 * 16;
  const uint64_t rb128 = (rb16 + 127) / 128 * 128;
  long pct = 30;
  if (const char* env = getenv("FLATNAV_ROW_PAD_PCT")) pct = strtol(env, nullptr, 10);
  if (pct > 0 && (rb128 - rb16) * 100 <= (uint64_t)pct * rb16) return (uint32_t)rb128;
  return (uint32_t)rb16;
}

// SPLIT ROWS (round 6, distance.hpp): a row of exactly three 128-byte lines plus at most 32 bytes (d = 97 ... 104 float32, 385 ... 416
// one-byte elements) keeps its whole lines in the main table (stride 384) and its last one or two chunks in a dense side
// table -- as long as that table stays small enough to live in L2 / Infinity Cache (FLATNAV_SPLIT_TAIL_MAX_MB, default 64 MB:
// 4 M rows of 16 bytes), where the fourth request of a gather no longer costs an HBM line that is 7/8 padding.
// FLATNAV_SPLIT_ROWS=0 turns it off (rows are then padded to four lines, as in rounds 2-5).  Every handle on the same
// buffers (views, fnv_index_adopt, replicas, the ranks of a broadcast) derives the same layout from (dim, type, capacity).
struct RowLayout {
  uint32_t row_bytes, tail_bytes;
};
inline RowLayout row_layout(uint32_t dim, int data_type, uint64_t capacity) {
  const uint64_t rb16 = ((uint64_t)dim * dtype_size(data_type) + 15) / 16 * 16;
  const uint64_t rem = rb16 % 128;
  long on = 1, max_mb = 64;
  if (const char* env = getenv("FLATNAV_SPLIT_ROWS")) on = strtol(env, nullptr, 10);
  if (const char* env = getenv("FLATNAV_SPLIT_TAIL_MAX_MB")) max_mb = strtol(env, nullptr, 10);
  if (on && rb16 - rem == 384 && rem > 0 && rem <= 32 && capacity * rem <= ((uint64_t)max_mb << 20))
    return RowLayout{384u, (uint32_t)rem};
  return RowLayout{row_stride_bytes(dim, data_type), 0u};
}

inline uint32_t pow2_ceil(uint64_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}
inline uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

// ---- launch configuration ---------------------------------------------------------------------------------
// How a query slot's LDS is laid out depends on the kernel: the two-heap kernel keeps {query, neighbours heap,
// candidates heap, visited table, staging}; the merged-beam kernel keeps {query, [beam array], visited table, staging}.
enum { MODE_HEAPS = 0, MODE_MERGED_REGS = 1, MODE_MERGED_LDS = 2 };

// Visited-table geometry for a table of `slots` (2^j or 3*2^j) and the LDS layout that follows from it; returns the
// bytes of LDS one query slot needs.  16-bit tags whenever the per-bucket id range fits 14 bits: buckets =
// mult*2^k, t = nbits - k, need t <= 14 (mult 1) or t <= 15 (mult 3).
inline uint32_t lay_out(const PlanInputs* ix, SearchParams& p, uint32_t slots, int mode) {
  uint32_t nbits = 1;
  while (nbits < 32 && (1ull << nbits) < ix->capacity) nbits++;
  const uint32_t mult = (slots % 3 == 0) ? 3u : 1u;
  uint32_t k = 0;
  for (uint32_t b = slots / 4 / mult; b > 1; b >>= 1) k++;
  const bool can16 = !ix->visited_wide && ix->visited_tag_bits <= 16 && nbits <= 30 && k <= nbits && (nbits - k) <= (mult == 3 ? 15u : 14u);
  // otherwise 64-bit buckets: three 21-bit tags (slots = 3 * 2^j) or two 32-bit tags (slots = 2^j)
  const uint32_t w = can16 ? 16u : (slots % 3 == 0 ? 21u : 32u);
  const uint32_t wbuckets = w == 21 ? slots / 3 : slots / 2;
  uint32_t wk = 0;
  for (uint32_t b = wbuckets; b > 1; b >>= 1) wk++;
  const bool canw = !can16 && !ix->visited_wide && wk <= nbits && (nbits - wk) <= w - 2;
  if (!can16 && !canw && mult == 3) slots = pow2_ceil(slots);  // the open-addressing table needs a power of two
  p.vis_slots = slots;
  p.vis_tag16 = (can16 || canw) ? 1u : 0u;
  p.vis_w = w;
  p.vis_mult = can16 ? mult : 1u;
  p.vis_nmask = (uint32_t)((1ull << nbits) - 1ull);
  p.vis_rshift = can16 ? nbits - k : (canw ? nbits - wk : 0);
  p.vis_rmask = p.vis_tag16 ? (uint32_t)((1ull << p.vis_rshift) - 1ull) : 0;
  p.vis_bytes = can16 ? slots * 2 : (canw ? wbuckets * 8 : slots * 4);
  p.vis_shift = 32;
  for (uint32_t sft = p.vis_slots; sft > 1; sft >>= 1) p.vis_shift--;
  p.vis_limit = p.vis_slots / 4 * 3;

  uint32_t off = 0;
  p.off_q = off;
  off = align16(off + p.q_lds_bytes);
  // neighbours heap (exact search) / sorted beam: arrays start at 16n + 8 so that child pairs are 16-byte aligned
  p.off_nbr = off + 8;
  // (merged-beam kernel: the same bytes stage a link row's distances, [WAVE + 1] floats, between two merges)
  off = align16(off + 8 + std::max<uint32_t>(((uint32_t)p.B + 2) * 8, mode == MODE_MERGED_REGS ? (WAVE + 1) * 4 : 0));
  p.off_stage_d = p.off_nbr;
  if (mode == MODE_MERGED_LDS) {  // LDS form: the array is the beam itself, the staging area its own
    p.off_stage_d = off;
    off = align16(off + (WAVE + 1) * 4);
  }
  p.off_cand = off + 8;  // candidates heap of the exact search: cand_slots entries in LDS (0: all of it in HBM)
  if (p.cand_slots) off = align16(off + 8 + (p.cand_slots + 1) * 8);
  p.off_vis = off;
  off = align16(off + p.vis_bytes);
  p.off_stage_ids = off;
  off = align16(off + (WAVE + 1) * 4);  // + one write-only slot for lanes with nothing to stage
  p.off_ovf = off;
  off = align16(off + (OVF_LIST + 2 + STASH) * 4);
  return off;
}

// Chooses the visited-table size for `kern` in `mode`, fills p's geometry/layout fields; outputs the LDS bytes per
// slot and the slots one CU keeps resident.
// Table sizes, ascending: 256, 384, 512, 768, ...  The roomy size (visited_factor * B + 600, <= 60 % load on the
// reference workloads) keeps every id in LDS; but LDS is also what limits how many queries a CU keeps in flight, and
// a lone wave issues slowly -- below ~13 resident queries per CU the loss of latency hiding costs more than sending
// part of the ids to the HBM bitmap (measured: profiles/r1_visited_sizing.md).  So: the largest size <= roomy that
// still leaves `occupancy_target` queries per CU, but never below visited_floor slots.
// gfx950 hands LDS out in 1280-byte granules (160 KiB = 128 of them): a workgroup that asks for 7712 bytes holds seven, and
// a CU keeps 18 such workgroups, not the floor(163840 / 7712) = 21 that hipOccupancyMaxActiveBlocksPerMultiprocessor reports.
// Measured in round 4 (tools/dev/probes/lds_granule.cpp: resident single-wave workgroups per CU against the dynamic LDS size
// -- 7680 bytes: 21, 7681: 18; 8960: 18, 8961: 16; 10240: 16, 10241: 14; 32768: 4) after the launch timeline of the uint8 index
// showed 18 busy slots per CU under a grid of 21 (profiles/r4_launch_timeline.md).
constexpr uint32_t kLdsGranule = 1280, kLdsPerCu = 160u * 1024u;  // (160 KiB = 163840 bytes)
inline uint32_t lds_allocated(uint32_t lds) { return (lds + kLdsGranule - 1) / kLdsGranule * kLdsGranule; }

template <class Runtime>
inline int configure_launch(const PlanInputs* ix, SearchParams& p, Runtime& rt, std::string& err, int mode, uint32_t* lds_out,
                            int* bpc_out, bool grow_free = true, uint32_t forced_slots = 0) {
  // query slots one CU holds with this much LDS each, as the occupancy API counts them.  The table-size rules below were
  // calibrated against THIS number in rounds 1-3 and keep using it (same layouts as measured); what a CU really keeps
  // resident -- `really_resident` -- decides the granule trim at the end.
  auto resident = [&](uint32_t lds) -> int {
    if (lds > kLdsPerCu) return 0;
    return rt.occupancy(mode, lds);
  };
  auto really_resident = [&](uint32_t lds) -> int {  // registers and wave slots: the API; LDS: whole granules
    return std::min<int>(resident(lds), (int)(kLdsPerCu / lds_allocated(std::max<uint32_t>(lds, 1u))));
  };
  uint32_t lds_bytes;
  if (forced_slots == 0) forced_slots = (uint32_t)ix->visited_slots;
  if (forced_slots) {
    lds_bytes = lay_out(ix, p, forced_slots, mode);
  } else {
    const uint64_t want = std::max<uint64_t>((uint64_t)ix->visited_factor * (uint64_t)p.B + 600, 256);
    std::vector<uint32_t> sizes;
    for (uint32_t base = 256; base <= (1u << 15); base <<= 1) {
      sizes.push_back(base);
      if (base >= want) break;
      if (base < (1u << 15)) {
        sizes.push_back(base / 2 * 3);
        if ((uint64_t)base / 2 * 3 >= want) break;
      }
    }
    size_t pick = sizes.size() - 1;  // roomy
    lds_bytes = lay_out(ix, p, sizes[pick], mode);
    (void)rt.raise_lds_limit(mode, std::min<uint32_t>(lds_bytes, kLdsPerCu));  // (a failure here is ignored, and leaves no message)
    // (a table that holds every id is worth more than the last resident queries: it is kept down to
    // `occupancy_roomy` (9) of them -- measured with the merged-beam kernel at ef 160-200: -4...-18 % time at 9-11 resident
    // queries against a smaller table that overflows at 15; below that the smaller table wins again)
    const int target = (mode != MODE_HEAPS && resident(lds_bytes) >= (int)ix->occupancy_roomy) ? 0 : (int)ix->occupancy_target;
    const uint32_t roomy_tag16 = p.vis_tag16;
    for (size_t cand = pick; cand-- > 0 && sizes[cand] >= (uint32_t)ix->visited_floor && resident(lds_bytes) < target;) {
      const uint32_t smaller = lay_out(ix, p, sizes[cand], mode);
      // not a step down: the tag format lost (too few buckets for this id width), or -- wider tags per slot -- no
      // fewer bytes than the table already chosen
      if (p.vis_tag16 != roomy_tag16 || smaller >= lds_bytes) continue;
      pick = cand;
      lds_bytes = smaller;
    }
    lds_bytes = lay_out(ix, p, sizes[pick], mode);
    // A bigger table that costs no resident query is free: at ef=52 the 2048-slot table (60 % full at the end of a
    // query) already sends ids to the HBM bitmap; 3072 slots fit the same 16 queries per CU (-7 % kernel time).
    if (grow_free && pick + 1 == sizes.size()) {
      for (int step = 0; step < 2; step++) {
        const uint32_t have = p.vis_slots;
        const uint32_t next = (have & (have - 1)) == 0 ? have / 2 * 3 : have / 3 * 4;
        if (next > (1u << 15)) break;
        SearchParams q = p;
        const uint32_t bytes = lay_out(ix, q, next, mode);
        if (q.vis_tag16 != p.vis_tag16 || q.vis_slots != next || bytes > kLdsPerCu || resident(bytes) < resident(lds_bytes)) break;
        p = q;
        lds_bytes = bytes;
      }
    }
  }
  if (lds_bytes > kLdsPerCu)
    return err = "ef_search too large for the on-chip beam state (needs " + std::to_string(lds_bytes) +
                 " bytes of LDS, 163840 available); lower ef_search or the *_slots options", FNV_ERR_INVALID;
  if (const char* e = rt.raise_lds_limit(mode, lds_bytes)) {
    err = std::string("raise_lds_limit((const void*)kern, ix->device, lds_bytes) failed: ") + e;
    return FNV_ERR_NO_DEVICE;
  }
  // A layout that ends a few bytes into a granule pays a whole granule per slot for them.  If dropping at most an eighth of
  // the exact search's LDS heap entries (its overflow continues in the slot's HBM spill area; the heap is sized by rule of
  // thumb: cand_factor * B + 192) brings the slot one granule down AND that keeps one more query resident, do so
  // (the uint8 index at ef=52: 7712 -> 7680 bytes, 18 -> 21 slots per CU, +3 % queries/s, profiles/r4_launch_timeline.md).
  if (ix->cand_slots == 0 && p.cand_slots > (uint32_t)p.B + 1) {
    const uint32_t lower = lds_allocated(lds_bytes) - kLdsGranule;
    const uint32_t over = lds_bytes - lower, entries = (over + 7) / 8;
    if (lower > 0 && entries <= p.cand_slots / 8 && p.cand_slots - entries >= (uint32_t)p.B + 1 && really_resident(lower) > really_resident(lds_bytes)) {
      SearchParams q = p;
      q.cand_slots = p.cand_slots - entries;
      uint32_t bytes = lay_out(ix, q, p.vis_slots, mode);
      for (int i = 0; i < 2 && bytes > lower && q.cand_slots > (uint32_t)p.B + 2; i++) {  // (16-byte alignment of what follows the heap)
        q.cand_slots--;
        bytes = lay_out(ix, q, p.vis_slots, mode);
      }
      if (bytes <= lower && q.vis_slots == p.vis_slots && q.vis_tag16 == p.vis_tag16) {
        p = q;
        lds_bytes = bytes;
      }
    }
  }
  // The GRID is the slots a CU really keeps resident (round 5).  Rounds 1-4 launched the occupancy API's count, also where
  // that is one more than the LDS granules allow (the surplus workgroup starts when the first slot exits, finds the dispenser
  // empty and leaves): sizing the grid by `really_resident` lost 0.7-2.9 % then, because the exact tail is a percentage of the
  // grid and 75 % of the API's count sat nearer the best tail length.  With the hand-over the configurations where the two
  // counts differ run without a tail, and the two grids measure the same (c4 ef=110: 2.0857 vs 2.0837 ms, 10M x 768 ef=670:
  // 102.37 vs 102.40 ms; gpurun r5 run 24) -- so `blocks_per_cu` now says what it means.  The table-size rules above keep
  // comparing the API's counts (the layouts they choose are the measured ones).
  int bpc = really_resident(lds_bytes);
  if (bpc < 1) bpc = 1;
  if (ix->blocks_per_cu > 0) bpc = std::min<int>(bpc, (int)ix->blocks_per_cu);
  *lds_out = lds_bytes;
  *bpc_out = bpc;
  return FNV_OK;
}

// Records of the hand-over log per query slot (kernels.hpp): a query logs ~6 records per beam entry on the reference workloads
// (1M x 128 at ef=52: ~310; a hop is a header + the row's admissible neighbours); 24 per entry + 512, in [1024, 16384] records
// of 8 bytes per slot = 8-128 KB, or what "tie_log_entries" says (in [WAVE + 2, 2^20]).  A log that overflows ends (the query
// is searched again from scratch if equal keys meet).
inline uint32_t log_entries_for(const PlanInputs* ix, int B) {
  if (!ix->tie_replay) return 0u;
  if (ix->tie_log_entries) return (uint32_t)std::min<int64_t>(1 << 20, std::max<int64_t>(WAVE + 2, ix->tie_log_entries));
  return std::min<uint32_t>(16384u, std::max<uint32_t>(1024u, pow2_ceil(24ull * (uint64_t)B + 512)));
}

// Per query slot of a launch on this index: words of the visited set's HBM bitmap (whole 16-byte groups: wide clears) and
// entries of the list of ids whose bitmap words need clearing.
inline uint32_t bitmap_words_of(const PlanInputs* ix) { return (uint32_t)(((ix->capacity + 31) / 32 + 3) / 4 * 4); }
inline uint32_t ovf_cap_of(const PlanInputs* ix) {
  return ix->overflow_list >= 0 ? (uint32_t)ix->overflow_list : ((uint64_t)bitmap_words_of(ix) * 4 > (512u << 10) ? 16384u : 0u);
}

// How the kernels walk a row of this index: the row configuration, the chunks of a staged query, whether rows are whole spans.
struct RowGeometry {
  int cfg;
  uint32_t nchunks, tail_chunks, q_chunks;
  bool full;
};
inline RowGeometry row_geometry(const PlanInputs* ix) {
  RowGeometry g;
  g.nchunks = ix->row_bytes / 16;
  g.tail_chunks = ix->tail_bytes / 16;
  g.cfg = pick_row_cfg(g.nchunks, g.tail_chunks);
  const uint32_t per_iter = (uint32_t)(kCfgs[g.cfg].G * kCfgs[g.cfg].CU);
  g.q_chunks = (g.nchunks + per_iter - 1) / per_iter * per_iter;
  if (g.tail_chunks) g.q_chunks = g.nchunks + (uint32_t)kCfgs[g.cfg].G;  // split rows: lane g also reads query chunk 24 + g (zero past the row)
  g.full = g.tail_chunks == 0 && (g.nchunks % per_iter) == 0;  // rows are whole spans: the lean FULL kernels apply
                                                                // (the three-line configuration's non-FULL form IS the split-row kernel)
  return g;
}

// What a search launch looks like for one (beam width, K) on one index: cached (launch.hip, which adds the kernels),
// because working it out costs several occupancy queries and a single-query search should not pay for them every time.
struct LaunchPlan {
  bool valid = false;
  int B = 0, K = 0, cfg = 0, mode = 0;
  bool full = false;
  uint64_t capacity = 0, options_version = 0, layouts_version = 0;  // (made under these: launch.hip, ensure_plan)
  SearchParams heaps, sorted;                 // geometry + LDS layout for each (pointers and per-call fields unset)
  uint32_t lds = 0, slds = 0;
  int bpc = 0, sbpc = 0;
};

// The launch plan for (beam width, K): depends on the live geometry, the options and `lc`, the layout fnv_tune measured for
// this beam width (default: none), only.  The caller marks it valid and adds what the planner does not know: the table
// pointers of both parameter blocks, the kernels, the options' version.
template <class Runtime>
inline int plan_launch(const PlanInputs* ix, int B, int K, const LayoutChoice& lc, Runtime& rt, std::string& err, LaunchPlan& plan) {
  plan = LaunchPlan();
  const RowGeometry g = row_geometry(ix);
  SearchParams p;
  memset(&p, 0, sizeof(p));
  p.tail_chunks = g.tail_chunks;
  p.M = ix->M;
  p.dim = ix->dim;
  p.row_bytes = ix->row_bytes;
  p.nchunks = g.nchunks;
  p.K = K;
  p.B = B;
  p.q_chunks = g.q_chunks;
  p.q_lds_bytes = cfg_query_in_regs(g.cfg) ? 0u : p.q_chunks * 16u;
  p.cand_slots = ix->cand_slots ? (uint32_t)ix->cand_slots : (uint32_t)(ix->cand_factor * p.B + 192);
  p.cand_slots = std::max<uint32_t>(p.cand_slots, (uint32_t)p.B + 1);  // also hosts the final result list
  p.spill_entries = (uint32_t)ix->spill_entries;
  p.bitmap_words = bitmap_words_of(ix);
  p.ovf_cap = ovf_cap_of(ix);
  p.log_entries = log_entries_for(ix, p.B);
  plan.cfg = g.cfg;
  plan.full = g.full;

  // the exact two-heap kernel: always configured (it also replays what a merged-beam kernel hands over)
  plan.heaps = p;
  int rc = configure_launch(ix, plan.heaps, rt, err, MODE_HEAPS, &plan.lds, &plan.bpc);
  if (rc) return rc;

  // Merged-beam kernel (merged_beam.hpp): the beam as one sorted array, one merge per link row -- in registers for
  // beams of at most 256 entries ("beam_registers" = 0: never), else in LDS; queries in which equal keys meet at a
  // decision are searched again by the same wave with the exact two-heap code.  Same results.  "sorted_beam":
  // 0 = never, 1 = always, 2 (default) = adaptive: measured against the two-heap kernel per beam width (below).
  const bool tagged = plan.heaps.vis_tag16 != 0;
  const bool want = ix->sorted_beam != 0 && B >= ix->sorted_beam_min && ix->capacity < (1ull << 31);
  plan.mode = (!tagged || !want) ? MODE_HEAPS : (B <= MB_MAX_BEAM && ix->beam_registers != 0) ? MODE_MERGED_REGS : MODE_MERGED_LDS;
  if (plan.mode != MODE_HEAPS) {
    // a layout that fnv_tune measured for this beam width overrides the rules below (heap home, table size)
    const int64_t cand_lds_mode = lc.cand_lds >= 0 ? lc.cand_lds : ix->sorted_cand_lds;
    const uint32_t forced = lc.vis_slots;
    // the exact re-run's candidates heap: in LDS if that costs neither resident queries nor visited-table
    // slots, else entirely in the slot's HBM spill area (slower for the few queries that need it)
    SearchParams with = p, without = p;
    without.cand_slots = 0;
    uint32_t lds_w = 0, lds_wo = 0;
    int bpc_w = 0, bpc_wo = 0;
    rc = configure_launch(ix, without, rt, err, plan.mode, &lds_wo, &bpc_wo, false, forced);
    if (rc) return rc;
    const int rc_w = configure_launch(ix, with, rt, err, plan.mode, &lds_w, &bpc_w, false, forced);
    // (an exact re-run whose candidates heap lives in HBM pays a global round trip per heap operation: a handful of
    // such queries per launch are stragglers that cost 10 % of it -- measured at ef=100 on float data with 5 re-runs
    // in 10 000 queries -- so up to beams of 128 the LDS home is worth going down to 9 resident queries; wider beams'
    // heaps cost more LDS than the stragglers cost time)
    bool keep_lds = rc_w == FNV_OK && (cand_lds_mode == 1 ||
                                       (cand_lds_mode == 2 && ((bpc_w >= bpc_wo && with.vis_slots >= without.vis_slots) ||
                                                               (B <= 2 * WAVE && bpc_w >= (int)ix->occupancy_roomy))));
    // both candidates once more with the free table growth; an LDS home that costs residency AND table slots is not taken
    SearchParams fin_w = p, fin_wo = p;
    // (p's own heap size, not `with`'s: configure_launch may already have trimmed that one by up to an eighth to fit an LDS
    //  granule, and the trim must be applied once, to the final layout)
    fin_w.cand_slots = p.cand_slots;
    fin_wo.cand_slots = 0u;
    uint32_t flds_w = 0, flds_wo = 0;
    int fbpc_w = 0, fbpc_wo = 0;
    rc = configure_launch(ix, fin_wo, rt, err, plan.mode, &flds_wo, &fbpc_wo, true, forced);
    if (rc) return rc;
    if (keep_lds) {
      rc = configure_launch(ix, fin_w, rt, err, plan.mode, &flds_w, &fbpc_w, true, forced);
      if (rc) return rc;
      if (cand_lds_mode == 2 && fin_w.vis_slots < fin_wo.vis_slots && fbpc_w < fbpc_wo) keep_lds = false;
    }
    plan.sorted = keep_lds ? fin_w : fin_wo;
    plan.slds = keep_lds ? flds_w : flds_wo;
    plan.sbpc = keep_lds ? fbpc_w : fbpc_wo;
    if (!plan.sorted.vis_tag16) plan.mode = MODE_HEAPS;
    if ((uint64_t)plan.sorted.cand_slots + plan.sorted.spill_entries < 3ull * (uint64_t)B + 256) plan.mode = MODE_HEAPS;
  }
  plan.B = B;
  plan.K = K;
  plan.capacity = ix->capacity;
  return FNV_OK;
}

// Which kernel variant the launch runs, and whether it is a sample for the adaptive choice.
struct KernelChoice {
  bool sorted;  // the merged-beam kernel (else the two-heap kernel, or its filtered form)
  int variant;
  bool multi_round, sample = false, exploratory = false;
  bool adaptive = false;  // nothing is pinned and "sorted_beam" = 2: the variant is for the measurements to decide (choose_kernel)
  int64_t tail_pct;
};
// A launch of more than one round of the merged-beam kernel's resident slots (an exact tail needs a second round).
inline bool multi_round_launch(const PlanInputs* ix, const LaunchPlan& plan, uint64_t nq) {
  return nq > (uint64_t)plan.sbpc * (uint64_t)ix->num_cus;
}
// Once the variant is known: what follows from it (variant 0 is the two-heap kernel; 2-5 carry their own tail).
inline void set_variant(KernelChoice& c, int variant) {
  c.variant = variant;
  c.sorted = variant != 0;
  if (variant >= 2) c.tail_pct = kTailPct[variant];
}
// A pinned variant (fnv_tune's launches / "sorted_variant"): as asked when this launch can run it, else the merged-beam kernel.
inline int pinned_variant(int pinned, bool multi_round, bool shadows_on) {
  return variant_allowed(pinned, multi_round, true, shadows_on, true) ? pinned : 1;
}
// Before any measurement: the kernel the plan prefers, whether the launch is longer than one round, the tail the option asks
// for -- or the variant that is pinned (`force_variant` >= 0: fnv_tune's launches; else "sorted_variant").
inline KernelChoice default_choice(const PlanInputs* ix, const LaunchPlan& plan, uint64_t nq, bool filtered, int force_variant = -1) {
  // Adaptive choice ("sorted_beam" = 2): both kernels give the same answers; which one is faster depends on how often
  // equal keys force the merged-beam kernel to search a query twice (rarely on float data, often on integer-valued
  // data with wide beams) -- so it is measured: launches of at least 2048 queries are timed by the events that bracket
  // them anyway, harvested when a later call finds them complete, first one kernel, then the other, then the faster.
  // A filtered launch always runs the two-heap kernel's filtered form: no merged beam, no samples for the adaptive choice
  // (the tuner's measurements are left alone), no hand-over, tie log or shadows.
  KernelChoice c;
  c.sorted = plan.mode != MODE_HEAPS && !filtered;
  c.variant = c.sorted ? 1 : 0;
  // The merged-beam kernel's stragglers: a query that is searched twice finishes a whole exact-search latency late, and
  // in the last round of a launch that lengthens the launch itself (one such query costs as much as hundreds).  With
  // "sorted_tail_exact_pct" = p the last p % of one round of queries skip the sorted pass (the exact search is slower but
  // never needs a second one): -15 % on the integer-valued SIFT stand-in at ef=52, +0-4 % on float data without ties --
  // so by default (-1) it is one more variant that the adaptive choice measures.
  c.multi_round = c.sorted && multi_round_launch(ix, plan, nq);
  c.tail_pct = ix->sorted_tail_exact_pct < 0 ? 0 : ix->sorted_tail_exact_pct;
  const int pinned = force_variant >= 0 ? force_variant : (int)ix->sorted_variant;
  c.adaptive = c.sorted && pinned < 0 && ix->sorted_beam == 2;
  if (c.sorted && pinned >= 0) set_variant(c, pinned_variant(pinned, c.multi_round, ix->shadow_exact != 0));
  return c;
}
// The adaptive choice ("sorted_beam" = 2) keeps, per tuner_key, the best time of each variant (Tuner, in the handle's
// Measurements: measurements.hpp); choose_kernel (launch.hip) hands the timing of an `adaptive` choice's last sample to
// Measurements::harvest, asks the three rules below and hands the answer to set_variant.
// A hidden lane runs the fastest variant its owner has measured (-1: none measured); the lowest ordinal wins a tie.
inline int lane_variant(const Tuner& t, bool multi_round, bool try_tail, bool shadows_on) {
  int best = -1;
  for (int v = 0; v < kNumVariants; v++)
    if (variant_allowed(v, multi_round, try_tail, shadows_on) && t.samples[v] > 0 && (best < 0 || t.best[v] < t.best[best])) best = v;
  return best;
}
// The owner: the next variant to sample (-1: every allowed one has its three samples) ...
inline int owner_next_sample(const Tuner& t, bool multi_round, bool try_tail, bool shadows_on) {
  int pick = -1;
  for (int v : {1, 0, 6, 4, 3, 2, 5})
    if (variant_allowed(v, multi_round, try_tail, shadows_on) && pick < 0 && t.samples[v] < 3) pick = v;
  return pick;
}
// ... and its final pick: the fastest, the merged-beam kernel (1) winning a tie against the two-heap kernel (0).
inline int owner_final_variant(const Tuner& t, bool multi_round, bool try_tail, bool shadows_on) {
  int pick = 0;
  for (int v = 1; v < kNumVariants; v++)
    if (variant_allowed(v, multi_round, try_tail, shadows_on) && t.samples[v] > 0 &&
        (t.best[v] < t.best[pick] || (v == 1 && t.best[1] <= t.best[0])))
      pick = v;
  return pick;
}

// Small launches on small indexes (round 5): when a bitmap of ALL node ids fits the LDS of the slots the launch needs, the
// visited set is that bitmap (csrc/visited.hpp visited_insert_direct: one LDS round trip per link row, nothing overflows)
// instead of the tag table, and the launch runs the kernel's DIRECT instantiation -- a launch that leaves the GPU mostly idle
// is a chain of dependent latencies, and the tag table is 1.8 k of a lone hop's 7.9 k cycles.  The table is the last but
// two of the slot's LDS areas: only what follows it moves.
// Only in launches that fill at most a quarter of the slots, and not when the caller has pinned the table's shape
// ("visited_slots", "visited_tag_bits", "visited_wide"); "visited_direct" = 0 turns it off.
inline bool lay_out_direct(const PlanInputs* ix, SearchParams& p, uint32_t* lds_bytes, int bpc, uint32_t nslots) {
  if (ix->visited_direct == 0 || ix->visited_slots != 0 || ix->visited_tag_bits != 0 || ix->visited_wide != 0 || !p.vis_tag16) return false;
  const uint64_t ids = std::max<uint64_t>(ix->capacity, ix->parent_capacity);
  const uint64_t bytes = ((ids + 7) / 8 + 15) / 16 * 16;
  if (bytes + p.off_vis + 1024 <= kLdsPerCu) {
    SearchParams d = p;
    d.vis_w = 1;
    d.vis_bytes = (uint32_t)bytes;
    d.vis_slots = (uint32_t)(bytes * 8);  // (what fnv_last_launch_geometry reports: one slot per node id)
    uint32_t off = align16(d.off_vis + d.vis_bytes);
    d.off_stage_ids = off;
    off = align16(off + (WAVE + 1) * 4);
    d.off_ovf = off;
    off = align16(off + (OVF_LIST + 2 + STASH) * 4);
    const uint64_t per_cu = std::min<uint64_t>((uint64_t)bpc, kLdsPerCu / lds_allocated(off));
    if (off <= kLdsPerCu && (uint64_t)nslots <= per_cu * (uint64_t)ix->num_cus) {
      p = d;
      *lds_bytes = off;
      return true;
    }
  }
  return false;
}

// The shape of one launch of `nq` queries over `live` nodes with the kernel `c` chose, `bpc` slots per CU resident.
struct LaunchShape {
  bool small_launch, shadow;
  uint32_t nslots, tail_shadows, max_slots;  // the grid; exact shadows of the last queries; the slots the workspace is sized for
  uint32_t tail_exact;                       // (before shadows, which switch it off)
  uint32_t scan_step, n_scan;                // the entry scan
};
inline LaunchShape launch_shape(const PlanInputs* ix, const LaunchPlan& plan, const KernelChoice& c, int bpc, uint64_t nq,
                                int num_initializations, uint64_t live) {
  LaunchShape s;
  const bool sorted = c.sorted;
  // Shadow mode (search_types.h): a launch that fills at most a quarter of the resident slots starts, next to the
  // merged-beam search of every query, an exact search of the same query on another slot.  A query in which equal keys
  // meet at a decision is then answered after ONE exact-search latency from the start of the launch instead of a
  // merged-beam pass plus a re-run (batch of 64 at ef=100 on the integer-valued data: p50 0.80 -> 0.47 ms); the shadow of
  // a query that needs none stops at its next hop.  Same bytes either way.
  s.small_launch = 4 * nq <= (uint64_t)bpc * (uint64_t)ix->num_cus;
  s.shadow = sorted && ix->shadow_exact != 0 && s.small_launch;
  s.nslots = s.shadow ? (uint32_t)(2 * nq) : (uint32_t)std::min<uint64_t>(nq, (uint64_t)bpc * (uint64_t)ix->num_cus);
  // Tail shadows (variant 6, search_types.h): one exact shadow per slot at most -- of the queries dispensed last
  s.tail_shadows = (sorted && !s.shadow && c.variant == kVariantTailShadows) ? (uint32_t)std::min<uint64_t>(nq, s.nslots) : 0u;
  s.max_slots = std::max<uint32_t>(s.nslots, (uint32_t)std::min<uint64_t>(nq, (uint64_t)std::max(plan.bpc, plan.sbpc) * (uint64_t)ix->num_cus));
  // Index.h:851-861: step = max(1, N / n_init); nodes 0, step, 2*step, ... < N
  uint64_t step = live / (uint64_t)num_initializations;
  if (step == 0) step = 1;
  s.scan_step = (uint32_t)step;
  s.n_scan = (uint32_t)((live + step - 1) / step);
  s.tail_exact = c.multi_round && sorted ? (uint32_t)std::min<uint64_t>((uint64_t)c.tail_pct * s.nslots / 100, nq) : 0u;
  return s;
}

// One graph-search launch, whole: its shape, the slots per CU and LDS bytes of the kernel `c` chose, whether it runs the DIRECT
// form, the mode it reports -- and `p`, filled in place with that kernel's parameter block of the plan (the DIRECT layout
// applied).  `filtered_bpc`: a filtered launch's resident slots per CU with the filtered kernel (0: the launch is not filtered).
// The one function search_device_impl (launch.hip) and the CPU test's harness both shape a launch with.
struct SearchLaunch : LaunchShape {
  int bpc, mode;
  uint32_t lds;
  bool direct;
};
inline SearchLaunch shape_search(const PlanInputs* ix, const LaunchPlan& plan, const KernelChoice& c, int filtered_bpc, uint64_t nq,
                                 int num_initializations, uint64_t live, SearchParams& p) {
  SearchLaunch s;
  s.bpc = c.sorted ? plan.sbpc : filtered_bpc ? filtered_bpc : plan.bpc;
  s.lds = c.sorted ? plan.slds : plan.lds;
  s.mode = c.sorted ? plan.mode : MODE_HEAPS;
  static_cast<LaunchShape&>(s) = launch_shape(ix, plan, c, s.bpc, nq, num_initializations, live);
  p = c.sorted ? plan.sorted : plan.heaps;
  s.direct = c.sorted && s.small_launch && lay_out_direct(ix, p, &s.lds, s.bpc, s.nslots);
  return s;
}

// K0 (entry_scan_kernel, kernels.hpp): the batch's shared entry-scan rows staged in LDS tiles of whole rows, the row stride
// padded by 16 bytes against bank conflicts -- as many rows as 64 KB hold (at least one), behind the workgroup's staged
// queries (SCAN_WAVES of them at a time) and its SCAN_QPB results; one workgroup per SCAN_QPB queries.
struct EntryScanTile {
  uint32_t stride, rows, lds, grid;
};
inline EntryScanTile entry_scan_tile(uint32_t row_bytes, uint32_t q_chunks, uint32_t n_scan, uint64_t nq) {
  EntryScanTile t;
  t.stride = row_bytes + 16;
  t.rows = std::max<uint32_t>(1, std::min<uint32_t>(n_scan, (64u * 1024u) / t.stride));
  t.lds = SCAN_WAVES * q_chunks * 16 + SCAN_QPB * 8 + t.rows * t.stride;
  t.grid = (uint32_t)((nq + SCAN_QPB - 1) / SCAN_QPB);
  return t;
}

// HBM per query slot of a launch on this index, in bytes: the visited set's bitmap, the list of ids whose bitmap words need
// clearing, the candidates heap's spill area, the hand-over log of `log_entries` records (a plan's: log_entries_for its beam).
struct SlotWorkspace {
  uint64_t bitmap, ovf, spill, tielog;
  uint64_t bytes() const { return bitmap + ovf + spill + tielog; }
};
inline SlotWorkspace slot_workspace(const PlanInputs* ix, uint64_t log_entries) {
  return SlotWorkspace{(uint64_t)bitmap_words_of(ix) * 4, (uint64_t)ovf_cap_of(ix) * 4, (uint64_t)ix->spill_entries * 8, log_entries * 8};
}

// ---- exhaustive search (scan.hpp) and the scan stage of a routed filtered graph search ----------------------------
// 32-bit words of a bitmap with one bit per node id, and the `rows` node bitmaps of a grouped launch (n_filters + 2 of them).
inline uint64_t node_words(const PlanInputs* ix) { return (ix->capacity + 31) / 32; }
inline size_t filter_rows_bytes(const PlanInputs* ix, uint64_t rows) { return (size_t)rows * (size_t)node_words(ix) * 4; }

// How a launch of `nq` queries for K results is cut up: queries per tile (as many as a block's LDS budget holds next to their
// result lists, at most 32), row segments (enough blocks to fill the device, at most 64 and at most what keeps the partial
// lists within 256 MB; or what "scan_segment_rows" asks for).
constexpr uint32_t kScanLdsBudget = 20u << 10;  // per block: eight blocks per CU = two wavefronts per SIMD
constexpr uint32_t kScanMaxTile = 32, kScanMaxSegments = 64, kScanForcedSegments = 1024;
constexpr uint64_t kScanPartialBudget = 256ull << 20;
constexpr uint32_t kScanMaxLds = 160u << 10;  // one query and its list must fit a block's LDS
struct ScanShape {
  uint32_t tile, tiles, segments, lds;
};
// `filter_rows` != 0: a grouped launch over that many filter rows -- the id queue comes out of the block's LDS budget, and
// `tiles` is the bound on the data-dependent tile count that the launch covers (scan_select.hpp, group_tile_bound).
inline ScanShape scan_shape(const PlanInputs* ix, const RowGeometry& g, uint64_t nq, int K, uint64_t live, uint64_t filter_rows = 0) {
  ScanShape s;
  const uint32_t per_query = g.q_chunks * 16u + (uint32_t)K * 8u;
  const uint32_t queue = filter_rows ? SCAN_QUEUE_IDS * 4u : 0u;
  s.tile = std::max(1u, std::min(kScanMaxTile, (kScanLdsBudget - queue) / per_query));
  s.tile = (uint32_t)std::min<uint64_t>(s.tile, nq);
  s.lds = s.tile * per_query + queue;
  s.tiles = (uint32_t)(filter_rows ? group_tile_bound(nq, filter_rows, s.tile) : (nq + s.tile - 1) / s.tile);
  uint64_t seg;
  if (ix->scan_segment_rows > 0) {
    seg = std::min<uint64_t>((live + (uint64_t)ix->scan_segment_rows - 1) / (uint64_t)ix->scan_segment_rows, kScanForcedSegments);
  } else {
    const uint64_t want_blocks = (uint64_t)std::max(1, ix->num_cus) * 8u;
    seg = std::min<uint64_t>((want_blocks + s.tiles - 1) / s.tiles, std::max<uint64_t>(1, live / 1024));
    seg = std::min<uint64_t>(seg, kScanMaxSegments);
    seg = std::min<uint64_t>(seg, std::max<uint64_t>(1, kScanPartialBudget / (nq * (uint64_t)K * 8u)));
  }
  seg = std::min<uint64_t>(seg, 0x7FFFFFFFull / s.tiles);
  s.segments = (uint32_t)std::max<uint64_t>(1, seg);
  return s;
}
// The partial lists of a launch: one sorted list of K keys per (query, segment); the merge's LDS: three such lists.
inline size_t scan_partial_bytes(uint64_t nq, const ScanShape& s, int K) { return (size_t)nq * s.segments * (size_t)K * 8; }
inline uint32_t scan_merge_lds(uint32_t K) { return 3u * K * 8u; }

// The grouping arrays of a grouped scan (scan.hpp's group_* kernels), as uint32 offsets into one buffer.
// `routed` (the scan stage of a routed filtered graph search): nq route words and the overflow flag behind them as well.
struct GroupArrays {
  size_t query_row, perm, counts, cursor, row_count, slot_start, tile_start, tiles, route, bytes;
  size_t cleared_bytes;  // counts | cursor | row_count: contiguous, zero before the launch's first kernel (one memset from `counts`)
  GroupArrays(uint64_t nq, uint64_t rows, uint64_t tile_bound, bool routed = false) {
    query_row = 0;
    perm = query_row + nq;
    counts = perm + nq;
    cursor = counts + rows;
    row_count = cursor + rows;
    slot_start = row_count + rows;
    cleared_bytes = (slot_start - counts) * 4;
    tile_start = slot_start + rows + 1;
    tiles = tile_start + rows + 1;
    route = tiles + 3 * tile_bound;
    bytes = (route + (routed ? nq + 1 : 0)) * 4;
  }
};

// Filter routing of a filtered graph search ("filter_scan_max" / "filter_scan_on_overflow", scan_select.hpp): whether an
// option asks for it at all ...
inline bool filter_routing_on(const PlanInputs* ix) { return ix->filter_scan_max > 0 || ix->filter_scan_on_overflow != 0; }
// ... whether this launch over `filter_rows` node bitmaps (0: the call has no filter) routes, and the shape of its scan stage.
// Routing is not applied where the scan cannot take the call (K beyond its lists, rows too long for its LDS): an option
// never makes a valid call invalid.
struct ScanRouting {
  bool on = false;
  ScanShape shape{};
};
inline ScanRouting plan_scan_routing(const PlanInputs* ix, const RowGeometry& g, uint64_t nq, int K, uint64_t live, uint64_t filter_rows) {
  ScanRouting r;
  if (filter_rows == 0 || !filter_routing_on(ix) || K > SCAN_MAX_K) return r;
  r.shape = scan_shape(ix, g, nq, K, live, filter_rows);
  r.on = r.shape.lds <= kScanMaxLds;
  return r;
}
// HBM a routed launch takes on top of the search kernel's per-slot workspace: the node bitmaps, the grouping arrays with the
// route words, the partial lists.
inline size_t routed_scan_bytes(const PlanInputs* ix, uint64_t filter_rows, uint64_t nq, int K, const ScanShape& s) {
  return filter_rows_bytes(ix, filter_rows) + GroupArrays(nq, filter_rows, s.tiles, true).bytes + scan_partial_bytes(nq, s, K);
}

// The layouts fnv_tune times for one beam width: [0] the rules' own, then its neighbours.  `base_*`: what the rules chose
// for the merged-beam kernel (plan.sorted: table slots, tag width, whether the exact search's candidates heap is in LDS).
inline std::vector<LayoutChoice> tune_layout_candidates(const PlanInputs* ix, uint32_t base_slots, uint32_t base_vis_w, bool base_heap_lds) {
  std::vector<LayoutChoice> cands(1);  // [0]: the rules
  if (ix->tune_layout && ix->sorted_cand_lds == 2) {
    LayoutChoice c;
    c.cand_lds = base_heap_lds ? 0 : 1;
    cands.push_back(c);
  }
  if (ix->tune_layout && ix->visited_slots == 0 && base_slots >= 512) {
    const bool pow2 = (base_slots & (base_slots - 1)) == 0;
    const uint32_t up = pow2 ? base_slots / 2 * 3 : base_slots / 3 * 4, down = pow2 ? base_slots / 4 * 3 : base_slots / 3 * 2;
    // ... and two sizes up (round 5): beyond 2^24 nodes the tag format alternates with the size -- three 21-bit tags per
    // 8-byte bucket at 3 * 2^j slots, two 32-bit tags at 2^j -- so one size up from 3072 slots (4096: same bytes as 6144, a
    // third fewer tags) is a step DOWN in tags per byte and hides the layout that is 18 % faster on 50M x 128 Gaussian rows
    // (6144 slots at 8 queries per CU: 3.06 ms against the rules' 3072 slots at 12 per CU: 3.74 ms; profiles/r5_table_sizes_50m.txt)
    // (only where tags are wide: with 16-bit tags every size has the same format and the neighbours above suffice)
    const uint32_t up2 = base_vis_w != 16u ? base_slots * 2 : 0u;  // 3 * 2^j -> 3 * 2^(j+1): the same tag format
    // (two sizes DOWN was measured in round 6 and is not a candidate: on 50M x 128 uint8 -- 128-byte rows, 12 resident queries
    //  per CU -- 1536 slots keep 18-20 queries resident and are 32-48 % SLOWER than 3072 slots at 12: what a smaller table sends
    //  to the HBM bitmap costs more than the queries in flight it buys; profiles/r6_table_sizes_50m_uint8.txt)
    for (uint32_t slots : {up, down, up2}) {
      if (slots < 256 || slots > (1u << 15)) continue;
      LayoutChoice c;
      c.vis_slots = slots;
      cands.push_back(c);
      if (ix->sorted_cand_lds == 2) {
        c.cand_lds = base_heap_lds ? 0 : 1;
        cands.push_back(c);
      }
    }
  }
  return cands;
}

}  // namespace fnv_dev
