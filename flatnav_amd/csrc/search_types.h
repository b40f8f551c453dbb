// search_types.h -- part of the gfx950 search engine: the launch constants and the kernel parameter block, in plain C++.
// No HIP header: the device code includes it through search_params.h / kernel_table.h, the launch planner (launch_plan.hpp)
// and its CPU test harness include it as it is.
#pragma once
#include <stdint.h>

namespace fnv_dev {

constexpr uint32_t EMPTY_ID = 0xFFFFFFFFu;
constexpr int WAVE = 64;

constexpr int MB_R = 4;                   // merged-beam kernel: 64-entry chunks of the beam held in registers
constexpr int MB_MAX_BEAM = MB_R * WAVE;  // ... = the widest beam it serves

enum : int { ST_OK = 0, ST_CAND_OVERFLOW = 1 };
enum : uint32_t { SH_NONE = 0u, SH_ANSWERED = 1u, SH_SHADOW = 2u, SH_OWN_RERUN = 3u };  // done_flags (exact shadows, below)
constexpr int SCAN_WAVES = 4;  // entry_scan_kernel (K0): waves per workgroup ...
constexpr int SCAN_QPB = 32;   // ... and queries per workgroup
constexpr uint32_t OVF_LIST = 30;  // ids remembered for a cheap clean-up of the HBM visited bitmap
// Round 3: a STASH of full ids behind the tag table (the "stash" of cuckoo hashing): an id whose two buckets are both full
// goes there first, and only when its stash bucket is full as well to the slot's HBM bitmap (visited.hpp).  At the load
// factors the layouts run at (40-65 %) a query overflows a few dozen ids: with the stash they never leave LDS, and a
// smaller table -- more resident queries -- no longer pays a dependent HBM round trip for them.  LDS: STASH words
// after the overflow list, at [OVF_LIST + 2 ...).
constexpr uint32_t STASH = 64;

struct SearchParams {
  const uint8_t* vectors;   // [n_nodes][row_bytes]
  const uint8_t* tails;     // split rows (round 6, distance.hpp): [n_nodes][tail_chunks * 16] -- the last chunks of every row, in a
                            // dense side table, when that lets the main table hold whole 128-byte lines only; else null
  const uint32_t* links;    // [n_nodes][M]
  const int32_t* labels;    // [n_nodes]
  const uint8_t* queries;   // [nq][dim] elements, dense
  float* out_dist;          // [nq][K]
  int32_t* out_labels;      // [nq][K]
  int32_t* out_count;       // [nq] or null
  uint64_t* out_ndist;      // [nq] or null
  uint64_t* out_nhops;      // [nq] or null
  uint32_t* dispenser;      // zero at launch; next work item = gridDim.x + its value (a slot's first item is its block index)
  uint32_t* redo_count;     // merged-beam kernel: [0] queries it handed to the exact search (equal keys at a decision),
                            // [1..4] by reason, [5] of them resumed from their log, [6] hops taken from the logs,
                            // [7] hops the merged-beam passes of the resumed queries had made
  int32_t* status;          // sticky error flag for the whole launch
  int32_t* host_status;     // (round 6, zero-copy small searches) the same flag in the caller's pinned result slab, or null
  uint32_t* ovf_bitmap;     // [nslots][bitmap_words] visited-set spill (all zero between queries)
  uint32_t* ovf_glist;      // [nslots][ovf_cap] ids sent to the bitmap beyond the first OVF_LIST (big indexes only)
  unsigned long long* cand_spill;  // [nslots][spill_entries]
  const uint32_t* entry_node;  // [nq] from entry_scan_kernel (null: scan inside the search kernel)
  const float* entry_dist;     // [nq]
  uint32_t* entry_node_out;    // entry_scan_kernel outputs
  float* entry_dist_out;
  uint32_t scan_tile_rows, scan_tile_stride;  // entry_scan_kernel: LDS tile geometry
  unsigned long long* phase_cycles;  // [16] profiling build only (FNV_PHASE_TIMING), else null
  uint64_t n_nodes;
  uint32_t nq, M, dim, row_bytes, nchunks, q_chunks;  // (split rows: row_bytes / nchunks describe the main table)
  uint32_t tail_chunks;    // split rows: 16-byte chunks per row in `tails` (1 or 2), else 0
  uint32_t q_lds_bytes;    // LDS the staged query takes per slot: q_chunks * 16, or 0 when it lives in registers (distance.hpp)
  int K, B;
  uint32_t n_scan, scan_step;
  uint32_t vis_slots, vis_shift, vis_limit;
  uint32_t vis_tag16;      // 1: bucketed tag table (below; tag width vis_w), 0: 32-bit open addressing
  uint32_t vis_w;          // 16: four tags per 8-byte bucket; 21 / 32: three / two tags per 64-bit bucket;
                           // 1 (round 5, small launches on small indexes): no table -- a bitmap of all node ids, vis_bytes long
  uint32_t vis_bytes;      // LDS bytes of the table
  uint32_t vis_nmask, vis_rshift, vis_rmask;  // tag16: 2^nbits-1, t = nbits-k, 2^t-1
  uint32_t vis_mult;       // tag16: buckets = vis_mult * 2^k with vis_mult in {1, 3}
  uint32_t off_ovf;        // LDS: [0] count, [1..OVF_LIST] ids that went to the HBM bitmap, [OVF_LIST + 2 ...) the stash
  uint32_t cand_slots, spill_entries, bitmap_words, ovf_cap;
  uint32_t off_q, off_nbr, off_cand, off_vis, off_stage_ids;
  uint32_t off_stage_d;     // LDS: [WAVE + 1] distances of a link row's unvisited neighbours (merged-beam kernel; = off_nbr:
                            // the permutation buffer is idle while they are staged)
  uint32_t tail_exact;     // merged-beam kernel: the last tail_exact queries of the launch skip the sorted pass
  // Exact shadows.  Work items >= shadow_base (= the number of queries) are exact (two-heap) searches of the LAST queries of
  // the launch, most recently dispensed first: item shadow_base + k shadows query shadow_base - 1 - k; nq (the dispenser's
  // limit) = queries + shadows.  A slot only ever pulls a shadow once every query has been handed out, i.e. when it would
  // otherwise go idle, and the queries it shadows first are the ones whose merged-beam search has only just begun.  One
  // word per query, done_flags[shadow_base] (zero at launch), settles who answers it:
  //   SH_NONE -> SH_ANSWERED    its merged-beam pass finished without a tie: a shadow stops at its next hop / never starts
  //   SH_NONE -> SH_SHADOW      a shadow claimed it: a merged-beam pass that meets a tie later does NOT search it again
  //   SH_NONE -> SH_OWN_RERUN   the merged-beam pass met a tie first and searches it again itself: no shadow starts
  // Both write the same bytes when both finish.  Two uses: small launches (at most a quarter of the slots: every query has a
  // shadow from the start; round 3) and -- round 4, "tail shadows" -- the end of ANY launch: instead of sending the whole last
  // round through the slower exact kernel so that no re-run becomes a straggler, every query runs the merged-beam kernel and
  // the slots that the drain leaves idle run the exact search of the queries still under way; a tie then costs one
  // exact-search latency from the query's start, paid by a slot that had nothing else to do.  0 = off.
  uint32_t shadow_base;
  uint32_t* done_flags;
  // Round 5: the hand-over log of the merged-beam kernel (kernels.hpp): log_entries 8-byte records per slot (0: no log --
  // a query in which equal keys meet at a decision is then searched again from scratch, as in rounds 2-4)
  unsigned long long* tie_log;  // [nslots][log_entries]
  uint32_t log_entries;
  // Filtered search (beam_search_filtered_kernel only): bit (i & 31) of word i >> 5 set = node i may be a result; null elsewhere.
  // (Behind every other kernel's fields: their parameter offsets stay as they were.)
  const uint32_t* node_bits;
  // Grouped filtered search (one filter per query): node_bits holds n_filters + 2 rows of filter_words words each (scan_select.hpp,
  // filter_row) and query q reads row filter_row(query_filter[q], n_filters).  query_filter null = a single-filter launch: row 0.
  const int32_t* query_filter;  // [nq]
  uint32_t filter_words;
  uint32_t n_filters;
  // Filter routing (beam_search_filtered_kernel only; scan_select.hpp, "filter routing"): [nq] route words and, at [nq], whether a
  // candidates heap that overflows hands its query to the scan.  A query whose word is not ROUTE_GRAPH at launch is skipped; null =
  // no routing.  (Cold, and behind every other field again.)
  uint32_t* query_route;
  // The handle's OTHER dispenser block (runtime.hpp, fnv_index_s::d_dispenser): this launch zeroes its 16 words for the launch
  // that follows it on the handle and touches it in no other way; null: nothing to zero.
  uint32_t* dispenser_next;
};

// The fields of the visited-table geometry that the per-hop probe needs (kept in scalar registers).
struct VisGeom {
  uint32_t nmask, rshift, rmask, mult, w;
};

// chunks covered per inner iteration = G*CU: 8,16,32,64,128,256 (128 B ... 4 KiB of a row), and 192 for rows of
// exactly 3 KiB (768-d float32: no clamped loads, four vectors in flight -- passes<64,3>)
struct KernelCfg {
  int G, CU;
};
// ... and 24 for rows of three whole lines: FULL = plain 384-byte rows, non-FULL = SPLIT rows (three lines in the main table +
// one or two chunks in the side table; distance.hpp row_has_tail)
constexpr KernelCfg kCfgs[] = {{8, 1}, {8, 2}, {8, 4}, {16, 4}, {32, 4}, {64, 4}, {64, 3}, {8, 3}};
constexpr int kNumCfgs = 8;
constexpr int kCfgThreeLines = 7;

// Row configuration for rows of `nchunks` 16-byte chunks: the narrowest one that covers the row in one span; longer
// rows loop over 256-chunk spans.  Rows of exactly 192 chunks (768-d float32) have their own: every lane loads exactly
// its three chunks, and the query lives in registers instead of LDS (distance.hpp, query_in_regs).
inline bool cfg_query_in_regs(int cfg) { return kCfgs[cfg].G == 64 && kCfgs[cfg].CU == 3; }
inline int pick_row_cfg(uint32_t nchunks, uint32_t tail_chunks = 0) {
  if (tail_chunks) return kCfgThreeLines;  // (the host splits rows of exactly 24 main chunks only)
  if (nchunks == 192) return 6;
  if (nchunks == 24) return kCfgThreeLines;
  for (int c = 0; c < 6; c++)
    if ((uint32_t)(kCfgs[c].G * kCfgs[c].CU) >= nchunks) return c;
  return 5;
}

// Forms of the merged-beam kernel (merged_beam.hpp): the beam in LDS (any width), or in one / two / MB_R 64-entry chunks of
// registers (beams of at most 64 / 128 / 256 entries) -- the kernel's R argument.
constexpr int kNumBeamForms = 4;
constexpr int kBeamFormR[kNumBeamForms] = {0, 1, 2, MB_R};
inline int beam_form(bool lds, int B) { return lds ? 0 : B <= WAVE ? 1 : B <= 2 * WAVE ? 2 : 3; }

}  // namespace fnv_dev
