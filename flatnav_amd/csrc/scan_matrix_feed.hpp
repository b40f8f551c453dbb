// scan_matrix_feed.hpp -- part of the gfx950 search engine (device code; included by the three matrix engines of the exhaustive
// search: scan_matrix.hpp, scan_matrix_f16.hpp, scan_matrix_f32.hpp).
// WHERE A GROUPED CALL'S ROWS COME FROM.  An engine scores 32-row tiles: the rows are the MFMA's M.  Each engine is ONE kernel
// template over the kind of call: the scoring is shared, the walk over the candidates is not.  An ungrouped kernel keeps its own
// walk over slots [lo, hi) of an id list, word for word as it was -- with the walk behind a common interface the compiler
// allocated the ungrouped kernels' registers differently, so they keep their text and compile to the same code as before.  A
// grouped kernel asks the feeder four things:
//     more()        is there a current tile                                             (wave-uniform)
//     nrows()       its rows, 1 .. 32; a short tile is the segment's last              (wave-uniform)
//     row(k, &id)   this lane's row (lane % 32) of the current tile (k = 0) or of the one after it (k = 1); false, and row 0 --
//                   a legal address whose data the engine discards -- where the tile has no such row or does not exist
//     advance()     the tile after the current one becomes the current one
// THE CONTRACT that lets an engine request tile k = 1 from HBM while it scores tile 0: between two calls of advance() the answers
// never change, and what row(1, ..) says before advance() is what row(0, ..) says after it.
//
// MatrixRowFeeder: a grouped call ("scan_matrix_grouped").  The candidates are the bits set in words [wlo, whi) of ONE filter
// row's node bitmap -- there is no id list, and building one per filter row would cost a pass and n ids of HBM per row.  The
// wavefront walks the words 64 a step (lane l: word w + l), the step after it already requested (`ahead`), so that a sparse row,
// where a step yields a handful of ids, does not wait for a load per step.  Set bits become node ids in an LDS queue: a wave prefix
// over the words' popcounts gives every lane the place of its word's ids, the words that fit the queue's free room -- a prefix of
// the lanes -- are appended whole, the others keep their bits for the next refill.  Tiles are handed out from the queue's head.
// Refills happen in advance() only, and only when fewer than TWO tiles are queued: the leftovers (at most 63 ids) move to the
// front, then words are appended until two tiles are there or the words are used up.  Hence the invariant
//     after construction and after every advance():  the queue holds at least 64 ids, or no word is left,
// which is the contract above: the tile after the current one is either full or the segment's last, and no later refill changes
// it.  Every set bit is queued exactly once (a word is appended whole and zeroed, or not at all) and leaves the queue in exactly
// one tile, whichever way the words split across refills; which tile a node falls into never shows, since the order of the
// results is total (scan_select.hpp).  Progress: a refill starts with at most 63 ids queued and a word holds at most 32, so the
// first word with a bit set always fits -- MATRIX_QUEUE_IDS >= 95, asserted below.
#pragma once
#include "scan.hpp"
namespace fnv_dev {

constexpr uint32_t MATRIX_TILE_ROWS = 32;  // the MFMA's M
static_assert(2u * MATRIX_TILE_ROWS <= (uint32_t)WAVE && 2u * MATRIX_TILE_ROWS - 1u + 32u <= MATRIX_QUEUE_IDS,
              "leftovers move in one step, and a word always fits behind them");

// One kernel template serves both kinds of call: its parameter block is ScanParams or GroupedScanParams.
__device__ __forceinline__ const ScanParams& matrix_scan_params(const ScanParams& p) { return p; }
__device__ __forceinline__ const ScanParams& matrix_scan_params(const GroupedScanParams& gp) { return gp.s; }
__device__ __forceinline__ const GroupedScanParams* matrix_grouped_params(const ScanParams&) { return nullptr; }
__device__ __forceinline__ const GroupedScanParams* matrix_grouped_params(const GroupedScanParams& gp) { return &gp; }

// What an ungrouped kernel has in the feeder's place: nothing (its candidates are slots of an id list or the live nodes).
struct MatrixNoFeeder {
  __device__ __forceinline__ MatrixNoFeeder(uint32_t*, const GroupedScanParams*, uint32_t, uint32_t, uint32_t, int) {}
  __device__ __forceinline__ bool more() const { return false; }
  __device__ __forceinline__ uint32_t nrows() const { return 0u; }
  __device__ __forceinline__ bool row(int, uint32_t*) const { return false; }
  __device__ __forceinline__ void advance() {}
};

struct MatrixRowFeeder {
  uint32_t* queue;       // LDS, MATRIX_QUEUE_IDS entries
  const uint32_t* bits;  // the filter row's words
  uint32_t cur, next, whi;  // `word` is word cur + lane, `ahead` word next + lane; the segment ends at whi   (wave-uniform)
  uint32_t word, ahead;     // this lane's word of the step being queued (the bits not yet queued) and of the step after it
  uint32_t head, count;     // the queue holds ids [head, count)                                              (wave-uniform)
  int lane;

  __device__ __forceinline__ uint32_t load(uint32_t w0) const { return w0 + (uint32_t)lane < whi ? bits[w0 + (uint32_t)lane] : 0u; }
  // The words of filter row `row` that row segment `seg` of `segments` covers, queued up to two tiles.
  __device__ __forceinline__ MatrixRowFeeder(uint32_t* q, const GroupedScanParams* gp, uint32_t row, uint32_t seg, uint32_t segments, int lane_)
      : queue(q), bits(gp->node_bits + (uint64_t)row * gp->row_words), cur((uint32_t)((uint64_t)gp->live_words * seg / segments)), next(cur),
        whi((uint32_t)((uint64_t)gp->live_words * (seg + 1) / segments)), word(0u), head(0u), count(0u), lane(lane_) {
    ahead = load(next);
    refill();
  }
  // Words into the queue until it holds two tiles or none is left.  On entry fewer than 64 ids are queued.
  __device__ __forceinline__ void refill() {
    if (head) {  // the leftovers to the front: one lane each
      const uint32_t rem = count - head;
      uint32_t keep = 0;
      if ((uint32_t)lane < rem) keep = queue[head + (uint32_t)lane];
      wave_sync();
      if ((uint32_t)lane < rem) queue[lane] = keep;
      head = 0u;
      count = rem;
    }
    while (count < 2u * MATRIX_TILE_ROWS) {
      if (!__ballot(word != 0u)) {  // this step is used up: the one requested ahead, and the request after it
        if (next >= whi) break;
        cur = next;
        word = ahead;
        next += (uint32_t)WAVE;
        ahead = load(next);
        continue;
      }
      const uint32_t pc = (uint32_t)__popc(word);
      uint32_t incl = pc;  // ids of lanes [0, lane]
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, WAVE);
        if (lane >= off) incl += up;
      }
      const bool fits = count + incl <= MATRIX_QUEUE_IDS;  // (incl never decreases along the lanes: a prefix of them)
      const int nfit = __popcll(__ballot(fits));            // through the first word with a bit at least: count <= 63 here
      if (fits) {
        uint32_t at = count + incl - pc;
        while (word) {
          queue[at++] = (cur + (uint32_t)lane) * 32u + (uint32_t)(__ffs((int)word) - 1);
          word &= word - 1u;
        }
      }
      count += (uint32_t)__shfl((int)incl, nfit - 1, WAVE);
    }
    wave_sync();
  }
  __device__ __forceinline__ bool more() const { return head < count; }
  __device__ __forceinline__ uint32_t nrows() const { return min(MATRIX_TILE_ROWS, count - head); }
  __device__ __forceinline__ bool row(int k, uint32_t* id) const {
    const uint32_t slot = head + (uint32_t)k * MATRIX_TILE_ROWS + ((uint32_t)lane & (MATRIX_TILE_ROWS - 1u));
    const bool valid = slot < count;
    *id = valid ? queue[slot] : 0u;
    return valid;
  }
  __device__ __forceinline__ void advance() {
    head = min(head + MATRIX_TILE_ROWS, count);
    if (count - head < 2u * MATRIX_TILE_ROWS && (next < whi || __ballot(word != 0u))) refill();
  }
};

}  // namespace fnv_dev
