// launch_plan_harness.cpp -- test infrastructure (tests/test_launch_plan.py compiles it with g++ and loads it with ctypes; the
// product never does): runs the launch planner of flatnav_amd/csrc/launch_plan.hpp on the CPU.  The HIP runtime is replaced
// by the byte-wise occupancy count the planner's comments describe: lds > 163840 ? 0 : min(wave_cap, 163840 / max(lds, 1)).
//
// Every result is a row of int64 whose column names the harness itself exports (lph_*_columns), so that the Python side
// never repeats the layout of SearchParams.
#include "../flatnav_amd/csrc/launch_plan.hpp"

using namespace fnv_dev;

namespace {

struct Runtime {
  int wave_cap;
  int occupancy(int, uint32_t lds) const { return lds > 163840u ? 0 : std::min<int>(wave_cap, (int)(163840u / std::max<uint32_t>(lds, 1u))); }
  const char* raise_lds_limit(int, uint32_t) const { return nullptr; }
};

#define LPH_OPTIONS(X)                                                                                                         \
  X(visited_factor) X(visited_slots) X(visited_floor) X(occupancy_target) X(occupancy_roomy) X(cand_factor) X(cand_slots)     \
  X(spill_entries) X(blocks_per_cu) X(visited_wide) X(visited_tag_bits) X(sorted_beam) X(sorted_beam_min) X(sorted_cand_lds)  \
  X(sorted_tail_exact_pct) X(beam_registers) X(shadow_exact) X(tie_replay) X(tie_log_entries) X(visited_direct) X(overflow_list)
#define LPH_PARAMS(X)                                                                                                          \
  X(M) X(dim) X(row_bytes) X(nchunks) X(q_chunks) X(tail_chunks) X(q_lds_bytes) X(K) X(B) X(vis_slots) X(vis_shift) X(vis_limit) \
  X(vis_tag16) X(vis_w) X(vis_bytes) X(vis_nmask) X(vis_rshift) X(vis_rmask) X(vis_mult) X(cand_slots) X(spill_entries)       \
  X(bitmap_words) X(ovf_cap) X(log_entries) X(off_q) X(off_nbr) X(off_stage_d) X(off_cand) X(off_vis) X(off_stage_ids) X(off_ovf)

int64_t* put_params(int64_t* out, const SearchParams& p) {
#define LPH_PUT(f) *out++ = (int64_t)p.f;
  LPH_PARAMS(LPH_PUT)
#undef LPH_PUT
  return out;
}

struct Plan {
  PlanInputs ix;
  LaunchPlan plan;
  int rc = 0;
};

}  // namespace

extern "C" {

#define LPH_NAME(f) #f ","
const char* lph_option_columns() { return LPH_OPTIONS(LPH_NAME); }
const char* lph_param_columns() { return LPH_PARAMS(LPH_NAME); }
#undef LPH_NAME
// (the heaps block, then the sorted block, follow these)
// (ws_*: slot_workspace for the plan's beam -- bytes per query slot, by part and in all)
const char* lph_plan_columns() { return "rc,mode,cfg,full,row_bytes,tail_bytes,lds,bpc,slds,sbpc,ws_bitmap,ws_ovf,ws_spill,ws_tielog,ws_bytes,"; }
// (the launch's parameter block follows these)
const char* lph_shape_columns() {
  return "sorted,variant,multi_round,small_launch,shadow,nslots,tail_shadows,max_slots,tail_exact,scan_step,n_scan,direct,lds,bpc,mode,";
}

// The plan of (dtype, dim, M, capacity, num_cus, options in lph_option_columns order, B, K) under `wave_cap`; `parent_capacity`:
// of a view's source, else 0.  Returns a handle for lph_launch (free it with lph_free) and fills `out` (lph_plan_columns).
void* lph_plan(int dtype, uint32_t dim, uint32_t M, uint64_t capacity, uint64_t parent_capacity, int num_cus, const int64_t* options,
               int B, int K, int wave_cap, int64_t* out) {
  Plan* h = new Plan();
  PlanInputs& ix = h->ix;
#define LPH_SET(f) ix.f = *options++;
  LPH_OPTIONS(LPH_SET)
#undef LPH_SET
  ix.dtype = dtype;
  ix.dim = dim;
  ix.M = M;
  ix.capacity = capacity;
  ix.parent_capacity = parent_capacity;
  ix.num_cus = num_cus;
  const RowLayout lay = row_layout(dim, dtype, capacity);
  ix.row_bytes = lay.row_bytes;
  ix.tail_bytes = lay.tail_bytes;
  Runtime rt{wave_cap};
  std::string err;
  h->rc = plan_launch(&ix, B, K, LayoutChoice(), rt, err, h->plan);
  const LaunchPlan& p = h->plan;
  const SlotWorkspace ws = slot_workspace(&ix, log_entries_for(&ix, B));
  for (int64_t v : {(int64_t)h->rc, (int64_t)p.mode, (int64_t)p.cfg, (int64_t)p.full, (int64_t)ix.row_bytes, (int64_t)ix.tail_bytes,
                    (int64_t)p.lds, (int64_t)p.bpc, (int64_t)p.slds, (int64_t)p.sbpc, (int64_t)ws.bitmap, (int64_t)ws.ovf,
                    (int64_t)ws.spill, (int64_t)ws.tielog, (int64_t)ws.bytes()})
    *out++ = v;
  out = put_params(out, p.heaps);
  put_params(out, p.sorted);
  return h;
}
void lph_free(void* plan) { delete (Plan*)plan; }

// One unfiltered launch of `nq` queries over `live` nodes on that plan, shaped by the two planner calls search_device_impl
// shapes it with: the plan's default kernel choice, or `pinned` (>= 0: a variant, as fnv_tune pins it).  Fills `out`
// (lph_shape_columns).
void lph_launch(const void* plan, uint64_t nq, int num_initializations, uint64_t live, int pinned, int64_t* out) {
  const Plan* h = (const Plan*)plan;
  const KernelChoice c = default_choice(&h->ix, h->plan, nq, false, pinned);
  SearchParams p;
  const SearchLaunch s = shape_search(&h->ix, h->plan, c, 0, nq, num_initializations, live, p);
  for (int64_t v : {(int64_t)c.sorted, (int64_t)c.variant, (int64_t)c.multi_round, (int64_t)s.small_launch, (int64_t)s.shadow,
                    (int64_t)s.nslots, (int64_t)s.tail_shadows, (int64_t)s.max_slots, (int64_t)s.tail_exact, (int64_t)s.scan_step,
                    (int64_t)s.n_scan, (int64_t)s.direct, (int64_t)s.lds, (int64_t)s.bpc, (int64_t)s.mode})
    *out++ = v;
  put_params(out, p);
}

// `n` cases in one call (rows of `cases`: dtype, dim, M, capacity, parent_capacity, num_cus, B, K, wave_cap, then the
// options), each planned and launched with every nqs[j] (live = capacity, pinned = -1): plans [n][plan_width],
// shapes [n][n_nq][shape_width].
void lph_sweep(const int64_t* cases, int64_t n, int64_t case_width, const int64_t* nqs, int n_nq, int num_initializations,
               int64_t* plans, int64_t plan_width, int64_t* shapes, int64_t shape_width) {
  for (int64_t i = 0; i < n; i++) {
    const int64_t* c = cases + i * case_width;
    void* h = lph_plan((int)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint64_t)c[3], (uint64_t)c[4], (int)c[5], c + 9, (int)c[6], (int)c[7],
                       (int)c[8], plans + i * plan_width);
    for (int j = 0; j < n_nq; j++) {
      int64_t* row = shapes + (i * n_nq + j) * shape_width;
      if (((const Plan*)h)->rc == FNV_OK) lph_launch(h, (uint64_t)nqs[j], num_initializations, (uint64_t)c[3], -1, row);
      else std::fill(row, row + shape_width, (int64_t)-1);
    }
    lph_free(h);
  }
}

// The exhaustive scan's shape and the routing decision.  Rows of `cases`: dtype, dim, capacity, num_cus, scan_segment_rows,
// filter_scan_max, filter_scan_on_overflow, nq, K, live, filter_rows; rows of `out` (lph_scan_columns): scan_shape's fields for
// that call, the row's q_chunks, the partial lists' bytes, the merge's LDS, and whether plan_scan_routing routes it.
const char* lph_scan_columns() { return "tile,tiles,segments,lds,q_chunks,partial_bytes,merge_lds,routed,"; }
void lph_scan_sweep(const int64_t* cases, int64_t n, int64_t* out) {
  for (int64_t i = 0; i < n; i++, cases += 11) {
    PlanInputs ix;
    ix.dtype = (int)cases[0], ix.dim = (uint32_t)cases[1], ix.capacity = (uint64_t)cases[2], ix.num_cus = (int)cases[3];
    ix.scan_segment_rows = cases[4], ix.filter_scan_max = cases[5], ix.filter_scan_on_overflow = cases[6];
    const RowLayout lay = row_layout(ix.dim, ix.dtype, ix.capacity);
    ix.row_bytes = lay.row_bytes, ix.tail_bytes = lay.tail_bytes;
    const RowGeometry g = row_geometry(&ix);
    const uint64_t nq = (uint64_t)cases[7], live = (uint64_t)cases[9], rows = (uint64_t)cases[10];
    const ScanShape s = scan_shape(&ix, g, nq, (int)cases[8], live, rows);
    for (int64_t v : {(int64_t)s.tile, (int64_t)s.tiles, (int64_t)s.segments, (int64_t)s.lds, (int64_t)g.q_chunks,
                      (int64_t)scan_partial_bytes(nq, s, (int)cases[8]), (int64_t)scan_merge_lds((uint32_t)cases[8]),
                      (int64_t)plan_scan_routing(&ix, g, nq, (int)cases[8], live, rows).on})
      *out++ = v;
  }
}
// GroupArrays(nq, rows, tile_bound, routed): its ten offsets in declaration order, then cleared_bytes.
void lph_group_arrays(uint64_t nq, uint64_t rows, uint64_t tile_bound, int routed, int64_t* out) {
  const GroupArrays ga(nq, rows, tile_bound, routed != 0);
  for (size_t v : {ga.query_row, ga.perm, ga.counts, ga.cursor, ga.row_count, ga.slot_start, ga.tile_start, ga.tiles, ga.route, ga.bytes,
                   ga.cleared_bytes})
    *out++ = (int64_t)v;
}
// K0's tile (entry_scan_tile): stride, rows, lds, grid.
void lph_entry_scan_tile(uint32_t row_bytes, uint32_t q_chunks, uint32_t n_scan, uint64_t nq, int64_t* out) {
  const EntryScanTile t = entry_scan_tile(row_bytes, q_chunks, n_scan, nq);
  for (int64_t v : {(int64_t)t.stride, (int64_t)t.rows, (int64_t)t.lds, (int64_t)t.grid}) *out++ = v;
}

// The variant rules.  which: 0 pinned_variant(pinned), 1 lane_variant, 2 owner_next_sample, 3 owner_final_variant.
int lph_variant(int which, const float* best, const int* samples, int multi_round, int try_tail, int shadows_on, int pinned) {
  Tuner t;
  for (int v = 0; v < kNumVariants; v++) t.best[v] = best[v], t.samples[v] = samples[v];
  switch (which) {
    case 0: return pinned_variant(pinned, multi_round != 0, shadows_on != 0);
    case 1: return lane_variant(t, multi_round != 0, try_tail != 0, shadows_on != 0);
    case 2: return owner_next_sample(t, multi_round != 0, try_tail != 0, shadows_on != 0);
    default: return owner_final_variant(t, multi_round != 0, try_tail != 0, shadows_on != 0);
  }
}
int lph_variant_allowed(int v, int multi_round, int try_tail, int shadows_on, int pinned_only) {
  return variant_allowed(v, multi_round != 0, try_tail != 0, shadows_on != 0, pinned_only != 0);
}

// Row configuration `cfg` of kCfgs: its lanes per row (G) and chunks per lane and span (CU).  Returns the number of
// configurations, so that tests/row_classes.py never repeats the table.
int lph_row_cfg(int cfg, int* G, int* CU) {
  if (cfg >= 0 && cfg < kNumCfgs) *G = kCfgs[cfg].G, *CU = kCfgs[cfg].CU;
  return kNumCfgs;
}

// Query slots of `lds` bytes that the LDS of one CU holds (whole granules).
int lph_slots_per_cu(uint32_t lds) { return (int)(kLdsPerCu / lds_allocated(lds)); }

// fnv_tune's candidate layouts around (base_slots, base_vis_w, base_heap_lds) under default options: (cand_lds, vis_slots) pairs.
int lph_tune_candidates(uint32_t base_slots, uint32_t base_vis_w, int base_heap_lds, int64_t* out, int max_pairs) {
  PlanInputs ix;
  const std::vector<LayoutChoice> cands = tune_layout_candidates(&ix, base_slots, base_vis_w, base_heap_lds != 0);
  for (size_t i = 0; i < cands.size() && (int)i < max_pairs; i++) out[2 * i] = cands[i].cand_lds, out[2 * i + 1] = cands[i].vis_slots;
  return (int)cands.size();
}

}  // extern "C"
