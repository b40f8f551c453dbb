// launch.hip -- one search launch of the host runtime (runtime.hpp): kernel lookup, the cached launch plan, the measurements
// of the adaptive kernel choice, the workspace, the filter bitmaps, the graph search's and the exhaustive scan's launches as
// sequences of named steps, the status word, and the entry points that take device buffers.  What a launch looks like -- its
// shape, LDS bytes, tiles, segments, byte counts -- is asked of the planner (launch_plan.hpp); here are the HIP calls.
// The only host unit that includes scan.hpp (its non-template kernels).
#include "runtime.hpp"
#ifdef FNV_DEV_FAST_BUILD
#include "kernels.hpp"
#include "merged_beam.hpp"
#endif
#include "scan.hpp"

namespace fnv_dev {

// Filtered search: node_bits[w] bit b = label_allowed(labels[32 w + b]) for the live nodes, 0 past them.  allowed_bits is a
// bitmap over label VALUES (byte L >> 3, bit L & 7); a label that is negative or >= n_bits is not allowed.  One thread per
// node; a wave's 64 verdicts are two words.
__global__ __launch_bounds__(256) void node_filter_kernel(const int32_t* labels, uint64_t n_live, uint64_t n_words,
                                                          const uint8_t* allowed_bits, uint64_t n_bits, uint32_t* node_bits) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (i < n_live) {
    const int32_t L = labels[i];
    ok = L >= 0 && (uint64_t)L < n_bits && ((allowed_bits[(uint32_t)L >> 3] >> (L & 7)) & 1u);
  }
  const unsigned long long m = __ballot(ok);
  const int lane = (int)(threadIdx.x & (WAVE - 1));
  const uint64_t w = i >> 5;
  if ((lane & 31) == 0 && w < n_words) node_bits[w] = (uint32_t)(lane ? m >> 32 : m);
}

// Grouped filtered search: the same rule for a TABLE of n_filters label bitmaps (filter f at allowed_bits + f * stride_bytes,
// one n_bits for all) in one launch, the filter on the grid's second dimension: node_bits[r][n_words].  Two fixed rows follow
// the filters' (scan_select.hpp, filter_row): row n_filters holds every live node, row n_filters + 1 none.
// row_count (null: not wanted) [n_filters + 2], zero at launch: the nodes set in each row -- the block's four wavefronts add up in
// LDS first, so a row takes one global atomic per 256 nodes that has any bit set.
__global__ __launch_bounds__(256) void node_filter_table_kernel(const int32_t* labels, uint64_t n_live, uint64_t n_words,
                                                                const uint8_t* allowed_bits, uint64_t stride_bytes, uint64_t n_bits,
                                                                uint32_t n_filters, uint32_t* node_bits, uint32_t* row_count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & (WAVE - 1));
  const uint64_t w = i >> 5;
  const bool live = i < n_live;
  const int32_t L = live ? labels[i] : -1;
  const bool in_range = L >= 0 && (uint64_t)L < n_bits;
  __shared__ uint32_t wave_pop[4];
  for (uint32_t r = blockIdx.y; r < n_filters + 2u; r += gridDim.y) {  // (the grid's second dimension ends at 65535)
    bool ok = live && r == n_filters;
    if (r < n_filters && in_range) ok = (allowed_bits[(uint64_t)r * stride_bytes + ((uint32_t)L >> 3)] >> (L & 7)) & 1u;
    const unsigned long long m = __ballot(ok);
    if ((lane & 31) == 0 && w < n_words) node_bits[(uint64_t)r * n_words + w] = (uint32_t)(lane ? m >> 32 : m);
    if (row_count) {  // (uniform over the block)
      if (lane == 0) wave_pop[threadIdx.x / WAVE] = (uint32_t)__popcll(m);
      __syncthreads();
      if (threadIdx.x == 0) {
        const uint32_t total = wave_pop[0] + wave_pop[1] + wave_pop[2] + wave_pop[3];
        if (total) atomicAdd(row_count + r, total);
      }
      __syncthreads();
    }
  }
}

}  // namespace fnv_dev

// hipFuncAttributeMaxDynamicSharedMemorySize is global per (kernel, device) while several handles (views, replicas on
// one device) launch concurrently with different beam widths: the limit is only ever RAISED, under one process-wide
// mutex -- set(A), set(B < A), launch(A) cannot happen.  (A larger limit than a launch needs costs nothing: residency
// follows the bytes the launch asks for.)
hipError_t raise_lds_limit(const void* kern, int device, uint32_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, uint32_t> limit;
  std::lock_guard<std::mutex> lock(mu);
  uint32_t& have = limit[{device, kern}];
  if (bytes <= have) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

namespace {

// ---- kernel lookup ----------------------------------------------------------------------------------------------
#ifdef FNV_DEV_FAST_BUILD
// Developer builds (-DFNV_DEV_FAST_BUILD): ONE translation unit, ONE instantiation per kernel -- element type
// FNV_DEV_T, metric FNV_DEV_METRIC, G = FNV_DEV_G, CU = FNV_DEV_CU, FULL rows -- compiles in seconds (float/8/4: 128-d f32
// rows; unsigned char/8/1: 128-d u8 rows; float/64/3 with FNV_METRIC_IP: 768-d inner product).  Every table slot points at it.
#ifndef FNV_DEV_T
#define FNV_DEV_T float
#endif
#ifndef FNV_DEV_CU
#define FNV_DEV_CU 4
#endif
#ifndef FNV_DEV_G
#define FNV_DEV_G 8
#endif
#ifndef FNV_DEV_METRIC
#define FNV_DEV_METRIC FNV_METRIC_L2
#endif
#define FNV_DEV_KERNEL(K, ...) K<FNV_DEV_T, FNV_DEV_METRIC, FNV_DEV_G, FNV_DEV_CU, true __VA_ARGS__>
constexpr bool kHalfRowsBuilt = false;  // (one instantiation per kernel: no mirror-row kernels)
const KernelTable& kernel_table(int, int, bool = false) {
  static KernelTable t = [] {
    KernelTable k;
    const kernel_fn merged[kNumBeamForms][2] = {
        {FNV_DEV_KERNEL(beam_search_merged_kernel, , 0), FNV_DEV_KERNEL(beam_search_merged_kernel, , 0, true)},
        {FNV_DEV_KERNEL(beam_search_merged_kernel, , 1), FNV_DEV_KERNEL(beam_search_merged_kernel, , 1, true)},
        {FNV_DEV_KERNEL(beam_search_merged_kernel, , 2), FNV_DEV_KERNEL(beam_search_merged_kernel, , 2, true)},
        {FNV_DEV_KERNEL(beam_search_merged_kernel, , MB_R), FNV_DEV_KERNEL(beam_search_merged_kernel, , MB_R, true)}};
    for (int c = 0; c < kNumCfgs; c++)
      for (int f = 0; f < 2; f++) {
        k.exact[c][f] = FNV_DEV_KERNEL(beam_search_kernel);
        k.exact_f[c][f] = FNV_DEV_KERNEL(beam_search_filtered_kernel);
        k.scan[c][f] = FNV_DEV_KERNEL(entry_scan_kernel);
        for (int form = 0; form < kNumBeamForms; form++)
          for (int d = 0; d < 2; d++) k.merged[form][d][c][f] = merged[form][d];
        k.select[c][f] = FNV_DEV_KERNEL(wire_select_kernel);
        k.connect[c][f] = FNV_DEV_KERNEL(wire_connect_kernel);
        k.flat[c][f] = FNV_DEV_KERNEL(exhaustive_scan_kernel);
        k.flat_g[c][f] = FNV_DEV_KERNEL(exhaustive_scan_grouped_kernel);
      }
    return k;
  }();
  return t;
}
#undef FNV_DEV_KERNEL
#else
// Product builds: the instantiations live in kernel_inst.hip objects (one per family x element type x metric).
// `half_rows`: the tables of the row format f32h (float32 queries on mirror rows, half_rows.hpp; float32 indexes only) -- the
// exact and merged-beam kernels of the row configurations a mirror exists for, null everywhere else.
constexpr bool kHalfRowsBuilt = true;
const KernelTable& kernel_table(int dtype, int metric, bool half_rows = false) {
  static KernelTable tables[10];  // (static: zero-initialised -- the slots no filler writes are null)
  static std::once_flag once;
  std::call_once(once, [] {
    int i = 0;
#define FNV_FILL_FAMILY(ordinal, family, tag, mtag) fill_##family##_##tag##_##mtag(tables[i]);
#define FNV_FILL(T, tag, M, mtag)                       \
    FNV_FOR_EACH_FAMILY(FNV_FILL_FAMILY, tag, mtag) \
    i++;
    FNV_FOR_EACH_TYPE_METRIC(FNV_FILL)
#undef FNV_FILL
#define FNV_FILL(M, mtag)                                          \
    FNV_FOR_EACH_HALF_ROWS_FAMILY(FNV_FILL_FAMILY, f32h, mtag) \
    i++;
    FNV_FOR_EACH_HALF_ROWS_METRIC(FNV_FILL)
#undef FNV_FILL
#undef FNV_FILL_FAMILY
  });
  if (half_rows) return tables[8 + (metric == FNV_METRIC_IP ? 1 : 0)];
  int t;  // order of FNV_FOR_EACH_TYPE_METRIC; every caller has passed validate_geometry (dtype_size != 0)
  switch (dtype) {
    case FNV_DTYPE_FLOAT32: t = 0; break;
    case FNV_DTYPE_UINT8: t = 1; break;
    case FNV_DTYPE_INT8: t = 2; break;
    case FNV_DTYPE_FLOAT16: t = 3; break;
    default: fprintf(stderr, "flatnav_hip: kernel_table(%d): unsupported data type\n", dtype); abort();  // (unreachable)
  }
  return tables[2 * t + (metric == FNV_METRIC_IP ? 1 : 0)];
}
#endif

kernel_fn pick_scan_kernel(int dtype, int metric, int cfg, bool full) { return kernel_table(dtype, metric).scan[cfg][full]; }

}  // namespace

wire_fn pick_wire_kernel(int dtype, int metric, int cfg, bool full) { return kernel_table(dtype, metric).select[cfg][full]; }
wire_fn pick_connect_kernel(int dtype, int metric, int cfg, bool full) { return kernel_table(dtype, metric).connect[cfg][full]; }

// Whether this handle's rows can have one at all: float32 rows of an eligible geometry, in a build that has the kernels.
bool half_rows_possible(const fnv_index_s* ix) {
  return kHalfRowsBuilt && !ix->half.off && half_rows_eligible(ix->dtype, row_geometry(ix));
}

// The status word of a launch -> the call's result (`advice`: how each caller has always ended the message).
int check_status(int32_t st, const char* advice) {
  if (st == ST_CAND_OVERFLOW) return fail(FNV_ERR_CAPACITY, std::string("candidate heap overflowed its HBM spill area; ") + advice);
  return FNV_OK;
}
int check_device_status(fnv_index_s* ix, const char* advice) {  // (the stream has been waited for)
  int32_t st = 0;
  HIP_TRY(hipMemcpy(&st, ix->last_block + 1, sizeof(int32_t), hipMemcpyDeviceToHost));  // (the most recent launch's block)
  return check_status(st, advice);
}
// The dispenser block of the launch that is about to be enqueued on `stream`, zero when its kernel starts (THE RULE:
// runtime.hpp, d_dispenser): the other block than the most recent launch's; the host's memset unless that launch's kernel
// zeroes exactly this block ahead of us on the same stream.  The caller holds ix->mu.
static int next_dispenser_block(fnv_index_s* ix, hipStream_t stream, uint32_t** block, uint32_t** other) {
  const int mine = ix->last_block == ix->d_dispenser ? 1 : 0;
  *block = ix->d_dispenser + mine * fnv_index_s::kDispenserStride;
  *other = ix->d_dispenser + (1 - mine) * fnv_index_s::kDispenserStride;
  const bool zeroed = ix->launched && ix->zeroed_block == mine && ix->last_stream == stream;
  if (!zeroed) HIP_TRY(hipMemsetAsync(*block, 0, 16 * sizeof(uint32_t), stream));
  return FNV_OK;
}

// ---- what a search launch is made of (search_device_impl and scan_device_impl, below, run the steps in order under the
// handle's mutex; every decision that is arithmetic is the planner's, launch_plan.hpp) ------------------------------------
// (a) The launch plan: depends on (beam width, K, live geometry, options) only -> cached between calls.
// The HIP runtime as the planner sees it: the kernels of one (index, beam width) by MODE_*.
// A launch reads the mirror only while it is live, covers every live row and the option is on.
static bool half_rows_usable(const fnv_index_s* ix, uint64_t live) {
  const fnv_index_s* src = rows_source(ix);
  return ix->half_rows != 0 && half_rows_possible(ix) && src->half.state.load() == HALF_LIVE && src->half.covered.load() >= live &&
         src->half.rows.load() != nullptr;
}
// THE place where a search kernel meets its table (BoundKernel): the exact and the merged-beam kernels (DIRECT forms included)
// read the mirror when `half_rows` asks for it (the row format f32h); the filtered kernel has no such instantiation and keeps
// reading the float32 table, with the same results.
enum KernelKind { KERNEL_EXACT, KERNEL_MERGED, KERNEL_MERGED_DIRECT, KERNEL_FILTERED };
static BoundKernel bind_search_kernel(const fnv_index_s* ix, const RowGeometry& g, KernelKind kind, bool lds, int B, bool half_rows) {
  auto pick = [&](const KernelTable& t) -> kernel_fn {
    switch (kind) {
      case KERNEL_EXACT: return t.exact[g.cfg][g.full];
      case KERNEL_FILTERED: return t.exact_f[g.cfg][g.full];
      default: return t.merged[beam_form(lds, B)][kind == KERNEL_MERGED_DIRECT][g.cfg][g.full];
    }
  };
  if (half_rows && kind != KERNEL_FILTERED)
    if (kernel_fn fn = pick(kernel_table(ix->dtype, ix->metric, true)))
      return BoundKernel{fn, rows_source(ix)->half.rows.load(), ix->row_bytes / 2, true};
  return BoundKernel{pick(kernel_table(ix->dtype, ix->metric)), ix->d_vectors, ix->row_bytes, false};
}
struct PlanRuntime {
  const fnv_index_s* ix;
  RowGeometry g;
  int B;
  bool half_rows;
  BoundKernel bound(int mode, bool direct = false) const {
    return bind_search_kernel(ix, g, mode == MODE_HEAPS ? KERNEL_EXACT : direct ? KERNEL_MERGED_DIRECT : KERNEL_MERGED,
                              mode == MODE_MERGED_LDS, B, half_rows);
  }
  kernel_fn kernel(int mode) const { return bound(mode).fn; }
  int occupancy(int mode, uint32_t lds) const {
    int n = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)kernel(mode), WAVE, lds) == hipSuccess ? n : 0;
  }
  const char* raise_lds_limit(int mode, uint32_t lds) const {
    const hipError_t e = ::raise_lds_limit((const void*)kernel(mode), ix->device, lds);
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
  }
};
static int ensure_plan(fnv_index_s* ix, int B, int K, bool half_rows) {
  PlannedLaunch& plan = ix->plan;
  // (a mirror that was dropped and built again is another allocation: the plan's kernels carry the table they read)
  const bool same_rows = plan.half_rows == half_rows && (!half_rows || plan.kern.rows == rows_source(ix)->half.rows.load());
  if (plan.valid && plan.B == B && plan.K == K && plan.capacity == ix->capacity && plan.options_version == ix->options_version &&
      plan.layouts_version == ix->measured.layouts_version() && same_rows)
    return FNV_OK;
  plan = PlannedLaunch();
  const PlanRuntime rt{ix, row_geometry(ix), B, half_rows};
  LayoutChoice lc;  // a layout that fnv_tune measured for this beam width overrides the planner's rules (heap home, table size)
  if (const LayoutChoice* measured = ix->measured.layout(B)) lc = *measured;
  std::string err;
  const int rc = plan_launch(ix, B, K, lc, rt, err, plan);
  if (rc) return fail(rc, err);
  for (SearchParams* p : {&plan.heaps, &plan.sorted}) {  // (`vectors` / `row_bytes`: per launch, from the kernel it runs)
    p->tails = ix->tails();
    p->links = ix->d_links;
  }
  plan.kern = rt.bound(MODE_HEAPS);
  if (plan.mode != MODE_HEAPS) {
    plan.skern = rt.bound(plan.mode);
    plan.skern_direct = rt.bound(plan.mode, true);
  }
  plan.half_rows = half_rows;
  plan.options_version = ix->options_version;
  plan.layouts_version = ix->measured.layouts_version();
  plan.valid = true;
  return FNV_OK;
}

// (b) Which kernel variant the launch runs, and whether it is a sample for the adaptive choice (KernelChoice and the rules
// of each pick: launch_plan.hpp).  Here only what needs the handle and the runtime: the measurements of an adaptive choice.
static KernelChoice choose_kernel(fnv_index_s* ix, int B, uint64_t nq, int force_variant, bool filtered) {
  KernelChoice c = default_choice(ix, ix->plan, nq, filtered, force_variant);  // (what the plan prefers, or what was pinned)
  if (!c.adaptive) return c;
  const bool multi_round = c.multi_round;
  const bool shadows_on = ix->shadow_exact != 0;
  const bool try_tail = ix->sorted_tail_exact_pct < 0;
  if (ix->is_lane) {
    // a hidden lane runs what its owner has measured (copied by sync_lane) and never explores or samples: a production
    // caller that happens to land on a lane must not pay for 3 x variants exploratory launches per lane
    if (const Tuner* t = ix->measured.find(tuner_key(B, multi_round)); nq >= 2048 && t)
      if (const int best = lane_variant(*t, multi_round, try_tail, shadows_on); best >= 0) set_variant(c, best);
    return c;
  }
  if (ix->measured.has_pending() && ix->launched && hipEventQuery(ix->ev1) == hipSuccess) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ix->ev0, ix->ev1) != hipSuccess) ms = 0.f;
    ix->measured.harvest(ms);  // (a change: lanes re-copy the measurements)
  }
  if (nq >= 2048) {
    const Tuner* found = ix->measured.find(tuner_key(B, multi_round));
    const Tuner t = found ? *found : Tuner();  // (nothing measured yet: every variant is still to be sampled)
    // three samples each (the first launch of a kernel is a cold one; the best of the rest decides), then the fastest
    // (fnv_tune takes all the samples in one call, so that no caller's launch is an exploratory one)
    int v = owner_next_sample(t, multi_round, try_tail, shadows_on);
    c.exploratory = v >= 0;
    if (v < 0) v = owner_final_variant(t, multi_round, try_tail, shadows_on);
    c.sample = t.samples[v] < 4;
    set_variant(c, v);
  }
  return c;
}

// (c) The workspace, grown on demand and sized for whichever kernel keeps more slots resident.
static int grow_workspace(fnv_index_s* ix, uint32_t max_slots, uint64_t nq, bool sorted, bool done_flags, bool filtered) {
  const SlotWorkspace per_slot = slot_workspace(ix, sorted ? ix->plan.sorted.log_entries : 0);
  int rc = FNV_OK;
  for (int attempt = 0; attempt < 2; attempt++) {
    rc = ix->ws.bitmap.grow((size_t)max_slots * per_slot.bitmap, true);
    if (!rc) rc = ix->ws.ovf.grow((size_t)max_slots * per_slot.ovf);
    if (!rc) rc = ix->ws.spill.grow((size_t)max_slots * per_slot.spill);
    if (!rc && done_flags) rc = ix->d_done.grow((size_t)nq * 4);
    if (!rc && sorted) rc = ix->ws.tielog.grow((size_t)max_slots * per_slot.tielog);
    if (!rc && filtered) rc = ix->d_nodebits.grow((size_t)node_words(ix) * 4);
    ix->ws_bytes = ix->ws.bytes();
    // out of memory on the handle itself: the hidden lanes' idle workspaces go first, then once more (the lock order: fnv_index_s)
    if (rc != FNV_ERR_NO_DEVICE || attempt || ix->is_lane || ix->parent) break;
    (void)hipGetLastError();
    if (release_idle_lanes(ix, nullptr) == 0) break;
  }
  return rc;
}

// ---- grouped filters: the node bitmaps of a launch with one filter per query ---------------------------------------
// ws.rows for the n_filters + 2 rows of a grouped launch (filter_rows_bytes, launch_plan.hpp).  The one allocation of the
// library whose size the caller's n_filters decides: its failure says how much that was, and a host-buffer caller's lane is
// admitted with it counted.
static int grow_filter_rows(fnv_index_s* ix, const SearchFilter& f) {
  const size_t need = filter_rows_bytes(ix, f.rows());
  const int rc = ix->ws.rows.grow(need);
  ix->ws_bytes = ix->ws.bytes();
  if (rc == FNV_OK) return FNV_OK;
  (void)hipGetLastError();
  return fail(FNV_ERR_RUNTIME, "the filter rows of this launch need " + std::to_string(need) + " bytes of device memory (" +
                                   std::to_string(f.rows()) + " node bitmaps), which could not be allocated");
}
// ... filled from the filter table and the labels as they are now.  `ga` (null: not wanted): the launch's grouping arrays in
// ws.group -- their cleared prefix is zeroed here, and row_count takes the nodes set per row.
static int launch_filter_rows(fnv_index_s* ix, const SearchFilter& f, uint64_t live, hipStream_t stream, const GroupArrays* ga) {
  const uint64_t words = node_words(ix);
  uint32_t* const w = ix->ws.group.as<uint32_t>();
  if (ga) HIP_TRY(hipMemsetAsync(w + ga->counts, 0, ga->cleared_bytes, stream));
  uint32_t* const row_count = ga ? w + ga->row_count : nullptr;
  const dim3 grid((unsigned)((words * 32 + 255) / 256), (unsigned)std::min<uint64_t>(f.rows(), 65535));
  hipLaunchKernelGGL(node_filter_table_kernel, grid, dim3(256), 0, stream, (const int32_t*)ix->d_labels, live, words, f.bits, f.stride,
                     f.n_bits, (uint32_t)f.n_filters, ix->ws.rows.as<uint32_t>(), row_count);
  HIP_TRY(hipGetLastError());
  return FNV_OK;
}
// One filter for the launch: the label bitmap -> d_nodebits, by the labels as they are now (after reorder(), device builds ...)
static int launch_node_filter(fnv_index_s* ix, const SearchFilter& f, uint64_t live, hipStream_t stream) {
  const uint64_t words = node_words(ix);
  hipLaunchKernelGGL(node_filter_kernel, dim3((unsigned)((words * 32 + 255) / 256)), dim3(256), 0, stream, (const int32_t*)ix->d_labels,
                     live, words, f.bits, f.n_bits, ix->d_nodebits.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  return FNV_OK;
}
// What every launch checks after its own arguments; false: the call is over with *rc (an empty batch is FNV_OK).
static bool batch_to_launch(const void* d_queries, uint64_t nq, const SearchOutputs& out, int* rc) {
  *rc = FNV_OK;
  if (nq == 0) return false;
  if (!d_queries || !out.dist || !out.labels) *rc = fail(FNV_ERR_INVALID, "null buffer");
  else if (nq > 0x7FFFFFFFull) *rc = fail(FNV_ERR_INVALID, "too many queries in one batch");
  return *rc == FNV_OK;
}
// What the launch was, for the fnv_last_* calls: grid, block, LDS bytes, then five values of the kernel's own (geom[6]: its mode).
// `dispenser`: the block the launch owns; `zeroed`: the block its kernel zeroes for the next launch (-1: none); `timed`: ev0 / ev1
// bracket it.
static void record_launch(fnv_index_s* ix, hipStream_t stream, uint32_t* dispenser, int zeroed, bool timed, uint64_t grid, uint64_t block,
                          uint64_t lds, uint64_t g3, uint64_t g4, uint64_t g5, uint64_t mode, uint64_t g7) {
  ix->last_stream = stream;
  ix->last_block = dispenser;
  ix->zeroed_block = zeroed;
  ix->last_timed = timed;
  ix->launched = true;
  if (!ix->is_lane) ix->last_served = nullptr;  // the handle's own launch is its most recent one
  const uint64_t geom[8] = {grid, block, lds, g3, g4, g5, mode, g7};
  for (int i = 0; i < 8; i++) ix->geom[i] = geom[i];
}
// ---- exhaustive search (scan.hpp): the launch ---------------------------------------------------------------------
// (how a launch is cut up, its grouping arrays and byte counts: scan_shape, GroupArrays and their neighbours in launch_plan.hpp)

// Filter routing of a filtered graph search (plan_scan_routing, launch_plan.hpp): whether this launch routes, the shape of the
// scan stage, and its filter as a TABLE -- the grouped call's own, or, the single-filter call, a table of that one filter with a
// null query_filter (every query reads row 0).
struct RoutedLaunch : ScanRouting {
  SearchFilter table{nullptr, 0};
};
static RoutedLaunch plan_routing(const fnv_index_s* ix, const SearchFilter* filter, const RowGeometry& g, uint64_t nq, int K, uint64_t live) {
  RoutedLaunch r;
  if (!filter || !filter_routing_on(ix)) return r;  // (as the planner will say: nothing to rewrite for it)
  r.table = *filter;
  if (!filter->grouped) {
    r.table.grouped = true;
    r.table.n_filters = 1;
    r.table.stride = (filter->n_bits + 7) / 8;
    r.table.query_filter = nullptr;
  }
  static_cast<ScanRouting&>(r) = plan_scan_routing(ix, g, nq, K, live, r.table.rows());
  return r;
}
// HBM a routed launch of `nq` queries takes on top of the search kernel's per-slot workspace (0: the launch does not route).
// What a host-buffer caller's lane is admitted with.
size_t routed_workspace_bytes(fnv_index_s* ix, const SearchFilter& f, uint64_t nq, int K) {
  std::lock_guard<std::mutex> lock(ix->mu);
  const uint64_t live = live_nodes(ix);
  if (nq == 0 || nq > 0x7FFFFFFFull || K < 1) return 0;
  const RoutedLaunch r = plan_routing(ix, &f, row_geometry(ix), nq, K, live);
  return r.on ? routed_scan_bytes(ix, r.table.rows(), nq, K, r.shape) : 0;
}

// What the scan kernels are told about the index and the call (cand_ids / cand_count, the single-filter scan's own, stay null).
static ScanParams scan_params(const fnv_index_s* ix, const RowGeometry& g, const void* d_queries, uint64_t nq, int K,
                              const SearchOutputs& out, const SearchOptions& opt, const ScanShape& shape, uint64_t live) {
  ScanParams p;
  memset(&p, 0, sizeof(p));
  p.vectors = ix->d_vectors;
  p.tails = ix->tails();
  p.labels = (opt.node_ids || ix->output_node_ids != 0) ? nullptr : ix->d_labels;
  p.queries = (const uint8_t*)d_queries;
  p.partial = ix->ws.scan.as<uint64_t>();
  p.out_dist = out.dist;
  p.out_labels = out.labels;
  p.out_count = out.count;
  p.out_ndist = out.ndist;
  p.n_live = live;
  p.nq = (uint32_t)nq;
  p.dim = ix->dim;
  p.row_bytes = ix->row_bytes;
  p.nchunks = g.nchunks;
  p.q_chunks = g.q_chunks;
  p.tail_chunks = g.tail_chunks;
  p.K = (uint32_t)K;
  p.segments = shape.segments;
  p.tile_queries = shape.tile;
  p.tiles = shape.tiles;
  return p;
}
// The queries of a grouped scan grouped by filter row into tiles (scan.hpp's group_* kernels; counts and cursor are zero, the
// filter rows and row_count under way on `stream`), and what the scan and its merge are told about it.  `route` (null: every
// query): the route words of a routed filtered graph search, whose scan stage takes only the queries whose word is set.
static int launch_grouping(fnv_index_s* ix, const SearchFilter& f, const GroupArrays& ga, const ScanShape& shape, uint64_t nq, uint64_t live,
                           hipStream_t stream, const uint32_t* route, GroupedScanParams* gp) {
  uint32_t* const w = ix->ws.group.as<uint32_t>();
  const uint32_t rows = (uint32_t)f.rows(), n = (uint32_t)nq;
  if (route)
    hipLaunchKernelGGL(group_rows_routed_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, f.query_filter, route, n,
                       (uint32_t)f.n_filters, w + ga.query_row, w + ga.counts);
  else
    hipLaunchKernelGGL(group_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, f.query_filter, n, (uint32_t)f.n_filters,
                       w + ga.query_row, w + ga.counts);
  hipLaunchKernelGGL(group_prefix_kernel, dim3(1), dim3(256), 0, stream, (const uint32_t*)(w + ga.counts), rows, shape.tile,
                     w + ga.slot_start, w + ga.tile_start);
  hipLaunchKernelGGL(group_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t*)(w + ga.query_row), n,
                     (const uint32_t*)(w + ga.slot_start), w + ga.cursor, w + ga.perm);
  hipLaunchKernelGGL(group_tiles_kernel, dim3((shape.tiles + 255) / 256), dim3(256), 0, stream, (const uint32_t*)(w + ga.slot_start),
                     (const uint32_t*)(w + ga.tile_start), rows, shape.tile, shape.tiles, (GroupTile*)(w + ga.tiles));
  HIP_TRY(hipGetLastError());
  gp->node_bits = ix->ws.rows.as<uint32_t>();
  gp->tiles = (const GroupTile*)(w + ga.tiles);
  gp->perm = w + ga.perm;
  gp->query_row = w + ga.query_row;
  gp->row_count = w + ga.row_count;
  gp->row_words = (uint32_t)node_words(ix);
  gp->live_words = (uint32_t)((live + 31) / 32);
  return FNV_OK;
}
// The grouped scan and its merge.  `route` as above: the merge then answers the routed queries only and zeroes their out_nhops.
static int launch_grouped_scan(fnv_index_s* ix, scan_grouped_fn kern_g, const GroupedScanParams& gp, const ScanShape& shape, uint64_t nq,
                               hipStream_t stream, const uint32_t* route = nullptr, uint64_t* out_nhops = nullptr) {
  const uint32_t merge_lds = scan_merge_lds(gp.s.K);
  HIP_TRY(raise_lds_limit((const void*)kern_g, ix->device, shape.lds));
  hipLaunchKernelGGL(kern_g, dim3(shape.tiles * shape.segments), dim3(WAVE), shape.lds, stream, gp);
  HIP_TRY(hipGetLastError());
  if (route) hipLaunchKernelGGL(exhaustive_merge_routed_kernel, dim3((unsigned)nq), dim3(WAVE), merge_lds, stream, gp, route, out_nhops);
  else hipLaunchKernelGGL(exhaustive_merge_grouped_kernel, dim3((unsigned)nq), dim3(WAVE), merge_lds, stream, gp);
  HIP_TRY(hipGetLastError());
  return FNV_OK;
}

// The single-filter scan's candidates: the label bitmap -> this handle's node bitmap -> the list of allowed node ids.
static int launch_candidate_list(fnv_index_s* ix, const SearchFilter& f, uint64_t live, hipStream_t stream, ScanParams* p) {
  uint32_t* const ids = ix->d_scanids.as<uint32_t>();
  const int rc = launch_node_filter(ix, f, live, stream);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(ids, 0, 16, stream));
  hipLaunchKernelGGL(exhaustive_compact_kernel, dim3((unsigned)((live + 255) / 256)), dim3(256), 0, stream,
                     (const uint32_t*)ix->d_nodebits.as<uint32_t>(), live, ids + 4, ids);
  HIP_TRY(hipGetLastError());
  p->cand_ids = ids + 4;
  p->cand_count = ids;
  return FNV_OK;
}

// One exhaustive search: shape (planner), workspace, filter bitmaps, the scan and its merge, record.
static int scan_device_impl(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, const SearchOutputs& out, void* hip_stream,
                            const SearchOptions& opt) {
  int rc;
  if (K < 1 || K > SCAN_MAX_K) return fail(FNV_ERR_INVALID, "K of an exhaustive search must be between 1 and 1024");
  if (!batch_to_launch(d_queries, nq, out, &rc)) return rc;
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  hipStream_t stream = (hipStream_t)hip_stream;
  const SearchFilter* filter = opt.filter;
  const uint64_t live = live_nodes(ix);
  const RowGeometry g = row_geometry(ix);
  const bool grouped = filter && filter->grouped, listed = filter && !grouped;

  // -- shape
  const ScanShape shape = scan_shape(ix, g, nq, K, live, grouped ? filter->rows() : 0);
  if (shape.lds > kScanMaxLds) return fail(FNV_ERR_INVALID, "rows are too long for an exhaustive search (one query and its list must fit in LDS)");
  const GroupArrays ga(nq, grouped ? filter->rows() : 0, shape.tiles);

  // -- workspace
  rc = ix->ws.scan.grow(scan_partial_bytes(nq, shape, K));
  if (!rc && grouped) rc = grow_filter_rows(ix, *filter);
  if (!rc && grouped) rc = ix->ws.group.grow(ga.bytes);
  if (!rc && listed) rc = ix->d_nodebits.grow((size_t)node_words(ix) * 4);
  if (!rc && listed) rc = ix->d_scanids.grow(16 + (size_t)ix->capacity * 4);
  ix->ws_bytes = ix->ws.bytes();
  if (rc) return rc;

  // -- filter bitmaps (grouped: with their popcounts, and the queries grouped by row into tiles)
  GroupedScanParams gp;
  memset(&gp, 0, sizeof(gp));
  gp.s = scan_params(ix, g, d_queries, nq, K, out, opt, shape, live);
  // (the status word: this path never sets it; the scan's kernels zero no block, so the next search launch memsets its own)
  uint32_t* const block = ix->last_block;
  HIP_TRY(hipMemsetAsync(block, 0, 16 * sizeof(uint32_t), stream));
  if (grouped) rc = launch_filter_rows(ix, *filter, live, stream, &ga);
  if (!rc && grouped) rc = launch_grouping(ix, *filter, ga, shape, nq, live, stream, nullptr, &gp);
  if (listed) rc = launch_candidate_list(ix, *filter, live, stream, &gp.s);
  if (rc) return rc;

  // -- the scan and its merge
  ix->measured.drop_pending();  // ev0 / ev1 no longer bracket a graph-search launch
  HIP_TRY(hipEventRecord(ix->ev0, stream));
  if (grouped) {
    rc = launch_grouped_scan(ix, kernel_table(ix->dtype, ix->metric).flat_g[g.cfg][g.full], gp, shape, nq, stream);
    if (rc) return rc;
  } else {
    const scan_fn kern = kernel_table(ix->dtype, ix->metric).flat[g.cfg][g.full];
    HIP_TRY(raise_lds_limit((const void*)kern, ix->device, shape.lds));
    hipLaunchKernelGGL(kern, dim3(shape.tiles * shape.segments), dim3(WAVE), shape.lds, stream, gp.s);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(exhaustive_merge_kernel, dim3((unsigned)nq), dim3(WAVE), scan_merge_lds((uint32_t)K), stream, gp.s);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ix->ev1, stream));

  // -- record (mode 3 of fnv_last_launch_geometry: the exhaustive scan; its grouped form: queries per tile, entries of the id
  // queue, row segments)
  record_launch(ix, stream, block, -1, true, (uint64_t)shape.tiles * shape.segments, WAVE, shape.lds, grouped ? shape.tile : 0,
                grouped ? SCAN_QUEUE_IDS : 0, grouped ? shape.segments : 0, 3, 0);
  return FNV_OK;
}

// ---- one graph search: plan, shape (planner), workspace, filter bitmaps, K0, the launch, scan stage, record ---------------
// Plan: the mirror's state, the cached plan, and -- a filtered launch's first -- the filtered kernel with its residency.
static int plan_search(fnv_index_s* ix, int B, int K, uint64_t live, bool filtered) {
  // The half-width mirror (half_rows.hpp): its state is the source's, read at every launch.  Launches with and without it run
  // different kernels, so what was measured in the other mode (kernel variant, LDS layout) is discarded with the plan.
  const bool half_rows = half_rows_usable(ix, live);
  (void)ix->measured.rows_changed(half_rows);  // (the layouts' version then makes ensure_plan plan again)
  const int rc = ensure_plan(ix, B, K, half_rows);
  if (rc) return rc;
  PlannedLaunch& plan = ix->plan;
  if (filtered && !plan.fkern.fn) {
    plan.fkern = bind_search_kernel(ix, row_geometry(ix), KERNEL_FILTERED, false, B, half_rows);
    HIP_TRY(raise_lds_limit((const void*)plan.fkern.fn, ix->device, plan.lds));
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)plan.fkern.fn, WAVE, plan.lds) != hipSuccess) n = 0;
    plan.fbpc = std::max(1, std::min(plan.bpc, n));
  }
  return FNV_OK;
}
// The per-call fields of the parameter block (the plan left them unset), the dispenser block's among them.
static void fill_call_fields(fnv_index_s* ix, SearchParams& p, const void* d_queries, uint64_t nq, const SearchOutputs& out,
                             const SearchOptions& opt, const SearchLaunch& L, bool sorted, uint64_t live, uint32_t* block, uint32_t* other) {
  p.labels = (opt.node_ids || ix->output_node_ids != 0) ? nullptr : ix->d_labels;  // ("output_node_ids": read under the handle's mutex)
  p.queries = (const uint8_t*)d_queries;
  p.out_dist = out.dist;
  p.out_labels = out.labels;
  p.out_count = out.count;
  p.out_ndist = out.ndist;
  p.out_nhops = out.nhops;
  p.n_nodes = live;
  p.nq = (uint32_t)nq;
  p.scan_step = L.scan_step;  // Index.h:851-861
  p.n_scan = L.n_scan;
  p.ovf_bitmap = ix->ws.bitmap.as<uint32_t>();
  p.ovf_glist = ix->ws.ovf.as<uint32_t>();
  p.cand_spill = ix->ws.spill.as<unsigned long long>();
  p.tie_log = ix->ws.tielog.as<unsigned long long>();
  if (!sorted) p.log_entries = 0u;
  p.dispenser = block;
  p.dispenser_next = other;
  p.status = (int32_t*)(block + 1);
  p.host_status = opt.host_status;
  p.redo_count = block + 3;  // [3] queries searched exactly after a tie, [4..7] by reason
  p.phase_cycles = ix->d_phase;
  p.tail_exact = L.tail_exact;
}
// Filter bitmaps: the filter table -> this handle's node bitmaps, every query reading its own row (routed: the rows' popcounts
// -> who goes to the scan, before the search kernel has seen it); or the one filter -> d_nodebits.
static int launch_search_filter(fnv_index_s* ix, const SearchFilter* filter, const SearchFilter* rows_of, const RoutedLaunch& routing,
                                const GroupArrays& ga, uint64_t nq, uint64_t live, hipStream_t stream, SearchParams& p) {
  if (!rows_of) {
    if (filter) p.node_bits = ix->d_nodebits.as<uint32_t>();
    return filter ? launch_node_filter(ix, *filter, live, stream) : FNV_OK;
  }
  const int rc = launch_filter_rows(ix, *rows_of, live, stream, routing.on ? &ga : nullptr);
  if (rc) return rc;
  p.node_bits = ix->ws.rows.as<uint32_t>();
  p.query_filter = rows_of->query_filter;
  p.filter_words = (uint32_t)node_words(ix);
  p.n_filters = (uint32_t)rows_of->n_filters;
  if (routing.on) {
    uint32_t* const gw = ix->ws.group.as<uint32_t>();
    hipLaunchKernelGGL(route_queries_kernel, dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, stream, routing.table.query_filter,
                       (uint32_t)nq, (uint32_t)routing.table.n_filters, (const uint32_t*)(gw + ga.row_count), (uint64_t)ix->filter_scan_max,
                       (uint32_t)(ix->filter_scan_on_overflow != 0), gw + ga.route);
    HIP_TRY(hipGetLastError());
    p.query_route = gw + ga.route;
  }
  return FNV_OK;
}
// K0: one pass over the shared entry-scan nodes for the whole batch (LDS-staged, entry_scan_tile), same stream.
static int launch_entry_scan(fnv_index_s* ix, SearchParams& p, uint64_t nq, hipStream_t stream) {
  const int rc = ix->d_entry.grow((size_t)nq * 8);
  if (rc) return rc;
  p.entry_node_out = ix->d_entry.as<uint32_t>();
  p.entry_dist_out = (float*)(ix->d_entry.as<uint8_t>() + (size_t)nq * 4);
  p.vectors = ix->d_vectors;  // (K0 stages float32 rows in LDS whichever table the search kernel reads)
  p.row_bytes = ix->row_bytes;
  const EntryScanTile tile = entry_scan_tile(p.row_bytes, p.q_chunks, p.n_scan, nq);
  p.scan_tile_stride = tile.stride;
  p.scan_tile_rows = tile.rows;
  kernel_fn scan = pick_scan_kernel(ix->dtype, ix->metric, ix->plan.cfg, ix->plan.full);
  HIP_TRY(raise_lds_limit((const void*)scan, ix->device, tile.lds));
  hipLaunchKernelGGL(scan, dim3(tile.grid), dim3(SCAN_WAVES * WAVE), tile.lds, stream, p);
  HIP_TRY(hipGetLastError());
  p.entry_node = p.entry_node_out;
  p.entry_dist = p.entry_dist_out;
  return FNV_OK;
}
// Scan stage of a routed launch, on the same stream: the queries whose route word is set, grouped by filter row into tiles.
static int launch_scan_stage(fnv_index_s* ix, const RoutedLaunch& routing, const GroupArrays& ga, const RowGeometry& g, const void* d_queries,
                             uint64_t nq, int K, const SearchOutputs& out, const SearchOptions& opt, uint64_t live, hipStream_t stream) {
  uint32_t* const route = ix->ws.group.as<uint32_t>() + ga.route;
  GroupedScanParams gp;
  memset(&gp, 0, sizeof(gp));
  const int rc = launch_grouping(ix, routing.table, ga, routing.shape, nq, live, stream, route, &gp);
  if (rc) return rc;
  gp.s = scan_params(ix, g, d_queries, nq, K, out, opt, routing.shape, live);
  return launch_grouped_scan(ix, kernel_table(ix->dtype, ix->metric).flat_g[g.cfg][g.full], gp, routing.shape, nq, stream, route, out.nhops);
}

int search_device_impl(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search, int num_initializations,
                              const SearchOutputs& out, void* hip_stream, const SearchOptions& opt) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (opt.exhaustive) return scan_device_impl(ix, d_queries, nq, K, out, hip_stream, opt);
  int rc = check_search_sizes(K, ef_search, num_initializations);
  if (rc) return rc;
  if (!batch_to_launch(d_queries, nq, out, &rc)) return rc;
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  hipStream_t stream = (hipStream_t)hip_stream;
  const SearchFilter* filter = opt.filter;
  const int B = std::max(ef_search, K);  // Index.h:392
  const uint64_t live = live_nodes(ix);

  // -- plan
  rc = plan_search(ix, B, K, live, filter != nullptr);
  if (rc) return rc;
  const PlannedLaunch& plan = ix->plan;

  // -- shape: the kernel variant, then everything shape_search (launch_plan.hpp) derives from it -- shadow mode, tail shadows,
  // the grid, the DIRECT form, the parameter block `p`; and whether the launch routes (a scan stage follows the search kernel)
  const KernelChoice c = choose_kernel(ix, B, nq, opt.force_variant, filter != nullptr);
  const bool sorted = c.sorted;
  SearchParams p;
  const SearchLaunch L = shape_search(ix, plan, c, filter ? plan.fbpc : 0, nq, num_initializations, live, p);
  const RowGeometry sg = row_geometry(ix);
  const RoutedLaunch routing = plan_routing(ix, filter, sg, nq, K, live);
  const SearchFilter* const rows_of = routing.on ? &routing.table : filter && filter->grouped ? filter : nullptr;  // a table of node bitmaps
  const GroupArrays ga(nq, routing.on ? routing.table.rows() : 0, routing.shape.tiles, true);

  // -- workspace (per slot; the node bitmaps; routed: the scan stage's lists and arrays), then the per-call fields
  rc = grow_workspace(ix, L.max_slots, nq, sorted, L.shadow || L.tail_shadows, filter != nullptr && !rows_of);
  if (!rc && rows_of) rc = grow_filter_rows(ix, *rows_of);
  if (!rc && routing.on) rc = ix->ws.scan.grow(scan_partial_bytes(nq, routing.shape, K));
  if (!rc && routing.on) rc = ix->ws.group.grow(ga.bytes);
  ix->ws_bytes = ix->ws.bytes();
  if (rc) return rc;
  const BoundKernel& kern = filter ? plan.fkern : !sorted ? plan.kern : L.direct ? plan.skern_direct : plan.skern;
  uint32_t *block = nullptr, *other = nullptr;
  rc = next_dispenser_block(ix, stream, &block, &other);
  if (rc) return rc;
  fill_call_fields(ix, p, d_queries, nq, out, opt, L, sorted, live, block, other);
  // ev0 / ev1 only where somebody will read them (runtime.hpp, time_launches)
  const bool timed = c.sample || opt.timed || opt.force_variant >= 0 || ix->time_launches.load();

  // -- filter bitmaps
  rc = launch_search_filter(ix, filter, rows_of, routing, ga, nq, live, stream, p);
  if (rc) return rc;
  if (timed) HIP_TRY(hipEventRecord(ix->ev0, stream));

  // -- K0 (split rows: its LDS tiles hold one table's rows; the in-kernel scan serves them)
  if (ix->entry_kernel && !ix->tail_bytes) rc = launch_entry_scan(ix, p, nq, stream);
  if (rc) return rc;
  // -- shadows: from here on the launch has more work items than queries -- the queries, then exact shadows of all of them
  // (shadow mode) or of the last `tail_shadows` (pulled by slots that would go idle); the two never meet in one launch
  if (L.shadow || L.tail_shadows) {
    HIP_TRY(hipMemsetAsync(ix->d_done.ptr, 0, (size_t)nq * 4, stream));
    p.shadow_base = (uint32_t)nq;
    p.done_flags = ix->d_done.as<uint32_t>();
    p.nq = (uint32_t)(nq + (L.shadow ? nq : L.tail_shadows));
    p.tail_exact = 0u;
  }

  // -- the launch
  p.vectors = kern.rows;  // the kernel and the table it reads: one BoundKernel
  p.row_bytes = kern.stride;
  HIP_TRY(raise_lds_limit((const void*)kern.fn, ix->device, L.lds));
  hipLaunchKernelGGL(kern.fn, dim3(L.nslots), dim3(WAVE), L.lds, stream, p);
  HIP_TRY(hipGetLastError());
  // the blocks change hands HERE: whatever fails below, the next launch must not take this one's block for a zeroed one
  ix->last_stream = stream;
  ix->last_block = block;
  ix->zeroed_block = (int)(other != ix->d_dispenser);

  // -- scan stage
  if (routing.on) rc = launch_scan_stage(ix, routing, ga, sg, d_queries, nq, K, out, opt, live, stream);
  if (rc) return rc;
  if (timed) HIP_TRY(hipEventRecord(ix->ev1, stream));

  // -- record: for the adaptive choice's next harvest, and for the fnv_last_* calls
  if (c.sample) ix->measured.expect(tuner_key(B, c.multi_round), c.variant, nq);  // (a sample is always timed)
  else ix->measured.drop_pending();
  ix->last_variant = sorted ? std::max(c.variant, 1) : 0;
  ix->last_exploratory = c.exploratory;
  if (c.exploratory) ix->explored_launches++;
  ix->last_shadow = L.shadow;
  ix->last_half = kern.half_rows;
  record_launch(ix, stream, block, (int)(other != ix->d_dispenser), timed, L.nslots, WAVE, L.lds, (uint64_t)L.bpc, p.vis_slots, p.cand_slots,
                (uint64_t)L.mode, p.tail_exact);
  return FNV_OK;
}

// ---- filtered search: results restricted to the nodes whose label is set in a bitmap over label values -------------
int check_filter_args(const void* allowed_bits, uint64_t n_bits) {
  if (n_bits > (1ull << 31)) return fail(FNV_ERR_INVALID, "n_bits must be at most 2^31 (labels are int32)");
  if (n_bits > 0 && !allowed_bits) return fail(FNV_ERR_INVALID, "allowed_bits is null but n_bits > 0");
  return FNV_OK;
}

// ---- exhaustive search: the exact K nearest among the live nodes, or among those whose label is allowed (scan.hpp) -----
int check_exhaustive_args(fnv_index_t ix, int K, int use_filter, const void* allowed_bits, uint64_t n_bits) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (K < 1 || K > SCAN_MAX_K) return fail(FNV_ERR_INVALID, "K of an exhaustive search must be between 1 and 1024");
  return use_filter ? check_filter_args(allowed_bits, n_bits) : FNV_OK;
}

// ---- grouped filters: a table of allowed sets and, per query, which of them it uses ----------------------------------
int check_grouped_args(const void* filters, uint64_t n_filters, uint64_t stride, uint64_t n_bits, const int32_t* query_filter,
                              uint64_t nq, SearchFilter* out) {
  if (n_bits > (1ull << 31)) return fail(FNV_ERR_INVALID, "n_bits must be at most 2^31 (labels are int32)");
  if (n_filters > 0x7FFFFFFFull) return fail(FNV_ERR_INVALID, "n_filters must be at most 2^31 - 1 (query_filter is int32)");
  if (n_filters > 0 && stride < (n_bits + 7) / 8) return fail(FNV_ERR_INVALID, "filter_stride_bytes is smaller than ceil(n_bits / 8)");
  if (n_filters > 0 && n_bits > 0 && !filters) return fail(FNV_ERR_INVALID, "filters is null but n_filters > 0 and n_bits > 0");
  if (nq > 0 && !query_filter) return fail(FNV_ERR_INVALID, "query_filter is null");
  *out = SearchFilter{n_filters && n_bits ? (const uint8_t*)filters : nullptr, n_bits};
  out->grouped = true;
  out->n_filters = n_filters;
  out->stride = stride;
  out->query_filter = query_filter;
  return FNV_OK;
}

// Only the C ABI is exported (the library is built with -fvisibility=hidden).
#pragma GCC visibility push(default)
extern "C" {

int fnv_search_batch_device(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search,
                            int num_initializations, float* d_out_dist, int32_t* d_out_labels,
                            int32_t* d_out_count, uint64_t* d_out_ndist, uint64_t* d_out_nhops, void* hip_stream) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  return search_device_impl(ix, d_queries, nq, K, ef_search, num_initializations,
                            SearchOutputs{d_out_dist, d_out_labels, d_out_count, d_out_ndist, d_out_nhops}, hip_stream);
}

int fnv_search_status(fnv_index_t ix) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (!ix->launched) return FNV_OK;
  ON_DEVICE(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->last_stream));
  return check_device_status(ix);
}

int fnv_search_batch_filtered_device(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search,
                                     int num_initializations, const void* d_allowed_bits, uint64_t n_bits, float* d_out_dist,
                                     int32_t* d_out_labels, int32_t* d_out_count, uint64_t* d_out_ndist, uint64_t* d_out_nhops,
                                     void* hip_stream) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  int rc = check_filter_args(d_allowed_bits, n_bits);
  if (rc) return rc;
  const SearchFilter f{n_bits ? (const uint8_t*)d_allowed_bits : nullptr, n_bits};
  SearchOptions opt;
  opt.filter = &f;
  return search_device_impl(ix, d_queries, nq, K, ef_search, num_initializations,
                            SearchOutputs{d_out_dist, d_out_labels, d_out_count, d_out_ndist, d_out_nhops}, hip_stream, opt);
}

int fnv_search_batch_exhaustive_device(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int use_filter,
                                       const void* d_allowed_bits, uint64_t n_bits, float* d_out_dist, int32_t* d_out_labels,
                                       int32_t* d_out_count, uint64_t* d_out_ndist, void* hip_stream) {
  int rc = check_exhaustive_args(ix, K, use_filter, d_allowed_bits, n_bits);
  if (rc) return rc;
  const SearchFilter f{n_bits ? (const uint8_t*)d_allowed_bits : nullptr, n_bits};
  SearchOptions opt;
  opt.filter = use_filter ? &f : nullptr;
  opt.exhaustive = true;
  return search_device_impl(ix, d_queries, nq, K, 1, 1, SearchOutputs{d_out_dist, d_out_labels, d_out_count, d_out_ndist, nullptr},
                            hip_stream, opt);
}

int fnv_search_batch_filtered_grouped_device(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search,
                                             int num_initializations, const void* d_filters, uint64_t n_filters,
                                             uint64_t filter_stride_bytes, uint64_t n_bits, const int32_t* d_query_filter,
                                             float* d_out_dist, int32_t* d_out_labels, int32_t* d_out_count, uint64_t* d_out_ndist,
                                             uint64_t* d_out_nhops, void* hip_stream) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  SearchFilter f{nullptr, 0};
  int rc = check_grouped_args(d_filters, n_filters, filter_stride_bytes, n_bits, d_query_filter, nq, &f);
  if (rc) return rc;
  SearchOptions opt;
  opt.filter = &f;
  return search_device_impl(ix, d_queries, nq, K, ef_search, num_initializations,
                            SearchOutputs{d_out_dist, d_out_labels, d_out_count, d_out_ndist, d_out_nhops}, hip_stream, opt);
}

int fnv_search_batch_exhaustive_grouped_device(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, const void* d_filters,
                                               uint64_t n_filters, uint64_t filter_stride_bytes, uint64_t n_bits,
                                               const int32_t* d_query_filter, float* d_out_dist, int32_t* d_out_labels,
                                               int32_t* d_out_count, uint64_t* d_out_ndist, void* hip_stream) {
  SearchFilter f{nullptr, 0};
  int rc = check_exhaustive_args(ix, K, 0, nullptr, 0);
  if (!rc) rc = check_grouped_args(d_filters, n_filters, filter_stride_bytes, n_bits, d_query_filter, nq, &f);
  if (rc) return rc;
  SearchOptions opt;
  opt.filter = &f;
  opt.exhaustive = true;
  return search_device_impl(ix, d_queries, nq, K, 1, 1, SearchOutputs{d_out_dist, d_out_labels, d_out_count, d_out_ndist, nullptr},
                            hip_stream, opt);
}

}  // extern "C"
#pragma GCC visibility pop
