// beam_search.hip -- MI355X (gfx950 / CDNA4) implementation of flatnav's batched k-NN search
// and the C ABI declared in include/flatnav_hip.h.
//
// Reference path being replaced (paths relative to the reference repo):
//   Index::search              include/flatnav/index/Index.h:387-409
//   Index::initializeSearch    include/flatnav/index/Index.h:845-870
//   Index::beamSearch          include/flatnav/index/Index.h:606-659
//   Index::processCandidateNode include/flatnav/index/Index.h:661-707
//   distance dispatch          include/flatnav/distances/{L2,IP}DistanceDispatcher.h
//   VisitedSet                 include/flatnav/util/VisitedSetPool.h:16-50
//   batched loop               python-bindings/src/flatnav/bindings.cpp:161-228
//
// Execution model: one 64-lane wavefront = one query at a time; a
// persistent grid of query slots (as many as LDS lets stay resident) pulls query ids
// from an atomic dispenser.  Per query, in LDS: the query vector, the two binary
// heaps of the reference (moved with libstdc++'s exact algorithm, flatnav/util/StlExact.h,
// cooperatively by the 64 lanes), an exact 16-bit-tag visited set, and a 64-entry id staging area.  Per hop the wave
// loads one link row (M ids, coalesced), tests/marks all of them in the visited set
// in parallel, gathers the unvisited neighbours' vectors with 16-byte loads (G lanes
// per vector so each lane group reads whole 128-byte lines, PU*CU loads in flight per
// lane), reduces the distances across lanes with DPP, then replays the reference's
// sequential admission rule on the results.
//
// The launch planner -- row layout, visited-table geometry, a slot's LDS layout, table-size ladder, kernel family and variant,
// launch shape: every decision that is arithmetic -- lives in launch_plan.hpp, free of HIP (tests/test_launch_plan.py runs
// it on the CPU); this file owns the HIP runtime around it: handles, buffers, streams and events, kernel lookup, the
// occupancy queries and LDS limits the planner asks for, the launches and the C ABI.
//
// Also here: incremental construction (fnv_index_write_nodes / write_links / insert_batch: Index::add,
// include/flatnav/index/Index.h:353-378 with selectNeighbors :714-763 and connectNeighbors :765-834 as the
// wire_select / wire_connect kernels of wire.hpp); the merged-beam search kernel is merged_beam.hpp.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/flatnav_hip.h"
#include "kernel_table.h"
#include "launch_plan.hpp"
#ifdef FNV_DEV_FAST_BUILD
#include "kernels.hpp"
#include "merged_beam.hpp"
#endif
#include "relayout.hpp"
#include "scan.hpp"

using namespace fnv_dev;

namespace {

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess)                                                                               \
      return fail(FNV_ERR_NO_DEVICE, std::string(#expr) + " failed: " + hipGetErrorString(_e));        \
  } while (0)

// Every entry point works on its index's device and gives the calling thread its current device back on every exit
// path: a library call must not move a torch (or any other HIP) caller's allocations to another GPU.
struct DeviceScope {
  int prev = -1;
  bool moved = false;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) {
      err = hipSetDevice(device);
      moved = err == hipSuccess;
    }
  }
  ~DeviceScope() {
    if (moved && prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};
#define ON_DEVICE(dev)                  \
  DeviceScope device_scope_(dev);       \
  HIP_TRY(device_scope_.err)

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
wire_fn pick_wire_kernel(int dtype, int metric, int cfg, bool full) { return kernel_table(dtype, metric).select[cfg][full]; }
wire_fn pick_connect_kernel(int dtype, int metric, int cfg, bool full) { return kernel_table(dtype, metric).connect[cfg][full]; }

}  // namespace

// The cached launch plan of a handle (launch_plan.hpp) and the kernels that run it.
// A search kernel TOGETHER WITH the vector table it reads (bind_search_kernel is the only place that makes one): a launch
// takes the function and `vectors` / `row_bytes` of its parameter block from the same BoundKernel, so a float32 kernel on
// mirror rows -- or the reverse, either of which reads out of bounds -- cannot be written down.
struct BoundKernel {
  kernel_fn fn = nullptr;
  const uint8_t* rows = nullptr;  // what SearchParams::vectors must be for fn
  uint32_t stride = 0;            // ... and SearchParams::row_bytes
  bool half_rows = false;         // fn reads the half-width mirror
};
struct PlannedLaunch : LaunchPlan {
  BoundKernel kern, skern;    // exact two-heap kernel; merged-beam kernel (mode != 0)
  BoundKernel skern_direct;   // ... its DIRECT form (small launches on small indexes)
  BoundKernel fkern;          // filtered search: the two-heap kernel's filtered form on the `heaps` layout (set at first use)
  int fbpc = 0;               // ... and the slots one CU keeps resident with it
  bool half_rows = false;     // planned for the half-width mirror (another kernel: its own occupancy, its own measurements)
};

// Filtered search (fnv_search_batch_filtered*): the caller's bitmap over label values, in device memory.
struct SearchFilter {
  const uint8_t* bits;  // byte L >> 3, bit L & 7 = label L allowed (null when n_bits == 0)
  uint64_t n_bits;
  // Grouped calls (fnv_search_batch_*_grouped): `bits` is a table of n_filters such bitmaps `stride` bytes apart, and query q
  // uses the one query_filter[q] names (scan_select.hpp, filter_row).  A single-filter call is not a grouped call with one row.
  bool grouped = false;
  uint64_t n_filters = 0, stride = 0;
  const int32_t* query_filter = nullptr;  // [nq]
  uint64_t rows() const { return n_filters + 2; }  // the node bitmaps of a grouped launch
};

// Where a search writes: [nq][K] distances and labels, and per query (each optional) the result count and the counters.
struct SearchOutputs {
  float* dist = nullptr;
  int32_t* labels = nullptr;
  int32_t* count = nullptr;
  uint64_t *ndist = nullptr, *nhops = nullptr;
};

// One slab of `nq` x `K` results at `base`: dist | labels | count | ndist | nhops (the counters 8-byte aligned).
// Returns the arrays; `bytes`: the slab's size (a null `base` asks for that alone).
static SearchOutputs lay_out_slab(void* base, uint64_t nq, int K, size_t* bytes = nullptr) {
  const uintptr_t b = (uintptr_t)base;
  const size_t o_lab = (size_t)nq * K * 4;
  const size_t o_cnt = o_lab + (size_t)nq * K * 4;
  const size_t o_nd = (o_cnt + (size_t)nq * 4 + 7) & ~(size_t)7;
  const size_t o_nh = o_nd + (size_t)nq * 8;
  if (bytes) *bytes = o_nh + (size_t)nq * 8;
  return SearchOutputs{(float*)b, (int32_t*)(b + o_lab), (int32_t*)(b + o_cnt), (uint64_t*)(b + o_nd), (uint64_t*)(b + o_nh)};
}

// What one search launch does differently from a plain one: a call names only what it changes.
struct SearchOptions {
  bool node_ids = false;            // write node ids whatever "output_node_ids" says (the device builder's beams)
  int force_variant = -1;           // >= 0: fnv_tune's launches (an argument, not index state: a concurrent caller's launch on
                                    // the same handle is never forced)
  int32_t* host_status = nullptr;   // zero-copy small searches: the error flag's copy in the caller's pinned slab
  const SearchFilter* filter = nullptr;  // filtered search: every query runs the filtered two-heap kernel
  bool exhaustive = false;          // fnv_search_batch_exhaustive: no graph search at all -- the scan of scan.hpp (over the
                                    // filter's nodes, if there is one)
};

// A host-buffer search that went through a pinned slab: what search_host_finish copies where.
struct PinnedCall {
  bool active = false;
  SearchOutputs slab, user;  // the results in pinned memory; the caller's arrays
  const int32_t* status = nullptr;
  uint64_t nq = 0;
  int K = 0;
  void arm(const SearchOutputs& slab_, const int32_t* status_, const SearchOutputs& user_, uint64_t nq_, int K_) {
    active = true;
    slab = slab_;
    status = status_;
    user = user_;
    nq = nq_;
    K = K_;
  }
};

// A buffer that grows on demand (never shrinks) and frees itself with its owner: device memory, or pinned host memory.
struct DeviceBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  const bool host;
  explicit DeviceBuf(bool pinned_host = false) : host(pinned_host) {}
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  ~DeviceBuf() { release(); }
  template <typename T>
  T* as() const { return (T*)ptr; }
  // At least `need` bytes (`headroom` more when it has to be allocated anew); the contents are not kept.
  int grow(size_t need, bool zero = false, size_t headroom = 0) {
    if (need <= bytes) return FNV_OK;
    if (ptr) HIP_TRY(host ? hipHostFree(ptr) : hipFree(ptr));
    ptr = nullptr;
    bytes = 0;
    HIP_TRY(host ? hipHostMalloc(&ptr, need + headroom, hipHostMallocDefault) : hipMalloc(&ptr, need + headroom));
    if (zero) HIP_TRY(hipMemset(ptr, 0, need + headroom));
    bytes = need + headroom;
    return FNV_OK;
  }
  size_t release() {  // returns the bytes given back
    if (ptr) (void)(host ? hipHostFree(ptr) : hipFree(ptr));
    const size_t freed = bytes;
    ptr = nullptr;
    bytes = 0;
    return freed;
  }
};

struct fnv_index_s : PlanInputs {  // (options, table geometry, capacity, num_cus: what the planner reads)
  bool owns_buffers = true;  // false: a view (fnv_index_view) of another handle's vectors / links / labels
  fnv_index_s* parent = nullptr;  // a view's source: its live node count is read at every launch
  std::atomic<int> n_views{0};    // live views of this handle's buffers (it cannot be freed before them)
  int device = 0;
  int metric = FNV_METRIC_L2;
  const uint8_t* tails() const { return tail_bytes ? d_vectors + capacity * (uint64_t)row_bytes : nullptr; }
  uint64_t vector_bytes() const { return capacity * ((uint64_t)row_bytes + tail_bytes); }
  std::atomic<uint64_t> n_nodes{0};  // live nodes: what a search sees (entry scan, id range); a view reads its source's at
                                     // every launch while the source may be growing -> atomic
  uint8_t* d_vectors = nullptr;
  // The half-width mirror of a float32 table (half_rows.hpp): an allocation of its own, kept by the handle that
  // made it (the owner of the buffers, or an adopted handle after fnv_index_build_half_rows).  Views and hidden lanes read
  // their source's at every launch, as they read n_nodes -> atomics; `rows` is published before `state` turns HALF_LIVE.
  struct HalfRows {
    std::atomic<uint8_t*> rows{nullptr};  // [capacity][row_bytes / 2]
    std::atomic<int> state{HALF_NONE};
    std::atomic<uint64_t> covered{0};     // rows [0, covered) are converted (a contiguous watermark from row 0)
    std::atomic<size_t> bytes{0};
    bool off = false;                     // FLATNAV_HALF_ROWS=0 when the handle was made: never built
  } half;
  int measured_half = -1;  // tuner / layouts hold measurements of launches with (1) / without (0) the mirror; -1: none yet
  bool last_half = false;  // the most recent launch read the mirror
  uint32_t* d_links = nullptr;
  int32_t* d_labels = nullptr;
  std::string gcn_arch;  // hipDeviceProp_t::gcnArchName: replicas on the same GPU model inherit the source's measurements
  uint64_t options_version = 0;
  PlannedLaunch plan;
  // adaptive kernel choice ("sorted_beam" = 2) and the layouts fnv_tune measured, per beam width (launch_plan.hpp)
  std::map<int, LayoutChoice> layouts;
  std::map<int, Tuner> tuner;
  int sample_B = 0, sample_kernel = -1;  // the launch between ev0 / ev1 is a sample for this entry (-1: it is not)
  uint64_t sample_nq = 0;
  int last_variant = 0;          // what the most recent launch ran: 0 two-heap kernel, 1 merged beam, 2-4 with exact tail
  bool last_exploratory = false;  // ... and whether the adaptive choice was still sampling (not its final pick)
  bool last_shadow = false;       // ... and whether every query had an exact shadow (small launches)
  // host-buffer searches: steady-clock time of launch / of completion (atomic: every lane's caller reports into the handle)
  std::atomic<uint64_t> t_enqueue_ns{0}, t_complete_ns{0};
  uint32_t* d_dispenser = nullptr;  // [0] dispenser, [1] status, [3] queries a merged-beam launch handed to the exact search, [4..7] by
                                    // reason, [8] of them resumed from their log, [9] hops taken from logs, [10] hops of those queries
  unsigned long long* d_phase = nullptr;  // profiling builds only
  // The launch workspace, per query slot: what search_device_impl grows, free_lane_workspace gives back and ws_bytes counts.
  struct Workspace {
    DeviceBuf bitmap;  // uint32 [nslots][bitmap_words]: the visited set's HBM part
    DeviceBuf ovf;     // uint32 [nslots][ovf_cap] ids whose bitmap words need clearing (big indexes)
    DeviceBuf spill;   // uint64 [nslots][spill_entries]: what the candidates heap does not keep in LDS
    DeviceBuf tielog;  // uint64, merged-beam kernel: [nslots][log_entries] hand-over log (round 5)
    DeviceBuf scan;    // uint64, exhaustive search: [nq][segments][K] partial lists (scan.hpp)
    DeviceBuf group;   // uint32, grouped exhaustive search: the grouping arrays (GroupArrays), O(nq + n_filters)
    DeviceBuf rows;    // uint32, grouped searches: [n_filters + 2][capacity / 32] node bitmaps (node_filter_table_kernel) -- here,
                       // not in d_nodebits: the caller's n_filters sizes them, so lane admission and ws_bytes must see them
    size_t bytes() const { return bitmap.bytes + ovf.bytes + spill.bytes + tielog.bytes + scan.bytes + group.bytes + rows.bytes; }
    size_t release() {
      return bitmap.release() + ovf.release() + spill.release() + tielog.release() + scan.release() + group.release() + rows.release();
    }
  } ws;
  // further buffers, each grown on demand
  DeviceBuf d_entry;      // [nq] uint32 entry nodes | [nq] float entry distances (K0 output)
  DeviceBuf d_done;       // uint32, shadow mode: [nq] "answered" flags
  DeviceBuf d_nodebits;   // uint32, filtered search: [capacity / 32] words, bit per node id (node_filter_kernel)
  DeviceBuf d_allowed;    // filtered search, host-buffer entry point: the caller's label bitmap staged in HBM (grouped calls:
                          // the filter table, then query_filter)
  DeviceBuf d_scanids;    // uint32, filtered exhaustive search: [0] the count, [4 ...) the allowed node ids (capacity of them)
  DeviceBuf d_wirebuf;    // fnv_index_insert_batch: [count*keep] x {req_target, req_index, sorted_target, sorted_req} | sort scratch
  DeviceBuf d_nodestage;  // write_nodes: AoS staging chunk + bad flag + "not lossless" flag of the mirror's conversion
  DeviceBuf d_halfflag;   // fnv_index_build_half_rows: the conversion's "not lossless" flag
  DeviceBuf d_linkstage;  // fnv_index_write_links: [count] ids | [count][M] rows | bad flag
  // staging for the host-buffer entry point
  DeviceBuf d_q, d_out;
  void* h_pin = nullptr;  // 1 MB of pinned host memory: staging of small host-buffer searches
  DeviceBuf h_res{true};  // pinned host memory for the result slab of larger host-buffer searches
  PinnedCall pin;
  hipStream_t stream = nullptr;  // owned, used by fnv_search_batch
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipStream_t last_stream = nullptr;
  bool launched = false;
  uint64_t geom[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::mutex mu;       // launch configuration + workspace growth
  std::mutex host_mu;  // the host-buffer entry point owns d_q / d_out / stream for the whole call
  // Round 4: a SECOND LANE for concurrent host-buffer callers.  Two threads calling fnv_search_batch on one handle used to
  // take turns; now the second caller runs on a hidden view of the handle (own stream, workspace and staging, the same HBM
  // buffers), so its copies and its launch overlap the first caller's -- the reference's search is callable from several
  // threads at once (bindings.cpp:198-211 runs it under executeInParallel), and two launches in flight are what hides a
  // launch's ramp and drain.  Created on first contention; freed with the handle.
  // Round 5: EVERY lane is admitted by the HBM its launch workspace would really take (lane_workspace_bytes: slots x (visited
  // bitmap + overflow list + candidate spill area) for this batch size and the plan's residency) against a budget for all
  // hidden lanes together -- an eighth of the device's memory (36 GB of 288): one full-grid lane at 50M nodes (19 GB), three
  // at 10M, all seven at 1M; 1024-query batches at 50M nodes cost 6.4 GB each, so five of those.  A lane that does not fit
  // is not used (the caller waits for the handle, as before lanes existed); an idle lane's workspace is released when the
  // budget or the owner's own allocation needs the room (release_idle_lanes).
  static constexpr int kMaxLanes = 8;
  bool is_lane = false;          // a hidden lane: never samples or explores (it copies the owner's measurements)
  std::atomic<uint64_t> explored_launches{0};  // launches that were exploratory samples of the adaptive choice
  std::atomic<size_t> ws_bytes{0};  // launch workspace this handle holds (visited bitmaps + overflow lists + spill areas)
  size_t lane_budget_bytes = 0;  // owner: budget for the hidden lanes' workspaces together (set at creation)
  std::atomic<fnv_index_s*> lanes[kMaxLanes] = {};  // [0] unused; written under lane_mu, read anywhere
  std::mutex lane_mu;            // creation of lanes
  std::atomic<fnv_index_s*> last_served{nullptr};  // the lane that ran the handle's most recent launch (null: the handle itself):
                                                   // fnv_last_kernel_ms / _replayed_queries / _handover_stats read ITS events and counters
  uint64_t tune_epoch = 0;       // bumped whenever tuner / layouts change: a lane copies them when its own epoch lags
  uint64_t lane_epoch = ~0ull, lane_options = ~0ull;  // (on a lane: what it last copied from its owner)
  // (on a replica, round 6) the handle fnv_replica_refresh last copied options from, that handle's options_version then, and
  // the tune_epoch whose measurements this replica holds: fnv_search_batch_multi hands newer measurements over (pointer
  // compared, never followed, outside calls that were given the source itself)
  const fnv_index_s* replica_of = nullptr;
  uint64_t replica_options = ~0ull, replica_epoch = ~0ull;
};

namespace {

int index_common_init(fnv_index_s* ix) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, ix->device));
  ix->num_cus = prop.multiProcessorCount;
  ix->gcn_arch = prop.gcnArchName;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;
    (void)hipGetLastError();
    ix->lane_budget_bytes = total_b / 8;
    if (const char* env = getenv("FLATNAV_LANE_BUDGET_MB")) ix->lane_budget_bytes = (size_t)strtoull(env, nullptr, 10) << 20;
  }
  if (const char* env = getenv("FLATNAV_HALF_ROWS")) ix->half.off = env[0] == '0';
  HIP_TRY(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&ix->ev0));
  HIP_TRY(hipEventCreate(&ix->ev1));
  HIP_TRY(hipMalloc(&ix->d_dispenser, 16 * sizeof(uint32_t)));
  HIP_TRY(hipMemset(ix->d_dispenser, 0, 16 * sizeof(uint32_t)));
#ifdef FNV_PHASE_TIMING
  HIP_TRY(hipMalloc(&ix->d_phase, NPHASE * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(ix->d_phase, 0, NPHASE * sizeof(unsigned long long)));
#endif
  return FNV_OK;
}

int validate_geometry(uint32_t M, uint64_t n_nodes, int data_type, int metric, uint32_t dim) {
  if (dtype_size(data_type) == 0) return fail(FNV_ERR_RUNTIME, "Unsupported data type");
  if (metric != FNV_METRIC_L2 && metric != FNV_METRIC_IP) return fail(FNV_ERR_INVALID, "Invalid metric");
  if (M == 0 || dim == 0) return fail(FNV_ERR_INVALID, "M and dim must be positive");
  if (n_nodes == 0) return fail(FNV_ERR_INVALID, "cannot upload an empty index");
  if (n_nodes >= 0xFFFFFFFFull) return fail(FNV_ERR_INVALID, "too many nodes for 32-bit node ids");
  return FNV_OK;
}

int alloc_buffers(fnv_index_s* ix) {  // the caller is on ix->device
  HIP_TRY(hipMalloc(&ix->d_vectors, ix->vector_bytes()));
  HIP_TRY(hipMalloc(&ix->d_links, ix->capacity * (uint64_t)ix->M * 4));
  HIP_TRY(hipMalloc(&ix->d_labels, ix->capacity * 4));
  return index_common_init(ix);
}

// ---- the half-width mirror (half_rows.hpp) ---------------------------------------------------------------------
// The handle whose mirror a launch on `ix` reads: a view's / hidden lane's source, else the handle itself.
const fnv_index_s* rows_source(const fnv_index_s* ix) { return ix->parent ? ix->parent : ix; }
// Whether this handle's rows can have one at all: float32 rows of an eligible geometry, in a build that has the kernels.
bool half_rows_possible(const fnv_index_s* ix) {
  return kHalfRowsBuilt && !ix->half.off && half_rows_eligible(ix->dtype, row_geometry(ix));
}
// The mirror is given up: searches stop using it at their next launch.  The memory goes back at once unless a view (or hidden
// lane) may be launching on it this very moment -- then it stays until the handle is freed.  The caller is on ix->device.
void half_rows_drop(fnv_index_s* ix) {
  fnv_index_s::HalfRows& h = ix->half;
  h.state = HALF_DROPPED;
  h.covered = 0;
  if (h.rows.load() && ix->n_views.load() == 0) {
    (void)hipDeviceSynchronize();
    (void)hipFree(h.rows.load());
    h.rows = nullptr;
    h.bytes = 0;
  }
}
// Room for the mirror of every row the buffers hold.  A failed allocation is not an error: there is no mirror then.
bool half_rows_allocate(fnv_index_s* ix) {
  fnv_index_s::HalfRows& h = ix->half;
  if (h.rows.load()) return true;
  void* p = nullptr;
  const size_t bytes = (size_t)ix->capacity * (ix->row_bytes / 2);
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  h.rows = (uint8_t*)p;
  h.bytes = bytes;
  return true;
}
// Converts rows [first, first + count) of d_vectors into the mirror on the null stream; *d_lossy is ORed.  The caller waits.
void half_rows_convert(fnv_index_s* ix, uint64_t first, uint64_t count, int* d_lossy) {
  const RowGeometry g = row_geometry(ix);
  const uint64_t units = count * (ix->row_bytes / 32);
  hipLaunchKernelGGL(half_rows_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, 0, ix->d_vectors, ix->row_bytes, first,
                     count, (uint32_t)kCfgs[g.cfg].G, (uint32_t)kCfgs[g.cfg].CU, ix->half.rows.load(), d_lossy);
}
// (Re)builds the mirror of rows [0, n_live) from d_vectors; the caller holds ix->mu and is on ix->device.  *built: a live mirror resulted.
int half_rows_build(fnv_index_s* ix, int* built) {
  *built = 0;
  if (ix->parent) return fail(FNV_ERR_INVALID, "fnv_index_build_half_rows: call it on the view's source (a view reads its source's mirror)");
  if (!half_rows_possible(ix)) return FNV_OK;
  const uint64_t live = ix->n_nodes.load();
  if (!half_rows_allocate(ix)) {
    half_rows_drop(ix);
    return FNV_OK;
  }
  int rc = ix->d_halfflag.grow(16);
  if (rc) return rc;
  HIP_TRY(hipMemset(ix->d_halfflag.ptr, 0, sizeof(int)));
  half_rows_convert(ix, 0, live, ix->d_halfflag.as<int>());
  HIP_TRY(hipGetLastError());
  int lossy = 0;
  HIP_TRY(hipMemcpy(&lossy, ix->d_halfflag.ptr, sizeof(int), hipMemcpyDeviceToHost));  // (waits for the null stream)
  if (lossy) {
    half_rows_drop(ix);
    return FNV_OK;
  }
  ix->half.covered = live;
  ix->half.state = HALF_LIVE;
  *built = 1;
  return FNV_OK;
}

// Copy AoS node records [data][M links][label] (reference Index.h:61-63) for nodes first..first+count-1 into the
// SoA device buffers, 256 MB at a time.  Link ids >= id_limit are flagged (and replaced by a self-loop).
// The half-width mirror follows the rows written here: converted chunk by chunk right behind the re-layout while the writes
// stay contiguous from row 0 and every value is lossless; a gap, a lossy value or a failed allocation ends it for good.
int write_nodes_impl(fnv_index_s* ix, uint64_t first_node, uint64_t count_nodes, const void* aos_rows,
                     uint64_t node_size, uint64_t data_size, uint64_t id_limit, int* bad_out) {
  ON_DEVICE(ix->device);
  const uint64_t chunk_nodes = std::max<uint64_t>(1, (256ull << 20) / node_size);
  // staging area: [chunk of AoS records][bad flag]; kept on the index (a device build writes dozens of batches)
  const size_t need = std::min(chunk_nodes, count_nodes) * node_size + 16;
  int rcg = ix->d_nodestage.grow(need);
  if (rcg) return rcg;
  uint8_t* d_stage = ix->d_nodestage.as<uint8_t>();
  int* d_bad = (int*)(d_stage + (need - 16));  // [0] bad link ids, [1] the mirror's "not lossless" flag
  HIP_TRY(hipMemset(d_bad, 0, 2 * sizeof(int)));
  bool mirror = false;  // this call converts what it writes
  if (ix->parent) {     // written through a view: its source's mirror no longer matches the rows (the memory stays the source's)
    if (ix->parent->half.state.load() == HALF_LIVE) ix->parent->half.state = HALF_DROPPED;
  } else if (half_rows_possible(ix) && ix->half.state.load() != HALF_DROPPED) {
    fnv_index_s::HalfRows& h = ix->half;
    if (first_node > h.covered.load()) half_rows_drop(ix);  // a gap: the rows before it came from somewhere the library did not see
    else if (ix->owns_buffers || h.rows.load()) {           // (an adopted handle only keeps up a mirror it was asked to build)
      mirror = half_rows_allocate(ix);
      if (!mirror) half_rows_drop(ix);
    }
  }
  const int word_ok = (node_size % 4 == 0 && data_size % 4 == 0) ? 1 : 0;
  for (uint64_t done = 0; done < count_nodes; done += chunk_nodes) {
    const uint64_t count = std::min(chunk_nodes, count_nodes - done);
    const uint64_t first = first_node + done;
    HIP_TRY(hipMemcpy(d_stage, (const uint8_t*)aos_rows + done * node_size, count * node_size, hipMemcpyHostToDevice));
    const uint32_t row_all = ix->row_bytes + ix->tail_bytes;  // bytes of a row over both tables
    const uint64_t units = count * (word_ok ? row_all / 4 : row_all);
    hipLaunchKernelGGL(relayout_vectors_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, 0, d_stage,
                       node_size, data_size, ix->row_bytes, ix->tail_bytes, first, count, ix->d_vectors,
                       const_cast<uint8_t*>(ix->tails()), word_ok);
    if (mirror) half_rows_convert(ix, first, count, d_bad + 1);
    hipLaunchKernelGGL(relayout_links_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, d_stage,
                       node_size, data_size, ix->M, first, count, id_limit, ix->d_links, ix->d_labels, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (mirror) {  // a lossy value ends the mirror at once: the chunks that follow are not converted for nothing
      int lossy = 0;
      HIP_TRY(hipMemcpy(&lossy, d_bad + 1, sizeof(int), hipMemcpyDeviceToHost));
      if (lossy) {
        half_rows_drop(ix);
        mirror = false;
      }
    }
  }
  int flags[2] = {0, 0};
  HIP_TRY(hipMemcpy(flags, d_bad, sizeof(flags), hipMemcpyDeviceToHost));
  *bad_out = flags[0];
  if (mirror && flags[1]) half_rows_drop(ix);
  else if (mirror) {
    ix->half.covered = std::max<uint64_t>(ix->half.covered.load(), first_node + count_nodes);
    ix->half.state = HALF_LIVE;
  }
  return FNV_OK;
}

}  // namespace

// Only the C ABI is exported (the library is built with -fvisibility=hidden).
#pragma GCC visibility push(default)
extern "C" {

const char* fnv_last_error(void) { return g_err.c_str(); }
const char* fnv_version(void) { return "flatnav_hip gfx950 r6"; }

int fnv_device_count(int* count) {
  if (!count) return fail(FNV_ERR_INVALID, "count is null");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(FNV_ERR_NO_DEVICE, std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e));
  }
  *count = n;
  return FNV_OK;
}

int fnv_row_layout(uint32_t dim, int data_type, uint64_t capacity, uint32_t* row_bytes, uint32_t* tail_bytes) {
  if (!row_bytes || !tail_bytes) return fail(FNV_ERR_INVALID, "null argument");
  if (dtype_size(data_type) == 0) return fail(FNV_ERR_RUNTIME, "Unsupported data type");
  if (dim == 0 || capacity == 0) return fail(FNV_ERR_INVALID, "dim and capacity must be positive");
  const RowLayout lay = row_layout(dim, data_type, capacity);
  *row_bytes = lay.row_bytes;
  *tail_bytes = lay.tail_bytes;
  return FNV_OK;
}

int fnv_index_alloc(uint32_t M, uint64_t n_nodes, int data_type, int metric, uint32_t dim, int device,
                    fnv_index_t* out) {
  if (!out) return fail(FNV_ERR_INVALID, "out is null");
  int rc = validate_geometry(M, n_nodes, data_type, metric, dim);
  if (rc) return rc;
  ON_DEVICE(device);
  fnv_index_s* ix = new fnv_index_s();
  ix->device = device;
  ix->dtype = data_type;
  ix->metric = metric;
  ix->M = M;
  ix->dim = dim;
  ix->n_nodes = n_nodes;
  ix->capacity = n_nodes;
  const RowLayout lay = row_layout(dim, data_type, n_nodes);
  ix->row_bytes = lay.row_bytes;
  ix->tail_bytes = lay.tail_bytes;
  rc = alloc_buffers(ix);
  if (rc) {
    fnv_index_free(ix);
    return rc;
  }
  *out = ix;
  return FNV_OK;
}

int fnv_index_upload(const void* aos_blob, uint64_t node_size, uint64_t data_size, uint32_t M, uint64_t n_nodes,
                     int data_type, int metric, uint32_t dim, int device, fnv_index_t* out) {
  if (!aos_blob || !out) return fail(FNV_ERR_INVALID, "null argument");
  int rc = validate_geometry(M, n_nodes, data_type, metric, dim);
  if (rc) return rc;
  if (data_size != (uint64_t)dim * dtype_size(data_type) || node_size != data_size + 4ull * M + 4)
    return fail(FNV_ERR_INVALID, "node geometry does not match [data][M links][label] (Index.h:176)");
  fnv_index_t ix = nullptr;
  rc = fnv_index_alloc(M, n_nodes, data_type, metric, dim, device, &ix);
  if (rc) return rc;

  int bad = 0;
  rc = write_nodes_impl(ix, 0, n_nodes, aos_blob, node_size, data_size, n_nodes, &bad);
  ix->d_nodestage.release();  // a one-off upload does not keep its (up to 256 MB) staging chunk
  if (rc) {
    fnv_index_free(ix);
    return rc;
  }
  if (bad) {
    fnv_index_free(ix);
    return fail(FNV_ERR_RUNTIME, "index blob holds link ids outside [0, n_nodes)");
  }
  *out = ix;
  return FNV_OK;
}

int fnv_index_view(fnv_index_t src, fnv_index_t* out) {
  if (!src || !out) return fail(FNV_ERR_INVALID, "null argument");
  fnv_index_s* v = new fnv_index_s();
  v->owns_buffers = false;
  v->device = src->device;
  static_cast<PlanInputs&>(*v) = static_cast<const PlanInputs&>(*src);  // options, row geometry, capacity
  v->metric = src->metric;
  v->n_nodes = src->n_nodes.load();
  v->d_vectors = src->d_vectors;
  v->d_links = src->d_links;
  v->d_labels = src->d_labels;
  v->parent = src->parent ? src->parent : src;  // a view of a view hangs off the owner
  v->parent_capacity = v->parent->capacity;
  DeviceScope scope(v->device);
  if (scope.err != hipSuccess) {
    delete v;
    return fail(FNV_ERR_NO_DEVICE, "hipSetDevice failed");
  }
  int rc = index_common_init(v);
  if (rc) {
    v->parent = nullptr;
    fnv_index_free(v);
    return rc;
  }
  v->parent->n_views.fetch_add(1);
  *out = v;
  return FNV_OK;
}

int fnv_index_adopt(const void* vectors, const void* links, const void* labels, uint32_t M, uint64_t n_nodes, int data_type,
                    int metric, uint32_t dim, int device, fnv_index_t* out) {
  if (!vectors || !links || !labels || !out) return fail(FNV_ERR_INVALID, "null argument");
  int rc = validate_geometry(M, n_nodes, data_type, metric, dim);
  if (rc) return rc;
  if (((uintptr_t)vectors & 15u) || ((uintptr_t)links & 3u) || ((uintptr_t)labels & 3u))
    return fail(FNV_ERR_INVALID, "fnv_index_adopt: vectors must be 16-byte aligned, links and labels 4-byte aligned");
  fnv_index_s* v = new fnv_index_s();
  v->owns_buffers = false;
  v->device = device;
  v->dtype = data_type;
  v->metric = metric;
  v->M = M;
  v->dim = dim;
  const RowLayout lay = row_layout(dim, data_type, n_nodes);  // (the owner's layout: same dim, type and capacity)
  v->row_bytes = lay.row_bytes;
  v->tail_bytes = lay.tail_bytes;
  v->n_nodes = n_nodes;
  v->capacity = n_nodes;
  v->d_vectors = (uint8_t*)const_cast<void*>(vectors);
  v->d_links = (uint32_t*)const_cast<void*>(links);
  v->d_labels = (int32_t*)const_cast<void*>(labels);
  DeviceScope scope(device);
  if (scope.err != hipSuccess) {
    delete v;
    return fail(FNV_ERR_NO_DEVICE, "hipSetDevice failed");
  }
  rc = index_common_init(v);
  if (rc) {
    fnv_index_free(v);
    return rc;
  }
  *out = v;
  return FNV_OK;
}

int fnv_index_device_buffers(fnv_index_t ix, void* ptrs[3], uint64_t sizes[3]) {
  if (!ix || !ptrs || !sizes) return fail(FNV_ERR_INVALID, "null argument");
  ptrs[0] = ix->d_vectors;
  ptrs[1] = ix->d_links;
  ptrs[2] = ix->d_labels;
  sizes[0] = ix->vector_bytes();  // (split rows: the main table, then the side table)
  sizes[1] = ix->capacity * (uint64_t)ix->M * 4;
  sizes[2] = ix->capacity * 4;
  return FNV_OK;
}

int fnv_index_info(fnv_index_t ix, uint64_t info[8]) {
  if (!ix || !info) return fail(FNV_ERR_INVALID, "null argument");
  info[0] = (uint64_t)ix->dtype;
  info[1] = ix->M;
  info[2] = (uint64_t)ix->row_bytes | ((uint64_t)ix->tail_bytes << 32);
  info[3] = ix->parent ? ix->parent->n_nodes.load() : ix->n_nodes.load();
  info[4] = ix->dim;
  info[5] = (uint64_t)ix->metric;
  info[6] = (uint64_t)ix->device;
  info[7] = ix->capacity * ((uint64_t)ix->row_bytes + ix->tail_bytes + 4ull * ix->M + 4) + ix->ws.bitmap.bytes + ix->ws.spill.bytes + ix->half.bytes.load();
  return FNV_OK;
}

int fnv_index_free(fnv_index_t ix) {
  if (!ix) return FNV_OK;
  for (std::atomic<fnv_index_s*>& l : ix->lanes) {  // the hidden lanes go first (they count as views of this handle)
    fnv_index_s* gone = l.exchange(nullptr);
    if (gone) (void)fnv_index_free(gone);
  }
  if (ix->n_views.load() > 0)
    return fail(FNV_ERR_INVALID, "fnv_index_free: the index still has live views (fnv_index_view) on its buffers; free them first");
  DeviceScope scope(ix->device);
  if (ix->stream) (void)hipStreamSynchronize(ix->stream);
  if (ix->parent) ix->parent->n_views.fetch_sub(1);
  if (!ix->owns_buffers) ix->d_vectors = nullptr, ix->d_links = nullptr, ix->d_labels = nullptr;
  for (void* b : {(void*)ix->half.rows.load(), (void*)ix->d_vectors, (void*)ix->d_links, (void*)ix->d_labels, (void*)ix->d_dispenser, (void*)ix->d_phase})
    if (b) (void)hipFree(b);
  if (ix->h_pin) (void)hipHostFree(ix->h_pin);
  if (ix->ev0) (void)hipEventDestroy(ix->ev0);
  if (ix->ev1) (void)hipEventDestroy(ix->ev1);
  if (ix->stream) (void)hipStreamDestroy(ix->stream);
  delete ix;  // (every DeviceBuf frees itself)
  return FNV_OK;
}

int fnv_index_build_half_rows(fnv_index_t ix, int* built) {
  if (!ix) return fail(FNV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  int made = 0;
  const int rc = half_rows_build(ix, &made);
  if (built) *built = made;
  return rc;
}

int fnv_index_half_rows(fnv_index_t ix, uint64_t info[4]) {
  if (!ix || !info) return fail(FNV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(ix->mu);
  const fnv_index_s* src = rows_source(ix);
  const int state = src->half.state.load();
  info[0] = (uint64_t)(!half_rows_eligible(ix->dtype, row_geometry(ix)) ? HALF_INELIGIBLE : state);
  info[1] = state == HALF_LIVE ? src->half.covered.load() : 0;
  info[2] = src->half.bytes.load();
  info[3] = ix->last_half ? 1 : 0;
  return FNV_OK;
}

int fnv_index_set_live_nodes(fnv_index_t ix, uint64_t n_live) {
  if (!ix) return fail(FNV_ERR_INVALID, "null argument");
  if (n_live == 0 || n_live > ix->capacity)
    return fail(FNV_ERR_INVALID, "live node count must be in [1, capacity]");
  std::lock_guard<std::mutex> lock(ix->mu);
  ix->n_nodes = n_live;
  return FNV_OK;
}

int fnv_index_write_nodes(fnv_index_t ix, uint64_t first_node, uint64_t count, const void* aos_rows,
                          uint64_t node_size, uint64_t data_size) {
  if (!ix || (!aos_rows && count)) return fail(FNV_ERR_INVALID, "null argument");
  if (data_size != (uint64_t)ix->dim * dtype_size(ix->dtype) || node_size != data_size + 4ull * ix->M + 4)
    return fail(FNV_ERR_INVALID, "node geometry does not match [data][M links][label] (Index.h:176)");
  if (first_node > ix->capacity || count > ix->capacity - first_node)
    return fail(FNV_ERR_RUNTIME, "Maximum number of nodes reached. (device index capacity)");
  if (count == 0) return FNV_OK;
  std::lock_guard<std::mutex> lock(ix->mu);
  int bad = 0;
  int rc = write_nodes_impl(ix, first_node, count, aos_rows, node_size, data_size, ix->capacity, &bad);
  if (rc) return rc;
  if (bad) return fail(FNV_ERR_RUNTIME, "node records hold link ids outside [0, capacity)");
  return FNV_OK;
}

int fnv_index_write_links(fnv_index_t ix, const uint32_t* node_ids, const uint32_t* link_rows, uint64_t count) {
  if (!ix || ((!node_ids || !link_rows) && count)) return fail(FNV_ERR_INVALID, "null argument");
  if (count == 0) return FNV_OK;
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  const size_t need = (size_t)count * (4 + 4ull * ix->M) + sizeof(int);
  int rc = ix->d_linkstage.grow(need, false, need / 2);
  if (rc) return rc;
  uint32_t* d_ids = ix->d_linkstage.as<uint32_t>();
  uint32_t* d_rows = d_ids + count;
  int* d_bad = (int*)(d_rows + count * ix->M);
  HIP_TRY(hipMemcpy(d_ids, node_ids, count * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_rows, link_rows, count * 4ull * ix->M, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_bad, 0, sizeof(int)));
  hipLaunchKernelGGL(scatter_links_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, d_ids, d_rows, count,
                     ix->M, ix->capacity, ix->d_links, d_bad);
  HIP_TRY(hipGetLastError());
  int bad = 0;
  HIP_TRY(hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost));
  if (bad) return fail(FNV_ERR_RUNTIME, "link rows hold node ids outside [0, capacity)");
  return FNV_OK;
}

int fnv_set_option(fnv_index_t ix, const char* name, int64_t value) {
  if (!ix || !name) return fail(FNV_ERR_INVALID, "null argument");
  std::string n(name);
  if (value < 0 && !((n == "sorted_tail_exact_pct" || n == "sorted_variant") && value == -1))
    return fail(FNV_ERR_INVALID, "option values must be non-negative");
  // Under the handle's mutex (round 5): a launch reads the options, the tuner and the layouts under it, and a concurrent
  // caller's lane copies them under it (sync_lane) -- an option may change while other threads search; each launch sees the
  // options either before or after the change.
  std::lock_guard<std::mutex> lock(ix->mu);
  if (n == "visited_factor") ix->visited_factor = std::max<int64_t>(1, value);
  else if (n == "visited_slots") {
    if (value && (value & (value - 1)) && ((value % 3) || ((value / 3) & (value / 3 - 1))))
      return fail(FNV_ERR_INVALID, "visited_slots must be 2^j or 3*2^j");
    if (value && value < 256) return fail(FNV_ERR_INVALID, "visited_slots must be at least 256");
    ix->visited_slots = value;
  } else if (n == "visited_floor") ix->visited_floor = std::max<int64_t>(256, value);
  else if (n == "occupancy_target") ix->occupancy_target = value;
  else if (n == "occupancy_roomy") ix->occupancy_roomy = std::max<int64_t>(1, value);
  else if (n == "cand_factor") ix->cand_factor = std::max<int64_t>(1, value);
  else if (n == "cand_slots") ix->cand_slots = value;
  else if (n == "spill_entries") ix->spill_entries = std::max<int64_t>(1, value);
  else if (n == "blocks_per_cu") ix->blocks_per_cu = value;
  else if (n == "visited_wide") ix->visited_wide = value;
  else if (n == "entry_kernel") ix->entry_kernel = value;
  else if (n == "output_node_ids") ix->output_node_ids = value;
  else if (n == "overflow_list") ix->overflow_list = value;
  else if (n == "sorted_beam") ix->sorted_beam = value;
  else if (n == "sorted_beam_min") ix->sorted_beam_min = value;
  else if (n == "sorted_cand_lds") ix->sorted_cand_lds = value;
  else if (n == "sorted_tail_exact_pct") ix->sorted_tail_exact_pct = value;
  else if (n == "beam_registers") ix->beam_registers = value;
  else if (n == "sorted_variant") {
    if (value >= kNumVariants) return fail(FNV_ERR_INVALID, "sorted_variant must be -1 (adaptive) or 0..6");
    ix->sorted_variant = value;
  }
  else if (n == "visited_tag_bits") ix->visited_tag_bits = value;
  else if (n == "tune_layout") ix->tune_layout = value;
  else if (n == "shadow_exact") ix->shadow_exact = value;
  else if (n == "tie_replay") ix->tie_replay = value;
  else if (n == "tie_log_entries") {
    if (value > (1 << 20)) return fail(FNV_ERR_INVALID, "tie_log_entries must be at most 1048576 records (8 MB per query slot)");
    ix->tie_log_entries = value;
  }
  else if (n == "visited_direct") ix->visited_direct = value;  // (read per launch)
  else if (n == "host_zero_copy") ix->host_zero_copy = value;  // (read per host-buffer call)
  else if (n == "scan_segment_rows") ix->scan_segment_rows = value;  // (read per exhaustive launch)
  else if (n == "half_rows") ix->half_rows = value;  // (read per launch; the mirror's launches are another kernel's: measurements go)
  else return fail(FNV_ERR_INVALID, "unknown option: " + n);
  // What fnv_tune measured (kernel variant, LDS layout) stays valid across options that change neither the launch plan
  // nor the kernel choice: Index.h::addBatchDevice flips output_node_ids around every device build, and a tune costs
  // dozens of launches.  (output_node_ids is read per launch; shadow_exact per launch; tune_layout by fnv_tune itself.)
  const bool keeps_tuning = n == "output_node_ids" || n == "shadow_exact" || n == "tune_layout" || n == "visited_direct" || n == "host_zero_copy" || n == "scan_segment_rows";
  if (!keeps_tuning) {
    ix->options_version++;
    ix->tuner.clear();
    ix->layouts.clear();
    ix->sample_kernel = -1;
  }
  ix->tune_epoch++;  // (the second lane of the host entry point re-copies options and measurements)
  return FNV_OK;
}

// One batched search launch.
static int search_device_impl(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search, int num_initializations,
                              const SearchOutputs& out, void* hip_stream, const SearchOptions& opt = SearchOptions());

int fnv_search_batch_device(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search,
                            int num_initializations, float* d_out_dist, int32_t* d_out_labels,
                            int32_t* d_out_count, uint64_t* d_out_ndist, uint64_t* d_out_nhops, void* hip_stream) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  return search_device_impl(ix, d_queries, nq, K, ef_search, num_initializations,
                            SearchOutputs{d_out_dist, d_out_labels, d_out_count, d_out_ndist, d_out_nhops}, hip_stream);
}

// ---- launch configuration: launch_plan.hpp ---------------------------------------------------------------------

// While fnv_tune / fnv_index_insert_batch run, their thread holds the handle's host_mu and lane_mu AND every lane's host_mu
// (taken up front, so that no host-buffer search runs on a lane meanwhile: the existing lanes are locked, and none is created --
// a caller that wants one waits on lane_mu, holding nothing).  release_idle_lanes then frees with the locks it already
// has -- try_lock on a std::mutex the calling thread owns is undefined behaviour.
static thread_local const fnv_index_s* t_holds_lanes_of = nullptr;
struct HoldAllLanes {
  std::lock_guard<std::mutex> host_lock, no_new_lanes;
  std::vector<std::unique_lock<std::mutex>> lane_locks;
  const fnv_index_s* before;
  explicit HoldAllLanes(fnv_index_s* ix) : host_lock(ix->host_mu), no_new_lanes(ix->lane_mu), before(t_holds_lanes_of) {
    for (std::atomic<fnv_index_s*>& slot : ix->lanes)
      if (fnv_index_s* l = slot.load()) lane_locks.emplace_back(l->host_mu);
    t_holds_lanes_of = ix;
  }
  ~HoldAllLanes() { t_holds_lanes_of = before; }
};

static size_t free_lane_workspace(fnv_index_s* l) {  // the caller owns l->host_mu
  std::lock_guard<std::mutex> lk(l->mu);
  DeviceScope scope(l->device);
  const size_t freed = l->ws.release();
  l->ws_bytes = 0;
  return freed;
}

// Frees the launch workspace of every hidden lane of `ix` that is idle right now (nobody inside a call on it), except
// `keep`; returns the bytes released.  The caller holds ix->lane_mu.  `all_held`: it also holds every lane's host_mu.
static size_t release_idle_lanes_locked(fnv_index_s* ix, const fnv_index_s* keep, bool all_held = false) {
  size_t freed = 0;
  for (std::atomic<fnv_index_s*>& slot : ix->lanes) {
    fnv_index_s* l = slot.load();
    if (!l || l == keep) continue;
    if (all_held) {
      freed += free_lane_workspace(l);
      continue;
    }
    std::unique_lock<std::mutex> idle(l->host_mu, std::try_to_lock);
    if (idle.owns_lock()) freed += free_lane_workspace(l);
  }
  (void)hipGetLastError();
  return freed;
}
// ... for a caller that holds nothing of the lanes.  Never blocks: a lane in use, or a handle whose lanes are being created /
// held by another thread's fnv_tune, is left alone.  The lanes re-grow on their next call.
static size_t release_idle_lanes(fnv_index_s* ix, const fnv_index_s* keep) {
  if (t_holds_lanes_of == ix) return release_idle_lanes_locked(ix, keep, /*all_held=*/true);
  std::unique_lock<std::mutex> lanes_lock(ix->lane_mu, std::try_to_lock);
  if (!lanes_lock.owns_lock()) return 0;
  return release_idle_lanes_locked(ix, keep);
}

// HBM a launch of `nq` queries needs as per-slot workspace on a handle of this index (what grow_workspace grows).
static size_t launch_workspace_bytes(fnv_index_s* ix, uint64_t nq) {
  std::lock_guard<std::mutex> lock(ix->mu);
  const int per_cu = ix->plan.valid ? std::max(ix->plan.bpc, ix->plan.sbpc) : 32;  // (no plan yet: the hardware's 32 waves per CU)
  const uint64_t slots = std::min<uint64_t>(2 * nq, (uint64_t)per_cu * (uint64_t)ix->num_cus);  // (small launches: a shadow per query)
  // (the plan's own formula -- plan.sorted is unset while the plan runs the two-heap kernel only; no plan yet: the largest automatic log)
  const uint64_t log_entries = ix->plan.valid ? log_entries_for(ix, ix->plan.B) : (ix->tie_replay ? std::max<uint64_t>(16384u, (uint64_t)ix->tie_log_entries) : 0u);
  return (size_t)(slots * ((uint64_t)bitmap_words_of(ix) * 4 + (uint64_t)ovf_cap_of(ix) * 4 + (uint64_t)ix->spill_entries * 8 + log_entries * 8));
}

// The status word of a launch -> the call's result (`advice`: how each caller has always ended the message).
static int check_status(int32_t st, const char* advice = "raise the spill_entries option") {
  if (st == ST_CAND_OVERFLOW) return fail(FNV_ERR_CAPACITY, std::string("candidate heap overflowed its HBM spill area; ") + advice);
  return FNV_OK;
}
static int check_device_status(fnv_index_s* ix, const char* advice = "raise the spill_entries option") {  // (the stream has been waited for)
  int32_t st = 0;
  HIP_TRY(hipMemcpy(&st, ix->d_dispenser + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
  return check_status(st, advice);
}

// ---- one search launch, step by step (search_device_impl runs them in this order under the handle's mutex) -----------
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
  if (plan.valid && plan.B == B && plan.K == K && plan.capacity == ix->capacity && plan.options_version == ix->options_version && same_rows)
    return FNV_OK;
  plan = PlannedLaunch();
  const PlanRuntime rt{ix, row_geometry(ix), B, half_rows};
  LayoutChoice lc;  // a layout that fnv_tune measured for this beam width overrides the planner's rules (heap home, table size)
  if (auto it = ix->layouts.find(B); it != ix->layouts.end()) lc = it->second;
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
  plan.valid = true;
  return FNV_OK;
}

// (b) Which kernel variant the launch runs, and whether it is a sample for the adaptive choice (KernelChoice and the rules
// of each pick: launch_plan.hpp).
// (tests/launch_plan_harness.cpp, lph_launch, repeats the pinned branch below and search_device_impl's choice of bpc / LDS bytes /
// DIRECT form to shape launches on the CPU: a change here or there belongs in that twin as well)
static KernelChoice choose_kernel(fnv_index_s* ix, int B, uint64_t nq, int force_variant, bool filtered) {
  const LaunchPlan& plan = ix->plan;
  KernelChoice c = default_choice(ix, plan, nq, filtered);  // (what the plan prefers; below: what was pinned or measured)
  const bool multi_round = c.multi_round;
  const int pinned = force_variant >= 0 ? force_variant : (int)ix->sorted_variant;  // fnv_tune / "sorted_variant"
  const bool shadows_on = ix->shadow_exact != 0;
  const bool try_tail = ix->sorted_tail_exact_pct < 0;
  if (c.sorted && pinned >= 0) {
    c.variant = pinned_variant(pinned, multi_round, shadows_on);
  } else if (c.sorted && ix->sorted_beam == 2 && ix->is_lane) {
    // a hidden lane runs what its owner has measured (copied by sync_lane) and never explores or samples: a production
    // caller that happens to land on a lane must not pay for 3 x variants exploratory launches per lane
    if (auto it = ix->tuner.find(tuner_key(B, multi_round)); nq >= 2048 && it != ix->tuner.end())
      if (const int best = lane_variant(it->second, multi_round, try_tail, shadows_on); best >= 0) c.variant = best;
  } else if (c.sorted && ix->sorted_beam == 2) {
    if (ix->sample_kernel >= 0 && ix->launched && hipEventQuery(ix->ev1) == hipSuccess) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ix->ev0, ix->ev1) == hipSuccess && ms > 0.f) {
        Tuner& t = ix->tuner[ix->sample_B];
        const float per_q = ms / (float)ix->sample_nq;
        if (t.samples[ix->sample_kernel] == 0 || per_q < t.best[ix->sample_kernel]) t.best[ix->sample_kernel] = per_q;
        t.samples[ix->sample_kernel]++;
        ix->tune_epoch++;  // (lanes re-copy the measurements)
      }
      ix->sample_kernel = -1;
    }
    if (nq >= 2048) {
      Tuner& t = ix->tuner[tuner_key(B, multi_round)];
      // three samples each (the first launch of a kernel is a cold one; the best of the rest decides), then the fastest
      // (fnv_tune takes all the samples in one call, so that no caller's launch is an exploratory one)
      c.variant = owner_next_sample(t, multi_round, try_tail, shadows_on);
      c.exploratory = c.variant >= 0;
      if (c.variant < 0) c.variant = owner_final_variant(t, multi_round, try_tail, shadows_on);
      c.sample = t.samples[c.variant] < 4;
    }
  }
  c.sorted = c.variant != 0;  // (unchanged where nothing was pinned or measured: variant 1 of a merged-beam plan, else 0)
  if (c.variant >= 2) c.tail_pct = kTailPct[c.variant];
  return c;
}

// (c) The workspace, grown on demand and sized for whichever kernel keeps more slots resident.
static int grow_workspace(fnv_index_s* ix, uint32_t max_slots, uint64_t nq, bool sorted, bool done_flags, bool filtered) {
  const LaunchPlan& plan = ix->plan;
  int rc = FNV_OK;
  for (int attempt = 0; attempt < 2; attempt++) {
    rc = ix->ws.bitmap.grow((size_t)max_slots * plan.heaps.bitmap_words * 4, true);
    if (!rc) rc = ix->ws.ovf.grow((size_t)max_slots * plan.heaps.ovf_cap * 4);
    if (!rc) rc = ix->ws.spill.grow((size_t)max_slots * plan.heaps.spill_entries * 8);
    if (!rc && done_flags) rc = ix->d_done.grow((size_t)nq * 4);
    if (!rc && sorted) rc = ix->ws.tielog.grow((size_t)max_slots * plan.sorted.log_entries * 8);
    if (!rc && filtered) rc = ix->d_nodebits.grow((size_t)(ix->capacity + 31) / 32 * 4);
    ix->ws_bytes = ix->ws.bytes();
    // out of memory on the handle itself: the hidden lanes' idle workspaces go first, then once more (from inside fnv_tune /
    // fnv_index_insert_batch, which hold the lanes, with the locks already held: t_holds_lanes_of)
    if (rc != FNV_ERR_NO_DEVICE || attempt || ix->is_lane || ix->parent) break;
    (void)hipGetLastError();
    if (release_idle_lanes(ix, nullptr) == 0) break;
  }
  return rc;
}

// (d) Small launches on small indexes run the kernel's DIRECT form on a bitmap of all node ids: lay_out_direct (launch_plan.hpp).

// ---- grouped filters: the node bitmaps of a launch with one filter per query ---------------------------------------
// ws.rows for the n_filters + 2 rows of a grouped launch.  The one allocation of the library whose size the caller's
// n_filters decides: its failure says how much that was, and a host-buffer caller's lane is admitted with it counted.
static size_t filter_rows_bytes(const fnv_index_s* ix, const SearchFilter& f) {
  return (size_t)f.rows() * (size_t)((ix->capacity + 31) / 32) * 4;
}
static int grow_filter_rows(fnv_index_s* ix, const SearchFilter& f) {
  const size_t need = filter_rows_bytes(ix, f);
  const int rc = ix->ws.rows.grow(need);
  ix->ws_bytes = ix->ws.bytes();
  if (rc == FNV_OK) return FNV_OK;
  (void)hipGetLastError();
  return fail(FNV_ERR_RUNTIME, "the filter rows of this launch need " + std::to_string(need) + " bytes of device memory (" +
                                   std::to_string(f.rows()) + " node bitmaps), which could not be allocated");
}
// ... filled from the filter table and the labels as they are now; row_count (null: not wanted, else zero): nodes set per row
static int launch_filter_rows(fnv_index_s* ix, const SearchFilter& f, uint64_t live, hipStream_t stream, uint32_t* row_count) {
  const uint64_t words = (ix->capacity + 31) / 32;
  const dim3 grid((unsigned)((words * 32 + 255) / 256), (unsigned)std::min<uint64_t>(f.rows(), 65535));
  hipLaunchKernelGGL(node_filter_table_kernel, grid, dim3(256), 0, stream, (const int32_t*)ix->d_labels, live, words, f.bits, f.stride,
                     f.n_bits, (uint32_t)f.n_filters, ix->ws.rows.as<uint32_t>(), row_count);
  HIP_TRY(hipGetLastError());
  return FNV_OK;
}
// One filter for the launch: the label bitmap -> d_nodebits, by the labels as they are now (after reorder(), device builds ...)
static int launch_node_filter(fnv_index_s* ix, const SearchFilter& f, uint64_t live, hipStream_t stream) {
  const uint64_t words = (ix->capacity + 31) / 32;
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
static void record_launch(fnv_index_s* ix, hipStream_t stream, uint64_t grid, uint64_t block, uint64_t lds, uint64_t g3, uint64_t g4,
                          uint64_t g5, uint64_t mode, uint64_t g7) {
  ix->last_stream = stream;
  ix->launched = true;
  if (!ix->is_lane) ix->last_served = nullptr;  // the handle's own launch is its most recent one
  const uint64_t geom[8] = {grid, block, lds, g3, g4, g5, mode, g7};
  for (int i = 0; i < 8; i++) ix->geom[i] = geom[i];
}
// The grouping arrays of a grouped scan (scan.hpp's group_* kernels), as uint32 offsets into one buffer.
struct GroupArrays {
  size_t query_row, perm, counts, cursor, row_count, slot_start, tile_start, tiles, bytes;
  GroupArrays(uint64_t nq, uint64_t rows, uint64_t tile_bound) {
    query_row = 0;
    perm = query_row + nq;
    counts = perm + nq;  // counts | cursor | row_count: cleared by one memset
    cursor = counts + rows;
    row_count = cursor + rows;
    slot_start = row_count + rows;
    tile_start = slot_start + rows + 1;
    tiles = tile_start + rows + 1;
    bytes = (tiles + 3 * tile_bound) * 4;
  }
};

// ---- exhaustive search (scan.hpp): the launch ---------------------------------------------------------------------
// How a launch of `nq` queries for K results is cut up: queries per tile (as many as a block's LDS budget holds next to their
// result lists, at most 32), row segments (enough blocks to fill the device, at most 64 and at most what keeps the partial
// lists within 256 MB; or what "scan_segment_rows" asks for).
constexpr uint32_t kScanLdsBudget = 20u << 10;  // per block: eight blocks per CU = two wavefronts per SIMD
constexpr uint32_t kScanMaxTile = 32, kScanMaxSegments = 64, kScanForcedSegments = 1024;
constexpr uint64_t kScanPartialBudget = 256ull << 20;
struct ScanShape {
  uint32_t tile, tiles, segments, lds;
};
// `filter_rows` != 0: a grouped launch over that many filter rows -- the id queue comes out of the block's LDS budget, and
// `tiles` is the bound on the data-dependent tile count that the launch covers (scan_select.hpp, group_tile_bound).
static ScanShape scan_shape(const fnv_index_s* ix, const RowGeometry& g, uint64_t nq, int K, uint64_t live, uint64_t filter_rows = 0) {
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

static int scan_device_impl(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, const SearchOutputs& out, void* hip_stream,
                            const SearchOptions& opt) {
  int rc;
  if (K < 1 || K > SCAN_MAX_K) return fail(FNV_ERR_INVALID, "K of an exhaustive search must be between 1 and 1024");
  if (!batch_to_launch(d_queries, nq, out, &rc)) return rc;
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  hipStream_t stream = (hipStream_t)hip_stream;
  const SearchFilter* filter = opt.filter;
  const uint64_t live = ix->parent ? ix->parent->n_nodes.load() : ix->n_nodes.load();  // a view follows its source's growth
  const RowGeometry g = row_geometry(ix);
  const bool grouped = filter && filter->grouped;
  const ScanShape shape = scan_shape(ix, g, nq, K, live, grouped ? filter->rows() : 0);
  if (shape.lds > 160u * 1024u) return fail(FNV_ERR_INVALID, "rows are too long for an exhaustive search (one query and its list must fit in LDS)");
  const scan_fn kern = kernel_table(ix->dtype, ix->metric).flat[g.cfg][g.full];
  const scan_grouped_fn kern_g = kernel_table(ix->dtype, ix->metric).flat_g[g.cfg][g.full];
  const GroupArrays ga(nq, grouped ? filter->rows() : 0, shape.tiles);

  rc = ix->ws.scan.grow((size_t)nq * shape.segments * (size_t)K * 8);
  if (!rc && grouped) rc = grow_filter_rows(ix, *filter);
  if (!rc && grouped) rc = ix->ws.group.grow(ga.bytes);
  if (!rc && filter && !grouped) rc = ix->d_nodebits.grow((size_t)(ix->capacity + 31) / 32 * 4);
  if (!rc && filter && !grouped) rc = ix->d_scanids.grow(16 + (size_t)ix->capacity * 4);
  ix->ws_bytes = ix->ws.bytes();
  if (rc) return rc;

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

  HIP_TRY(hipMemsetAsync(ix->d_dispenser, 0, 16 * sizeof(uint32_t), stream));  // (the status word: this path never sets it)
  GroupedScanParams gp;
  memset(&gp, 0, sizeof(gp));
  if (grouped) {  // the filter table -> this handle's node bitmaps and their popcounts; the queries grouped by row into tiles
    uint32_t* const w = ix->ws.group.as<uint32_t>();
    const uint32_t rows = (uint32_t)filter->rows(), n = (uint32_t)nq;
    HIP_TRY(hipMemsetAsync(w + ga.counts, 0, (size_t)3 * rows * 4, stream));  // counts | cursor | row_count
    rc = launch_filter_rows(ix, *filter, live, stream, w + ga.row_count);
    if (rc) return rc;
    hipLaunchKernelGGL(group_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, filter->query_filter, n,
                       (uint32_t)filter->n_filters, w + ga.query_row, w + ga.counts);
    hipLaunchKernelGGL(group_prefix_kernel, dim3(1), dim3(256), 0, stream, (const uint32_t*)(w + ga.counts), rows, shape.tile,
                       w + ga.slot_start, w + ga.tile_start);
    hipLaunchKernelGGL(group_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const uint32_t*)(w + ga.query_row), n,
                       (const uint32_t*)(w + ga.slot_start), w + ga.cursor, w + ga.perm);
    hipLaunchKernelGGL(group_tiles_kernel, dim3((shape.tiles + 255) / 256), dim3(256), 0, stream, (const uint32_t*)(w + ga.slot_start),
                       (const uint32_t*)(w + ga.tile_start), rows, shape.tile, shape.tiles, (GroupTile*)(w + ga.tiles));
    HIP_TRY(hipGetLastError());
    gp.node_bits = ix->ws.rows.as<uint32_t>();
    gp.tiles = (const GroupTile*)(w + ga.tiles);
    gp.perm = w + ga.perm;
    gp.query_row = w + ga.query_row;
    gp.row_count = w + ga.row_count;
    gp.row_words = (uint32_t)((ix->capacity + 31) / 32);
    gp.live_words = (uint32_t)((live + 31) / 32);
  } else if (filter) {  // the label bitmap -> this handle's node bitmap -> the list of allowed node ids
    uint32_t* const ids = ix->d_scanids.as<uint32_t>();
    rc = launch_node_filter(ix, *filter, live, stream);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ids, 0, 16, stream));
    hipLaunchKernelGGL(exhaustive_compact_kernel, dim3((unsigned)((live + 255) / 256)), dim3(256), 0, stream,
                       (const uint32_t*)ix->d_nodebits.as<uint32_t>(), live, ids + 4, ids);
    HIP_TRY(hipGetLastError());
    p.cand_ids = ids + 4;
    p.cand_count = ids;
  }
  ix->sample_kernel = -1;  // ev0 / ev1 no longer bracket a graph-search launch: a pending sample of the adaptive choice is dropped
  HIP_TRY(hipEventRecord(ix->ev0, stream));
  const uint32_t merge_lds = 3u * (uint32_t)K * 8u;
  if (grouped) {
    gp.s = p;
    HIP_TRY(raise_lds_limit((const void*)kern_g, ix->device, shape.lds));
    hipLaunchKernelGGL(kern_g, dim3(shape.tiles * shape.segments), dim3(WAVE), shape.lds, stream, gp);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(exhaustive_merge_grouped_kernel, dim3((unsigned)nq), dim3(WAVE), merge_lds, stream, gp);
  } else {
    HIP_TRY(raise_lds_limit((const void*)kern, ix->device, shape.lds));
    hipLaunchKernelGGL(kern, dim3(shape.tiles * shape.segments), dim3(WAVE), shape.lds, stream, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(exhaustive_merge_kernel, dim3((unsigned)nq), dim3(WAVE), merge_lds, stream, p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ix->ev1, stream));
  // (mode 3 of fnv_last_launch_geometry: the exhaustive scan; its grouped form: queries per tile, entries of the id queue, row segments)
  record_launch(ix, stream, (uint64_t)shape.tiles * shape.segments, WAVE, shape.lds, grouped ? shape.tile : 0, grouped ? SCAN_QUEUE_IDS : 0,
                grouped ? shape.segments : 0, 3, 0);
  return FNV_OK;
}

static int search_device_impl(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search, int num_initializations,
                              const SearchOutputs& out, void* hip_stream, const SearchOptions& opt) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (opt.exhaustive) return scan_device_impl(ix, d_queries, nq, K, out, hip_stream, opt);
  // Index.h:847-849
  if (num_initializations <= 0) return fail(FNV_ERR_INVALID, "num_initializations must be greater than 0.");
  if (K <= 0 || ef_search <= 0) return fail(FNV_ERR_INVALID, "K and ef_search must be positive");
  int rc;
  if (!batch_to_launch(d_queries, nq, out, &rc)) return rc;
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  hipStream_t stream = (hipStream_t)hip_stream;
  const SearchFilter* filter = opt.filter;

  const int B = std::max(ef_search, K);  // Index.h:392
  const uint64_t live = ix->parent ? ix->parent->n_nodes.load() : ix->n_nodes.load();  // a view follows its source's growth
  // The half-width mirror (half_rows.hpp): its state is the source's, read at every launch.  Launches with and without it run
  // different kernels, so what was measured in the other mode (kernel variant, LDS layout) is discarded with the plan.
  const bool half_rows = half_rows_usable(ix, live);
  if (ix->measured_half >= 0 && ix->measured_half != (int)half_rows) {
    ix->tuner.clear();
    ix->layouts.clear();
    ix->sample_kernel = -1;
    ix->tune_epoch++;
    ix->plan.valid = false;
  }
  ix->measured_half = (int)half_rows;
  rc = ensure_plan(ix, B, K, half_rows);
  if (rc) return rc;
  PlannedLaunch& plan = ix->plan;
  if (filter && !plan.fkern.fn) {
    plan.fkern = bind_search_kernel(ix, row_geometry(ix), KERNEL_FILTERED, false, B, half_rows);
    HIP_TRY(raise_lds_limit((const void*)plan.fkern.fn, ix->device, plan.lds));
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)plan.fkern.fn, WAVE, plan.lds) != hipSuccess) n = 0;
    plan.fbpc = std::max(1, std::min(plan.bpc, n));
  }
  const KernelChoice c = choose_kernel(ix, B, nq, opt.force_variant, filter != nullptr);
  const bool sorted = c.sorted;
  const int bpc = sorted ? plan.sbpc : opt.filter ? plan.fbpc : plan.bpc;
  uint32_t lds_bytes = sorted ? plan.slds : plan.lds;
  // (shadow mode, tail shadows, the grid: launch_shape, launch_plan.hpp)
  const LaunchShape shape = launch_shape(ix, plan, c, bpc, nq, num_initializations, live);
  const bool small_launch = shape.small_launch, shadow = shape.shadow;
  const uint32_t nslots = shape.nslots, tail_shadows = shape.tail_shadows;

  const bool grouped = filter && filter->grouped;
  rc = grow_workspace(ix, shape.max_slots, nq, sorted, shadow || tail_shadows, filter != nullptr && !grouped);
  if (!rc && grouped) rc = grow_filter_rows(ix, *filter);
  if (rc) return rc;

  SearchParams p = sorted ? plan.sorted : plan.heaps;
  const bool direct = sorted && small_launch && lay_out_direct(ix, p, &lds_bytes, bpc, nslots);

  // (e) the per-call fields, and the launch
  const BoundKernel& kern = filter ? plan.fkern : !sorted ? plan.kern : direct ? plan.skern_direct : plan.skern;
  p.labels = (opt.node_ids || ix->output_node_ids != 0) ? nullptr : ix->d_labels;  // ("output_node_ids": read under the handle's mutex)
  p.queries = (const uint8_t*)d_queries;
  p.out_dist = out.dist;
  p.out_labels = out.labels;
  p.out_count = out.count;
  p.out_ndist = out.ndist;
  p.out_nhops = out.nhops;
  p.n_nodes = live;
  p.nq = (uint32_t)nq;
  p.scan_step = shape.scan_step;  // Index.h:851-861
  p.n_scan = shape.n_scan;
  p.ovf_bitmap = ix->ws.bitmap.as<uint32_t>();
  p.ovf_glist = ix->ws.ovf.as<uint32_t>();
  p.cand_spill = ix->ws.spill.as<unsigned long long>();
  p.tie_log = ix->ws.tielog.as<unsigned long long>();
  if (!sorted) p.log_entries = 0u;
  p.dispenser = ix->d_dispenser;
  p.status = (int32_t*)(ix->d_dispenser + 1);
  p.host_status = opt.host_status;
  p.redo_count = ix->d_dispenser + 3;  // [3] queries searched exactly after a tie, [4..7] by reason
  p.phase_cycles = ix->d_phase;
  p.tail_exact = shape.tail_exact;

  HIP_TRY(hipMemsetAsync(ix->d_dispenser, 0, 16 * sizeof(uint32_t), stream));
  if (grouped) {  // the filter table -> this handle's node bitmaps; every query reads its own row
    rc = launch_filter_rows(ix, *filter, live, stream, nullptr);
    if (rc) return rc;
    p.node_bits = ix->ws.rows.as<uint32_t>();
    p.query_filter = filter->query_filter;
    p.filter_words = (uint32_t)((ix->capacity + 31) / 32);
    p.n_filters = (uint32_t)filter->n_filters;
  } else if (filter) {
    rc = launch_node_filter(ix, *filter, live, stream);
    if (rc) return rc;
    p.node_bits = ix->d_nodebits.as<uint32_t>();
  }
  HIP_TRY(hipEventRecord(ix->ev0, stream));
  if (ix->entry_kernel && !ix->tail_bytes) {  // (split rows: K0's LDS tiles hold one table's rows; the in-kernel scan serves them)
    // K0: one pass over the shared entry-scan nodes for the whole batch (LDS-staged), same stream
    rc = ix->d_entry.grow((size_t)nq * 8);
    if (rc) return rc;
    p.entry_node_out = ix->d_entry.as<uint32_t>();
    p.entry_dist_out = (float*)(ix->d_entry.as<uint8_t>() + (size_t)nq * 4);
    p.vectors = ix->d_vectors;  // (K0 stages float32 rows in LDS whichever table the search kernel reads)
    p.row_bytes = ix->row_bytes;
    p.scan_tile_stride = p.row_bytes + 16;
    const uint32_t fixed = SCAN_WAVES * p.q_chunks * 16 + SCAN_QPB * 8;
    p.scan_tile_rows = std::max<uint32_t>(1, std::min<uint32_t>(p.n_scan, (64u * 1024u) / p.scan_tile_stride));
    const uint32_t scan_lds = fixed + p.scan_tile_rows * p.scan_tile_stride;
    kernel_fn scan = pick_scan_kernel(ix->dtype, ix->metric, plan.cfg, plan.full);
    HIP_TRY(raise_lds_limit((const void*)scan, ix->device, scan_lds));
    hipLaunchKernelGGL(scan, dim3((unsigned)((nq + SCAN_QPB - 1) / SCAN_QPB)), dim3(SCAN_WAVES * WAVE), scan_lds, stream, p);
    HIP_TRY(hipGetLastError());
    p.entry_node = p.entry_node_out;
    p.entry_dist = p.entry_dist_out;
  }
  if (tail_shadows) {  // the queries, then exact shadows of the last `tail_shadows` of them (pulled by slots that would go idle)
    HIP_TRY(hipMemsetAsync(ix->d_done.ptr, 0, (size_t)nq * 4, stream));
    p.shadow_base = (uint32_t)nq;
    p.done_flags = ix->d_done.as<uint32_t>();
    p.nq = (uint32_t)(nq + tail_shadows);
    p.tail_exact = 0u;
  }
  if (shadow) {  // from here on the launch has 2 nq work items: the queries, then their exact shadows
    HIP_TRY(hipMemsetAsync(ix->d_done.ptr, 0, (size_t)nq * 4, stream));
    p.shadow_base = (uint32_t)nq;
    p.done_flags = ix->d_done.as<uint32_t>();
    p.nq = (uint32_t)(2 * nq);
    p.tail_exact = 0u;
  }
  p.vectors = kern.rows;  // the kernel and the table it reads: one BoundKernel
  p.row_bytes = kern.stride;
  HIP_TRY(raise_lds_limit((const void*)kern.fn, ix->device, lds_bytes));
  hipLaunchKernelGGL(kern.fn, dim3(nslots), dim3(WAVE), lds_bytes, stream, p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ix->ev1, stream));
  // (f) what the launch was: for the adaptive choice's next harvest, and for the fnv_last_* calls
  ix->sample_kernel = c.sample ? c.variant : -1;
  ix->sample_B = tuner_key(B, c.multi_round);
  ix->sample_nq = nq;
  ix->last_variant = sorted ? std::max(c.variant, 1) : 0;
  ix->last_exploratory = c.exploratory;
  if (c.exploratory) ix->explored_launches++;
  ix->last_shadow = shadow;
  ix->last_half = kern.half_rows;
  record_launch(ix, stream, nslots, WAVE, lds_bytes, (uint64_t)bpc, p.vis_slots, p.cand_slots, (uint64_t)(sorted ? plan.mode : MODE_HEAPS),
                p.tail_exact);
  return FNV_OK;
}

int fnv_search_status(fnv_index_t ix) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (!ix->launched) return FNV_OK;
  ON_DEVICE(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->last_stream));
  return check_device_status(ix);
}

static uint64_t now_ns() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Host-buffer search in two halves, so that several devices can be kept busy by one caller: enqueue (H2D of the
// queries, the search launch, D2H of the results -- all asynchronous on the index's own stream; the caller holds
// ix->host_mu) and finish (wait, report a capacity error).
// `host_filter` (filtered search): the label bitmap in host memory; it is staged into this handle's HBM first.
static int search_host_enqueue(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search,
                               int num_initializations, const SearchOutputs& user, const SearchFilter* host_filter = nullptr,
                               bool exhaustive = false) {
  ON_DEVICE(ix->device);
  SearchFilter dev_filter{nullptr, 0};
  SearchOptions opt;
  opt.exhaustive = exhaustive;
  const bool grouped = host_filter && host_filter->grouped;
  if (grouped) {  // the filter table (its rows `stride` apart, as the caller has them), then query_filter, through d_allowed
    const size_t row_bytes = (size_t)((host_filter->n_bits + 7) / 8);
    const size_t tbytes = host_filter->n_filters && row_bytes ? (size_t)(host_filter->n_filters - 1) * host_filter->stride + row_bytes : 0;
    const size_t qf_off = (tbytes + 15) & ~(size_t)15;
    {
      std::lock_guard<std::mutex> lock(ix->mu);
      int rc = ix->d_allowed.grow(qf_off + (size_t)nq * 4);
      if (rc) return rc;
    }
    uint8_t* const base = ix->d_allowed.as<uint8_t>();
    if (tbytes) HIP_TRY(hipMemcpyAsync(base, host_filter->bits, tbytes, hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemcpyAsync(base + qf_off, host_filter->query_filter, (size_t)nq * 4, hipMemcpyHostToDevice, ix->stream));
    dev_filter = *host_filter;
    dev_filter.bits = tbytes ? base : nullptr;
    dev_filter.query_filter = (const int32_t*)(base + qf_off);
    opt.filter = &dev_filter;
  } else if (host_filter) {
    const size_t fbytes = (size_t)((host_filter->n_bits + 7) / 8);
    if (fbytes) {
      {
        std::lock_guard<std::mutex> lock(ix->mu);
        int rc = ix->d_allowed.grow(fbytes);
        if (rc) return rc;
      }
      HIP_TRY(hipMemcpyAsync(ix->d_allowed.ptr, host_filter->bits, fbytes, hipMemcpyHostToDevice, ix->stream));
      dev_filter.bits = ix->d_allowed.as<uint8_t>();
    }
    dev_filter.n_bits = host_filter->n_bits;
    opt.filter = &dev_filter;
  }
  const size_t qbytes = (size_t)nq * ix->dim * dtype_size(ix->dtype);
  size_t obytes = 0;
  (void)lay_out_slab(nullptr, nq, K, &obytes);  // one output slab, on the device and in pinned memory
  // Small batches (a single query above all) go through one pinned host buffer: one H2D copy, one D2H copy of the
  // whole slab plus the status word, no pageable-memory copies (each of those synchronises) -- the host side of a
  // one-query search drops from ~10 driver round trips to 4 asynchronous calls and one wait.
  const size_t qoff = 0, ooff = (qbytes + 63) & ~(size_t)63, soff = ooff + ((obytes + 63) & ~(size_t)63);
  const bool pinned = soff + 64 <= (1u << 20);
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    int rc = ix->d_q.grow(qbytes);
    if (!rc) rc = ix->d_out.grow(obytes);
    if (rc) return rc;
    if (pinned && !ix->h_pin) HIP_TRY(hipHostMalloc(&ix->h_pin, 1u << 20, hipHostMallocDefault));
    // larger batches (round 4): the queries still go in as one pageable copy, but the five result arrays come back as ONE
    // slab into pinned memory (grown on demand, up to 256 MB of results) and are scattered by the CPU -- five pageable
    // device-to-host copies each synchronise with the runtime's staging
    const size_t res_need = ((obytes + 63) & ~(size_t)63) + 64;
    // best effort: pinned memory is commonly capped (ulimit -l, containers) -- without the slab the five pageable
    // copies below still work
    if (!pinned && res_need <= (256u << 20) && ix->h_res.grow(res_need, false, res_need / 4) != FNV_OK) {
      ix->h_res.release();
      (void)hipGetLastError();
    }
  }
  const bool pinned_results = !pinned && ix->h_res.ptr && ((obytes + 63) & ~(size_t)63) + 64 <= ix->h_res.bytes;
  const SearchOutputs dev_slab = lay_out_slab(ix->d_out.ptr, nq, K);
  ix->pin = PinnedCall();
  // A caller whose arrays are ALREADY pinned (hipHostMalloc / hipHostRegister / torch pin_memory) needs no staging at any batch
  // size (round 6): the kernel reads the queries from and writes the results into the caller's own memory -- each query
  // crosses PCIe once while the launch runs, nothing is copied before or after it.  (Batches that fit the staging buffer take
  // the path below whatever their memory is: one attribute query per array costs more than their copies.)
  if (!pinned && ix->host_zero_copy != 0 && !grouped) {  // (grouped calls: always the staged copies)
    auto device_view = [](const void* host) -> void* {
      if (!host) return nullptr;
      hipPointerAttribute_t a;
      if (hipPointerGetAttributes(&a, host) != hipSuccess || a.type != hipMemoryTypeHost || !a.devicePointer) {
        (void)hipGetLastError();  // (pageable memory is "invalid value" to the runtime)
        return nullptr;
      }
      return a.devicePointer;
    };
    void* dq = device_view(queries);
    void* dd = dq ? device_view(user.dist) : nullptr;
    void* dl = dd ? device_view(user.labels) : nullptr;
    void* dc = user.count ? device_view(user.count) : nullptr;
    void* dn = user.ndist ? device_view(user.ndist) : nullptr;
    void* dh = user.nhops ? device_view(user.nhops) : nullptr;
    if (dq && dd && dl && (!user.count || dc) && (!user.ndist || dn) && (!user.nhops || dh)) {
      int rc0 = search_device_impl(ix, dq, nq, K, ef_search, num_initializations,
                                   SearchOutputs{(float*)dd, (int32_t*)dl, (int32_t*)dc, (uint64_t*)dn, (uint64_t*)dh}, ix->stream, opt);
      if (rc0) return rc0;
      ix->t_enqueue_ns = now_ns();
      return FNV_OK;  // (search_host_finish: wait + the launch's status word)
    }
  }
  // ZERO-COPY (round 6, "host_zero_copy" = the largest batch that takes it; default: every call that fits the 1 MB pinned
  // staging buffer): the kernel reads the queries straight from the pinned buffer and writes results, counters and its error
  // flag straight into it -- three stream operations (one copy in, two out) fewer per call; each query is read over PCIe
  // once (when it is staged), its K results are posted writes.  Measured on 1M x 128 (profiles/r6_host_zero_copy.txt): kernel
  // time +0-3 %, wall time of a call -13 ... -40 us at every batch size from 1 to 1024 queries (one query: 0.157 -> 0.143 ms
  // at ef=50; 64: 0.24-0.26 -> 0.215 ms; 1024: 0.446 -> 0.405 ms).
  uint8_t* h = (uint8_t*)ix->h_pin;  // (small batches)
  if (pinned && nq <= (uint64_t)ix->host_zero_copy && !grouped) {
    memcpy(h + qoff, queries, qbytes);
    *(int32_t*)(h + soff) = ST_OK;
    const SearchOutputs pin_slab = lay_out_slab(h + ooff, nq, K);
    opt.host_status = (int32_t*)(h + soff);
    int rc0 = search_device_impl(ix, h + qoff, nq, K, ef_search, num_initializations, pin_slab, ix->stream, opt);
    if (rc0) return rc0;
    ix->t_enqueue_ns = now_ns();
    ix->pin.arm(pin_slab, opt.host_status, user, nq, K);
    return FNV_OK;
  }
  if (pinned) {
    memcpy(h + qoff, queries, qbytes);
    HIP_TRY(hipMemcpyAsync(ix->d_q.ptr, h + qoff, qbytes, hipMemcpyHostToDevice, ix->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(ix->d_q.ptr, queries, qbytes, hipMemcpyHostToDevice, ix->stream));
  }
  int rc = search_device_impl(ix, ix->d_q.ptr, nq, K, ef_search, num_initializations, dev_slab, ix->stream, opt);
  if (rc) return rc;
  ix->t_enqueue_ns = now_ns();
  if (pinned || pinned_results) {  // the whole slab and the status word into pinned memory; search_host_finish scatters them
    uint8_t* slab = pinned ? h + ooff : ix->h_res.as<uint8_t>();
    int32_t* status = (int32_t*)(pinned ? h + soff : slab + ((obytes + 63) & ~(size_t)63));
    HIP_TRY(hipMemcpyAsync(slab, ix->d_out.ptr, obytes, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipMemcpyAsync(status, ix->d_dispenser + 1, sizeof(int32_t), hipMemcpyDeviceToHost, ix->stream));
    ix->pin.arm(lay_out_slab(slab, nq, K), status, user, nq, K);
    return FNV_OK;
  }
  HIP_TRY(hipMemcpyAsync(user.dist, dev_slab.dist, (size_t)nq * K * 4, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipMemcpyAsync(user.labels, dev_slab.labels, (size_t)nq * K * 4, hipMemcpyDeviceToHost, ix->stream));
  if (user.count) HIP_TRY(hipMemcpyAsync(user.count, dev_slab.count, (size_t)nq * 4, hipMemcpyDeviceToHost, ix->stream));
  if (user.ndist) HIP_TRY(hipMemcpyAsync(user.ndist, dev_slab.ndist, (size_t)nq * 8, hipMemcpyDeviceToHost, ix->stream));
  if (user.nhops) HIP_TRY(hipMemcpyAsync(user.nhops, dev_slab.nhops, (size_t)nq * 8, hipMemcpyDeviceToHost, ix->stream));
  return FNV_OK;
}

static int search_host_finish(fnv_index_t ix) {
  ON_DEVICE(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->t_complete_ns = now_ns();
  PinnedCall& c = ix->pin;
  if (!c.active) return fnv_search_status(ix);
  c.active = false;
  const size_t nk = (size_t)c.nq * c.K * 4;
  memcpy(c.user.dist, c.slab.dist, nk);
  memcpy(c.user.labels, c.slab.labels, nk);
  if (c.user.count) memcpy(c.user.count, c.slab.count, (size_t)c.nq * 4);
  if (c.user.ndist) memcpy(c.user.ndist, c.slab.ndist, (size_t)c.nq * 8);
  if (c.user.nhops) memcpy(c.user.nhops, c.slab.nhops, (size_t)c.nq * 8);
  return check_status(*c.status);
}

static int check_search_args(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search,
                             int num_initializations, const float* out_dist, const int32_t* out_labels) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (num_initializations <= 0) return fail(FNV_ERR_INVALID, "num_initializations must be greater than 0.");
  if (K <= 0 || ef_search <= 0) return fail(FNV_ERR_INVALID, "K and ef_search must be positive");
  if (nq && (!queries || !out_dist || !out_labels)) return fail(FNV_ERR_INVALID, "null buffer");
  return FNV_OK;
}

// Hidden lane `which` (1 ... kMaxLanes - 1) of a handle (fnv_index_s::lanes): created on first contention, by a caller that
// holds ix->lane_mu and has been admitted (a lane costs a stream, two events, a dispenser and 1 MB of pinned host memory).
static fnv_index_s* create_lane_locked(fnv_index_t ix, int which) {
  fnv_index_t v = nullptr;
  if (fnv_index_view(ix, &v) != FNV_OK) return nullptr;
  v->is_lane = true;
  ix->lanes[which] = v;
  return v;
}
// The lane answers exactly like its owner: same options, same measured layouts and kernel choice (copied when they changed).
static void sync_lane(fnv_index_t ix, fnv_index_s* lane) {
  std::lock_guard<std::mutex> l1(ix->mu);
  std::lock_guard<std::mutex> l2(lane->mu);
  if (lane->lane_epoch == ix->tune_epoch && lane->lane_options == ix->options_version) return;
  static_cast<IndexOptions&>(*lane) = static_cast<const IndexOptions&>(*ix);
  lane->layouts = ix->layouts;
  lane->tuner = ix->tuner;
  lane->sample_kernel = -1;
  lane->options_version++;
  lane->plan.valid = false;
  lane->lane_epoch = ix->tune_epoch;
  lane->lane_options = ix->options_version;
}

// Large host-buffer searches take the plain path above: one pageable copy in, one launch, copies out (0.80-0.93 of the
// device-resident rate).  Round 4 tried to hide the copies inside one call, twice, and measured both slower:
// chunks of the batch as separate copy + launch + copy pipelines on two streams (every chunk pays a whole query latency
// and its own stragglers: 2.4-3.3 ms against 1.28 ms), and ONE launch that starts before its queries are there -- reading
// them from pinned host memory behind a gate word, results written straight back (every touch of host memory from a
// running wave costs microseconds: 1.7-2.6 ms).  Neither is in the tree.
static int search_batch_host(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                             const SearchOutputs& out, const SearchFilter* host_filter, bool exhaustive = false) {
  int rc = check_search_args(ix, queries, nq, K, ef_search, num_initializations, out.dist, out.labels);
  if (rc || nq == 0) return rc;
  // one caller at a time per lane (a lane's staging areas, stream and workspace are its caller's for the whole call); a
  // caller that finds the handle busy takes the second lane, a further ones take more lanes when their batches are small, else wait for the first
  fnv_index_s* lane = ix;
  std::unique_lock<std::mutex> host_lock(ix->host_mu, std::try_to_lock);
  if (!host_lock.owns_lock() && !ix->parent) {
    // A lane is taken only if the HBM its launch workspace needs fits the budget for all hidden lanes together (round 5;
    // fnv_index_s: an eighth of the device's memory) -- measured on 1M x 128 (r4_run18): 7.8 / 10.4 / 11.2 / 11.5 M queries/s
    // from 1 / 2 / 3 / 4 caller threads on four lanes; at 50M nodes one full-grid lane is 19 GB and the second does not fit.
    // Admission, reservation and creation happen under lane_mu: two concurrent callers cannot both pass the budget
    // test, and a batch that fits no lane (large index, FLATNAV_LANE_BUDGET_MB=0) creates none.  Lock order: lane_mu, then a
    // lane's host_mu by try_lock only (fnv_tune takes lane_mu, then every lane's host_mu, blocking).
    const size_t need = launch_workspace_bytes(ix, nq) + (host_filter && host_filter->grouped ? filter_rows_bytes(ix, *host_filter) : 0);
    if (need <= ix->lane_budget_bytes) {
      std::lock_guard<std::mutex> admission(ix->lane_mu);
      for (int which = 1; which < fnv_index_s::kMaxLanes; which++) {
        fnv_index_s* l = ix->lanes[which].load();
        std::unique_lock<std::mutex> lock2;
        if (l) {
          lock2 = std::unique_lock<std::mutex>(l->host_mu, std::try_to_lock);
          if (!lock2.owns_lock()) continue;
        }
        auto others = [&]() {
          size_t sum = 0;
          for (int o = 1; o < fnv_index_s::kMaxLanes; o++)
            if (fnv_index_s* other = o != which ? ix->lanes[o].load() : nullptr) sum += other->ws_bytes.load();
          return sum;
        };
        const size_t mine = std::max<size_t>(l ? l->ws_bytes.load() : 0, need);
        if (others() + mine > ix->lane_budget_bytes) (void)release_idle_lanes_locked(ix, l);  // idle lanes give their room back first
        if (others() + mine > ix->lane_budget_bytes) {
          if (!l) break;  // no further lane would fit either
          continue;       // does not fit: not this lane
        }
        if (!l) {
          l = create_lane_locked(ix, which);
          if (!l) break;
          lock2 = std::unique_lock<std::mutex>(l->host_mu);
        }
        l->ws_bytes = mine;  // the reservation: visible to the next caller's budget test before lane_mu is released
        lane = l;
        host_lock = std::move(lock2);
        break;
      }
    }
  }
  if (!host_lock.owns_lock()) host_lock = std::unique_lock<std::mutex>(ix->host_mu);
  if (lane != ix) sync_lane(ix, lane);
  rc = search_host_enqueue(lane, queries, nq, K, ef_search, num_initializations, out, host_filter, exhaustive);
  if (rc == FNV_ERR_NO_DEVICE && lane != ix) {
    // a lane could not get its workspace (another copy of the per-slot bitmaps and spill areas: 19 GB at 50M nodes): the
    // call waits for the handle's own lane instead, like any caller did before there were lanes
    (void)hipGetLastError();
    host_lock.unlock();  // (never hold a lane while waiting for the handle: fnv_tune takes them in the other order)
    host_lock = std::unique_lock<std::mutex>(ix->host_mu);
    lane = ix;
    rc = search_host_enqueue(ix, queries, nq, K, ef_search, num_initializations, out, host_filter, exhaustive);
  }
  if (rc) return rc;
  rc = search_host_finish(lane);
  if (lane != ix) {  // what fnv_last_launch_info / _geometry report for the handle: the most recent call, whichever lane
    std::lock_guard<std::mutex> l1(ix->mu);  // served it -- the whole record, under the handle's mutex (same order as sync_lane)
    std::lock_guard<std::mutex> l2(lane->mu);
    ix->t_enqueue_ns = lane->t_enqueue_ns.load();
    ix->t_complete_ns = lane->t_complete_ns.load();
    ix->last_variant = lane->last_variant;
    ix->last_exploratory = lane->last_exploratory;
    ix->last_shadow = lane->last_shadow;
    ix->last_half = lane->last_half;
    for (int i = 0; i < 8; i++) ix->geom[i] = lane->geom[i];
    ix->last_served = lane;  // (lanes live as long as the handle)
  }
  return rc;
}

int fnv_search_batch(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                     float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist,
                     uint64_t* out_nhops) {
  return search_batch_host(ix, queries, nq, K, ef_search, num_initializations,
                           SearchOutputs{out_dist, out_labels, out_count, out_ndist, out_nhops}, nullptr);
}

// ---- filtered search: results restricted to the nodes whose label is set in a bitmap over label values -------------
static int check_filter_args(const void* allowed_bits, uint64_t n_bits) {
  if (n_bits > (1ull << 31)) return fail(FNV_ERR_INVALID, "n_bits must be at most 2^31 (labels are int32)");
  if (n_bits > 0 && !allowed_bits) return fail(FNV_ERR_INVALID, "allowed_bits is null but n_bits > 0");
  return FNV_OK;
}

int fnv_search_batch_filtered(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                              const void* allowed_bits, uint64_t n_bits, float* out_dist, int32_t* out_labels,
                              int32_t* out_count, uint64_t* out_ndist, uint64_t* out_nhops) {
  int rc = check_filter_args(allowed_bits, n_bits);
  if (rc) return rc;
  const SearchFilter f{(const uint8_t*)allowed_bits, n_bits};
  return search_batch_host(ix, queries, nq, K, ef_search, num_initializations,
                           SearchOutputs{out_dist, out_labels, out_count, out_ndist, out_nhops}, &f);
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

// ---- exhaustive search: the exact K nearest among the live nodes, or among those whose label is allowed (scan.hpp) -----
static int check_exhaustive_args(fnv_index_t ix, int K, int use_filter, const void* allowed_bits, uint64_t n_bits) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (K < 1 || K > SCAN_MAX_K) return fail(FNV_ERR_INVALID, "K of an exhaustive search must be between 1 and 1024");
  return use_filter ? check_filter_args(allowed_bits, n_bits) : FNV_OK;
}

int fnv_search_batch_exhaustive(fnv_index_t ix, const void* queries, uint64_t nq, int K, int use_filter, const void* allowed_bits,
                                uint64_t n_bits, float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist) {
  int rc = check_exhaustive_args(ix, K, use_filter, allowed_bits, n_bits);
  if (rc) return rc;
  const SearchFilter f{(const uint8_t*)allowed_bits, n_bits};
  return search_batch_host(ix, queries, nq, K, /*ef_search=*/1, /*num_initializations=*/1,
                           SearchOutputs{out_dist, out_labels, out_count, out_ndist, nullptr}, use_filter ? &f : nullptr, true);
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

// ---- grouped filters: a table of allowed sets and, per query, which of them it uses ----------------------------------
static int check_grouped_args(const void* filters, uint64_t n_filters, uint64_t stride, uint64_t n_bits, const int32_t* query_filter,
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
// (host entry points: the array is theirs to read before anything is launched)
static int check_query_filter_values(const int32_t* query_filter, uint64_t nq, uint64_t n_filters) {
  for (uint64_t q = 0; q < nq; q++)
    if (query_filter[q] < -1 || (int64_t)query_filter[q] >= (int64_t)n_filters)
      return fail(FNV_ERR_INVALID, "query_filter[" + std::to_string(q) + "] = " + std::to_string(query_filter[q]) +
                                       " is neither -1 nor a filter of the table (n_filters = " + std::to_string(n_filters) + ")");
  return FNV_OK;
}

int fnv_search_batch_filtered_grouped(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                                      const void* filters, uint64_t n_filters, uint64_t filter_stride_bytes, uint64_t n_bits,
                                      const int32_t* query_filter, float* out_dist, int32_t* out_labels, int32_t* out_count,
                                      uint64_t* out_ndist, uint64_t* out_nhops) {
  SearchFilter f{nullptr, 0};
  int rc = check_grouped_args(filters, n_filters, filter_stride_bytes, n_bits, query_filter, nq, &f);
  if (!rc) rc = check_search_args(ix, queries, nq, K, ef_search, num_initializations, out_dist, out_labels);
  if (!rc) rc = check_query_filter_values(query_filter, nq, n_filters);
  if (rc) return rc;
  return search_batch_host(ix, queries, nq, K, ef_search, num_initializations,
                           SearchOutputs{out_dist, out_labels, out_count, out_ndist, out_nhops}, &f);
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

int fnv_search_batch_exhaustive_grouped(fnv_index_t ix, const void* queries, uint64_t nq, int K, const void* filters, uint64_t n_filters,
                                        uint64_t filter_stride_bytes, uint64_t n_bits, const int32_t* query_filter, float* out_dist,
                                        int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist) {
  SearchFilter f{nullptr, 0};
  int rc = check_exhaustive_args(ix, K, 0, nullptr, 0);
  if (!rc) rc = check_grouped_args(filters, n_filters, filter_stride_bytes, n_bits, query_filter, nq, &f);
  if (!rc && nq && (!queries || !out_dist || !out_labels)) rc = fail(FNV_ERR_INVALID, "null buffer");
  if (!rc) rc = check_query_filter_values(query_filter, nq, n_filters);
  if (rc) return rc;
  return search_batch_host(ix, queries, nq, K, /*ef_search=*/1, /*num_initializations=*/1,
                           SearchOutputs{out_dist, out_labels, out_count, out_ndist, nullptr}, &f, true);
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

// ---- several GPUs behind one call -----------------------------------------------------------------
int fnv_replicate(fnv_index_t src, int n_devices, const int* devices, fnv_index_t* out) {
  if (!src || !out || n_devices <= 0) return fail(FNV_ERR_INVALID, "null argument");
  int visible = 0;
  HIP_TRY(hipGetDeviceCount(&visible));
  for (int i = 0; i < n_devices; i++) out[i] = nullptr;
  auto undo = [&]() {
    for (int i = 0; i < n_devices; i++) {
      if (out[i]) fnv_index_free(out[i]);
      out[i] = nullptr;
    }
  };
  for (int i = 0; i < n_devices; i++) {
    const int dev = devices ? devices[i] : i;
    if (dev < 0 || dev >= visible) {
      undo();
      return fail(FNV_ERR_INVALID, "fnv_replicate: device ordinal " + std::to_string(dev) + " is not visible");
    }
    int rc = fnv_index_alloc(src->M, src->capacity, src->dtype, src->metric, src->dim, dev, &out[i]);
    if (rc) {
      undo();
      return rc;
    }
  }
  int rc = fnv_replica_refresh(src, n_devices, out);  // also hands the source's options to every replica
  if (rc) undo();
  return rc;
}

// What the source measured -- kernel variant per (beam width, batch class), LDS layout per beam width -- holds for a replica
// on the same GPU model under the same options (round 6; before, a refresh cleared it and each of the seven replicas of an
// 8-GPU run re-explored for up to 18 launches of its own).  Another GPU model starts empty and measures for itself.
// Both handles' mutexes are held by the caller (source first).
static void inherit_measurements(const fnv_index_s* src, fnv_index_s* r) {
  const bool same_model = r->num_cus == src->num_cus && r->gcn_arch == src->gcn_arch;
  if (same_model) {
    r->tuner = src->tuner;
    r->layouts = src->layouts;
  } else {
    r->tuner.clear();
    r->layouts.clear();  // measured under the old options (a stale table size could even change the kernel mode)
  }
  r->sample_kernel = -1;
  r->measured_half = same_model ? src->measured_half : -1;  // (a replica without the source's mirror discards them at its first launch)
  r->replica_epoch = src->tune_epoch;
  r->tune_epoch++;  // (the replica's own lanes re-copy)
}

int fnv_replica_refresh(fnv_index_t src, int n_replicas, fnv_index_t* replicas) {
  if (!src || (!replicas && n_replicas)) return fail(FNV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(src->mu);
  int caller_device = -1;
  (void)hipGetDevice(&caller_device);
  struct Restore {
    int dev;
    ~Restore() { if (dev >= 0) (void)hipSetDevice(dev); }
  } restore{caller_device};
  const uint64_t live = src->n_nodes;
  const size_t bytes[4] = {(size_t)live * src->row_bytes, (size_t)live * src->M * 4, (size_t)live * 4, (size_t)live * src->tail_bytes};
  for (int i = 0; i < n_replicas; i++) {
    fnv_index_t r = replicas[i];
    if (!r || r->capacity < live || r->row_bytes != src->row_bytes || r->tail_bytes != src->tail_bytes || r->M != src->M ||
        r->dtype != src->dtype || r->metric != src->metric)
      return fail(FNV_ERR_INVALID, "fnv_replica_refresh: replica geometry does not match the source index");
  }
  // A replica answers its shard of a batch exactly as the source would: same options (kernel choice, node ids vs
  // labels, table sizes ...), whatever they were when the replica was made.
  for (int i = 0; i < n_replicas; i++) {
    fnv_index_t r = replicas[i];
    std::lock_guard<std::mutex> rl(r->mu);
    static_cast<IndexOptions&>(*r) = static_cast<const IndexOptions&>(*src);
    r->options_version++;
    r->replica_of = src;
    r->replica_options = src->options_version;
    inherit_measurements(src, r);
    r->plan.valid = false;
  }
  // Doubling tree of peer copies over xGMI: in every round each index that already holds the data feeds one that
  // does not (1 -> 2 -> 4 -> 8 holders: three rounds for eight GPUs, every link busy once per round).  The copies
  // of a round run concurrently on the destination indexes' streams.
  for (int i = 0; i < n_replicas; i++)  // direct xGMI copies where the platform allows them (else staged by the runtime)
    if (replicas[i]->device != src->device) {
      (void)hipSetDevice(replicas[i]->device);
      (void)hipDeviceEnablePeerAccess(src->device, 0);
      for (int j = 0; j < n_replicas; j++)
        if (replicas[j]->device != replicas[i]->device) (void)hipDeviceEnablePeerAccess(replicas[j]->device, 0);
    }
  (void)hipGetLastError();  // "peer access already enabled" is not an error
  std::vector<fnv_index_t> have{src}, need(replicas, replicas + n_replicas);
  size_t next = 0;
  while (next < need.size()) {
    const size_t senders = have.size();
    std::vector<fnv_index_t> round;
    for (size_t s = 0; s < senders && next < need.size(); s++, next++) {
      fnv_index_t from = have[s], to = need[next];
      const void* srcp[4] = {from->d_vectors, from->d_links, from->d_labels, from->tails()};
      void* dstp[4] = {to->d_vectors, to->d_links, to->d_labels, const_cast<uint8_t*>(to->tails())};
      HIP_TRY(hipSetDevice(to->device));
      for (int b = 0; b < 4; b++) {
        if (bytes[b] == 0) continue;  // (no side table)
        if (from->device == to->device)
          HIP_TRY(hipMemcpyAsync(dstp[b], srcp[b], bytes[b], hipMemcpyDeviceToDevice, to->stream));
        else
          HIP_TRY(hipMemcpyPeerAsync(dstp[b], to->device, srcp[b], from->device, bytes[b], to->stream));
      }
      round.push_back(to);
    }
    for (fnv_index_t to : round) {
      HIP_TRY(hipSetDevice(to->device));
      HIP_TRY(hipStreamSynchronize(to->stream));
      to->n_nodes = live;
      have.push_back(to);
    }
  }
  // a source that is searched from its half-width mirror gives every replica one: rebuilt there from the rows just copied
  if (src->half.state.load() == HALF_LIVE && src->half.covered.load() >= live)
    for (int i = 0; i < n_replicas; i++) {
      fnv_index_t r = replicas[i];
      std::lock_guard<std::mutex> rl(r->mu);
      HIP_TRY(hipSetDevice(r->device));
      int built = 0;
      const int rc = half_rows_build(r, &built);
      if (rc) return rc;
    }
  return FNV_OK;
}

int fnv_search_batch_multi(fnv_index_t* indexes, int n_indexes, const void* queries, uint64_t nq, int K, int ef_search,
                           int num_initializations, float* out_dist, int32_t* out_labels, int32_t* out_count,
                           uint64_t* out_ndist, uint64_t* out_nhops) {
  if (!indexes || n_indexes <= 0) return fail(FNV_ERR_INVALID, "null argument");
  int rc = check_search_args(indexes[0], queries, nq, K, ef_search, num_initializations, out_dist, out_labels);
  if (rc || nq == 0) return rc;
  for (int g = 1; g < n_indexes; g++)
    if (!indexes[g] || indexes[g]->dim != indexes[0]->dim || indexes[g]->dtype != indexes[0]->dtype)
      return fail(FNV_ERR_INVALID, "fnv_search_batch_multi: indexes differ in geometry");
  for (int g = 1; g < n_indexes; g++)
    if (indexes[g]->output_node_ids != indexes[0]->output_node_ids)
      return fail(FNV_ERR_INVALID, "fnv_search_batch_multi: indexes differ in the output_node_ids option (labels and node ids would mix)");
  // Rows [g * ceil(Q/G), ...) go to index g.  Every shard is driven by its own host thread (shard 0 by
  // the caller's): a shard of the bench shape is 5 MB of pageable queries, and a pageable hipMemcpyAsync blocks its
  // host thread until the copy has been staged -- issued from ONE thread, GPU g+1 would not be launched before GPU g's
  // copy (and, on one stream per device, its kernel) had been waited for.  With a thread per device the staging copies,
  // launches and waits of all devices overlap, and hipSetDevice (per-thread state) never touches the caller's device.
  // Replicas of indexes[0] take over what it has measured since their last refresh (fnv_tune on the source after
  // fnv_replicate), as long as its options are still the ones they were given.
  for (int g = 1; g < n_indexes; g++) {
    fnv_index_t r = indexes[g], src = indexes[0];
    if (r == src || r->replica_of != src) continue;
    std::lock_guard<std::mutex> l1(src->mu);
    std::lock_guard<std::mutex> l2(r->mu);
    if (r->replica_options == src->options_version && r->replica_epoch != src->tune_epoch) {
      inherit_measurements(src, r);
      r->plan.valid = false;  // (a layout choice changes the plan)
    }
  }
  const uint64_t per = (nq + (uint64_t)n_indexes - 1) / (uint64_t)n_indexes;
  const size_t qrow = (size_t)indexes[0]->dim * dtype_size(indexes[0]->dtype);
  int shards = 0;
  for (int g = 0; g < n_indexes; g++)
    if (std::min<uint64_t>(nq, (uint64_t)g * per) < nq) shards = g + 1;
  std::vector<int> rcs((size_t)shards, FNV_OK);
  std::vector<std::string> msgs((size_t)shards);
  auto run_shard = [&](int g) {
    const uint64_t lo = std::min<uint64_t>(nq, (uint64_t)g * per), hi = std::min<uint64_t>(nq, lo + per);
    rcs[g] = fnv_search_batch(indexes[g], (const uint8_t*)queries + lo * qrow, hi - lo, K, ef_search, num_initializations,
                              out_dist + lo * K, out_labels + lo * K, out_count ? out_count + lo : nullptr,
                              out_ndist ? out_ndist + lo : nullptr, out_nhops ? out_nhops + lo : nullptr);
    if (rcs[g]) msgs[g] = g_err;  // thread-local: carried back by hand
  };
  std::vector<std::thread> workers;
  for (int g = 1; g < shards; g++) workers.emplace_back(run_shard, g);
  run_shard(0);
  for (std::thread& w : workers) w.join();
  for (int g = 0; g < shards; g++)
    if (rcs[g]) return fail(rcs[g], msgs[g]);
  return FNV_OK;
}

// ---- the adaptive kernel choice, taken in one go --------------------------------------------------------------------
// Runs every variant the adaptive choice ("sorted_beam" = 2) would try for this (beam width, batch size class) on the
// caller's queries -- a cold launch plus three timed ones each -- and settles the choice, so that the caller's own
// launches never are exploratory ones.  Results are discarded (scratch buffers of the index).
int fnv_tune(fnv_index_t ix, const void* queries, uint64_t nq, int queries_on_device, int K, int ef_search,
             int num_initializations) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (num_initializations <= 0) return fail(FNV_ERR_INVALID, "num_initializations must be greater than 0.");
  if (K <= 0 || ef_search <= 0) return fail(FNV_ERR_INVALID, "K and ef_search must be positive");
  if (!queries || nq == 0) return fail(FNV_ERR_INVALID, "fnv_tune needs a batch of queries");
  HoldAllLanes hold(ix);
  ON_DEVICE(ix->device);
  const size_t qbytes = (size_t)nq * ix->dim * dtype_size(ix->dtype);
  const size_t o_lab = (size_t)nq * K * 4, obytes = 2 * o_lab;
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    int rc = ix->d_q.grow(2 * qbytes);
    if (!rc) rc = ix->d_out.grow(obytes);
    if (rc) return rc;
  }
  // The batch twice in a row: a launch on rows [off, off + nq) searches the same queries in a rotated order.  Which
  // queries tie -- and so which ones are stragglers of the last round -- is a property of the queries: timing several
  // rotations and averaging measures a variant's EXPECTED time, not its luck with one order.
  uint8_t* dq2 = ix->d_q.as<uint8_t>();
  HIP_TRY(hipMemcpy(dq2, queries, qbytes, queries_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dq2 + qbytes, dq2, qbytes, hipMemcpyDeviceToDevice));
  const size_t qrow_bytes = (size_t)ix->dim * dtype_size(ix->dtype);
  SearchOutputs scratch;  // distances | labels, nothing else
  scratch.dist = ix->d_out.as<float>();
  scratch.labels = (int32_t*)(ix->d_out.as<uint8_t>() + o_lab);
  auto launch = [&](int variant, uint64_t rotate = 0) -> int {
    SearchOptions opt;
    opt.force_variant = variant;
    return search_device_impl(ix, dq2 + (rotate % nq) * qrow_bytes, nq, K, ef_search, num_initializations, scratch, ix->stream, opt);
  };
  // what kind of launch is this?  (one probing launch of the merged-beam kernel tells: plan, round size)
  const int B = std::max(ef_search, K);
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->layouts.erase(B);
    ix->tuner.erase(tuner_key(B, false));
    ix->tuner.erase(tuner_key(B, true));
    ix->plan.valid = false;
    ix->tune_epoch++;  // (whatever follows -- including the early return below -- lanes drop their copy of the old choice)
  }
  int rc = launch(1);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ix->stream));
  if (ix->geom[6] == MODE_HEAPS || ix->sorted_beam != 2 || ix->sorted_variant >= 0 || nq < 2048) return FNV_OK;  // nothing to choose
  // Every timed launch starts from cold caches: the SAME queries visit the same nodes launch after launch, so the index
  // rows and -- above all -- the words of the per-slot HBM visited bitmaps they touch would sit in the 256 MiB Infinity
  // Cache by the second launch, which flatters exactly the layouts that spill most (small visited tables); a caller's
  // consecutive batches are different queries.  (Measured: without this the layout choice for 100-d rows at ef=200
  // flipped between boxes to a 4096-slot table that is 10 % slower under the bench protocol.)
  struct Flush {
    void* p = nullptr;
    size_t bytes = 768u << 20;
    ~Flush() { if (p) (void)hipFree(p); }
  } flush;
  const char* flush_env = getenv("FLATNAV_TUNE_FLUSH");  // developer knob: 0 = time warm launches
  if (flush_env && flush_env[0] == '0') flush.p = nullptr;
  else if (hipMalloc(&flush.p, flush.bytes) != hipSuccess) flush.p = nullptr;  // (no room: tune warm, as before)
  (void)hipGetLastError();
  // mean of `reps` timed launches of one variant, each on another rotation of the batch (after a cold launch), ms per query
  auto time_variant = [&](int v, int reps, float* out) -> int {
    float sum = 0.f;
    for (int rep = 0; rep <= reps; rep++) {
      if (rep > 0 && flush.p) HIP_TRY(hipMemsetAsync(flush.p, rep, flush.bytes, ix->stream));
      const int r = launch(v, rep == 0 ? 0 : (uint64_t)(rep - 1) * nq / (uint64_t)reps);
      if (r) return r;
      HIP_TRY(hipStreamSynchronize(ix->stream));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
      if (rep > 0) sum += ms;  // the first launch of a kernel is a cold one
    }
    *out = sum / (float)reps / (float)nq;
    return FNV_OK;
  };

  // ---- 1. the LDS layout ------------------------------------------------------------------------------------------
  // Resident queries, visited-table slots and the LDS home of the exact search's candidates heap trade against each
  // other, and which trade wins depends on the data (how often queries tie, how many ids a query visits): rules cover
  // the common cases (configure_launch), this measures the neighbours of the rule's choice -- heap home flipped, the
  // table one size up / down -- with the merged-beam kernel alone and with its whole last round straight to the exact
  // search, and keeps the fastest.  Skipped for whatever the caller pinned with an option.
  // (from the plan, not from the probing launch's geometry record: a DIRECT launch reports its bitmap's bits there)
  uint32_t base_slots = 0, base_vis_w = 0;
  bool base_heap_lds = false;
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    base_slots = ix->plan.sorted.vis_slots;
    base_vis_w = ix->plan.sorted.vis_w;
    base_heap_lds = ix->plan.sorted.cand_slots != 0;
  }
  const std::vector<LayoutChoice> cands = tune_layout_candidates(ix, base_slots, base_vis_w, base_heap_lds);
  const bool tune_log = getenv("FLATNAV_TUNE_LOG") != nullptr;  // developer aid: every measurement on stderr
  size_t best_layout = 0;
  float best_layout_t = -1.f;
  // one layout's time: the better of the merged-beam kernel alone and with 75 % of its last round straight to the exact search
  auto time_layout = [&](size_t li, float* out) -> int {
    {
      std::lock_guard<std::mutex> lock(ix->mu);
      if (li == 0) ix->layouts.erase(B);
      else ix->layouts[B] = cands[li];
      ix->plan.valid = false;
    }
    float t1 = -1.f, t4 = -1.f;
    int r = time_variant(1, 4, &t1);
    if (r) return r;
    const bool multi = nq > (uint64_t)ix->plan.sbpc * (uint64_t)ix->num_cus;
    if (multi && ix->sorted_tail_exact_pct < 0 && (r = time_variant(3, 4, &t4)) != FNV_OK) return r;
    *out = (t4 > 0.f && t4 < t1) ? t4 : t1;
    if (tune_log)
      fprintf(stderr, "fnv_tune B=%d layout %zu (heap in LDS %d, table %u): merged %.4f ms, 75%% tail exact %.4f ms -> %u slots, %d per CU\n", B,
              li, (int)cands[li].cand_lds, cands[li].vis_slots, t1 * (float)nq, t4 * (float)nq, (unsigned)ix->geom[4], (int)ix->geom[3]);
    return FNV_OK;
  };
  // The device settles first.  After the GPU has idled (the caller computed something on the host) the first launches run
  // up to 70 % slower than the steady state, for about 0.3 s of work -- clocks and power state (measured inside bench.py:
  // the rules' layout, timed first, lost to a neighbour it beats by 10 %; launches of 8.3 ms that take 4.8 ms half a second
  // later).  The slow state is steady while it lasts, so "two launches agree" does not end it: launches repeat for half a
  // second, then until two in a row agree.
  {
    const auto t_begin = std::chrono::steady_clock::now();
    float prev = -1.f;
    for (int i = 0; i < 400; i++) {
      float t = 0.f;
      if (time_variant(1, 1, &t) != FNV_OK) break;
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
      if (tune_log) fprintf(stderr, "fnv_tune B=%d settling: %.4f ms (at %.2f s)\n", B, t * (float)nq, waited);
      if ((waited > 0.5 && prev > 0.f && fabsf(t - prev) < 0.02f * prev) || waited > 2.0) break;
      prev = t;
    }
  }
  bool won_by_duel = false;
  for (size_t li = 0; li < cands.size(); li++) {
    float t = -1.f;
    if (time_layout(li, &t) != FNV_OK) continue;  // e.g. a layout that does not fit LDS: not a candidate
    if (best_layout_t < 0.f || t < best_layout_t * 0.95f) {  // a neighbour must win by 5 %: less is box-to-box noise (round 4: a 2 % margin picked layouts that lost 5 % under the bench protocol)
      best_layout_t = t;
      best_layout = li;
      won_by_duel = false;
    } else if (t < best_layout_t * 0.985f) {
      // Inside the margin (round 6): ONE measurement cannot tell 2-4 % from drift, several that agree can -- the holder and the
      // challenger are timed twice more, alternately; the challenger takes over if it wins BOTH rounds by 1 % (round 5 saw
      // layouts that were 2-2.5 % faster on every box stay unused: 10M x 768 at 8192 slots; the means of four cold launches
      // repeat within 0.3 % -- 90.4 / 90.8 ms against 93.0 / 92.3 ms in the tune log behind profiles/r6_bench.json).
      float sum_b = 0.f, sum_c = 0.f;
      bool wins = true;
      int rounds = 0;
      for (; rounds < 2 && wins; rounds++) {
        float tb = -1.f, tc = -1.f;
        if (time_layout(best_layout, &tb) != FNV_OK || time_layout(li, &tc) != FNV_OK) wins = false;
        else wins = tc < tb * 0.99f;
        sum_b += tb;
        sum_c += tc;
      }
      if (tune_log) fprintf(stderr, "fnv_tune B=%d duel (%d round%s): layout %zu %.4f ms against layout %zu %.4f ms -> %s\n", B, rounds, rounds == 1 ? "" : "s",
                            li, sum_c / (float)rounds * (float)nq, best_layout, sum_b / (float)rounds * (float)nq,
                            wins ? "challenger" : "holder");
      if (wins) {
        best_layout_t = sum_c / (float)rounds;
        best_layout = li;
        won_by_duel = true;
      }
    }
  }
  if (best_layout != 0 && !won_by_duel) {  // a neighbour won on one measurement: the rules' layout was timed first, so it is timed once more, now last
    float again = -1.f;
    if (time_layout(0, &again) == FNV_OK && !(best_layout_t < again * 0.95f)) best_layout = 0;
  }
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    if (best_layout == 0) ix->layouts.erase(B);
    else ix->layouts[B] = cands[best_layout];
    ix->plan.valid = false;
    ix->tune_epoch++;
  }
  rc = launch(1);  // re-plan with the chosen layout
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ix->stream));

  // ---- 2. the kernel variant on that layout --------------------------------------------------------------------------
  const bool multi_round = nq > (uint64_t)ix->plan.sbpc * (uint64_t)ix->num_cus;
  Tuner t;
  for (int v = 0; v < kNumVariants; v++) {
    if (!variant_allowed(v, multi_round, ix->sorted_tail_exact_pct < 0, ix->shadow_exact != 0)) continue;
    rc = time_variant(v, 4, &t.best[v]);
    if (rc) return rc;
    if (tune_log) fprintf(stderr, "fnv_tune B=%d variant %d: %.4f ms\n", B, v, t.best[v] * (float)nq);
    t.samples[v] = 4;  // settled: later launches neither explore nor sample
  }
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->tuner[tuner_key(B, multi_round)] = t;
    ix->sample_kernel = -1;
    ix->tune_epoch++;
  }
  return check_device_status(ix);
}

// Measurement aid: the rate (GB/s of row bytes) a pure gather of random rows of this index's vector table reaches with
// the search kernel's own load pattern for this row width (relayout.hpp: gather_ceiling_kernel) at `waves_per_cu`
// resident waves (0: 16).  ~20-40 ms of GPU time.
int fnv_gather_ceiling(fnv_index_t ix, int waves_per_cu, double* gbps_out) {
  if (!ix || !gbps_out) return fail(FNV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  const uint64_t n_rows = ix->parent ? ix->parent->n_nodes.load() : ix->n_nodes.load();
  const uint32_t nchunks = ix->row_bytes / 16;
  const int cfg = pick_row_cfg(nchunks, ix->tail_bytes / 16);
  typedef void (*gather_fn)(const uint8_t*, uint64_t, uint32_t, int, uint32_t*);
  static const gather_fn kGather[kNumCfgs] = {gather_ceiling_kernel<8, 1>,  gather_ceiling_kernel<8, 2>,  gather_ceiling_kernel<8, 4>,
                                              gather_ceiling_kernel<16, 4>, gather_ceiling_kernel<32, 4>, gather_ceiling_kernel<64, 4>,
                                              gather_ceiling_kernel<64, 3>, gather_ceiling_kernel<8, 3>};  // (split rows: the main table's lines)
  const int G = kCfgs[cfg].G, CU = kCfgs[cfg].CU;
  const int PU = passes_of(G, CU);
  const int wpc = waves_per_cu > 0 ? std::min(waves_per_cu, 32) : 16;
  const uint32_t blocks = (uint32_t)(ix->num_cus * wpc);
  const double rows_per_iter = (double)blocks * (WAVE / G) * PU;  // rows one iteration of the whole grid reads
  const int iters = (int)std::max<double>(8.0, 120e9 / (rows_per_iter * (double)ix->row_bytes));  // ~120 GB ~ 20 ms
  uint32_t* d_sink = ix->d_dispenser + 2;  // an unused word of the workspace
  hipLaunchKernelGGL(kGather[cfg], dim3(blocks), dim3(WAVE), 0, ix->stream, ix->d_vectors, n_rows, ix->row_bytes, iters / 8 + 1, d_sink);  // warm
  HIP_TRY(hipEventRecord(ix->ev0, ix->stream));
  hipLaunchKernelGGL(kGather[cfg], dim3(blocks), dim3(WAVE), 0, ix->stream, ix->d_vectors, n_rows, ix->row_bytes, iters, d_sink);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ix->ev1, ix->stream));
  HIP_TRY(hipEventSynchronize(ix->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
  ix->sample_kernel = -1;  // ev0 / ev1 no longer bracket a search launch
  *gbps_out = rows_per_iter * (double)iters * (double)ix->row_bytes / 1e9 / ((double)ms / 1e3);
  return FNV_OK;
}

int fnv_last_launch_info(fnv_index_t ix, uint64_t info[4]) {
  if (!ix || !info) return fail(FNV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(ix->mu);
  info[0] = (uint64_t)ix->last_variant;
  info[1] = (ix->last_exploratory ? 1u : 0u) | (ix->last_shadow ? 2u : 0u);
  info[2] = ix->t_enqueue_ns;
  info[3] = ix->t_complete_ns;
  return FNV_OK;
}

int fnv_index_insert_batch(fnv_index_t ix, uint64_t first_node, uint64_t count, int ef_construction,
                           int num_initializations, uint64_t* evals_out) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (num_initializations <= 0) return fail(FNV_ERR_INVALID, "num_initializations must be greater than 0.");
  if (ef_construction <= 0) return fail(FNV_ERR_INVALID, "ef_construction must be positive");
  if (ix->M > (uint32_t)WAVE) return fail(FNV_ERR_INVALID, "device-side wiring supports max_edges_per_node <= 64");
  if (first_node != ix->n_nodes || first_node == 0)
    return fail(FNV_ERR_INVALID, "insert_batch: first_node must equal the live node count (and the graph be non-empty)");
  if (count > ix->capacity - first_node)
    return fail(FNV_ERR_RUNTIME, "Maximum number of nodes reached. (device index capacity)");
  if (evals_out) *evals_out = 0;
  if (count == 0) return FNV_OK;
  HoldAllLanes hold(ix);
  ON_DEVICE(ix->device);
  const int W = ef_construction;
  const uint32_t keep = std::max<uint32_t>(ix->M / 2, 1);  // Index.h:373
  const size_t esize = dtype_size(ix->dtype);
  const size_t qrow = (size_t)ix->dim * esize;
  const size_t qbytes = count * qrow;
  size_t obytes = 0;
  (void)lay_out_slab(nullptr, count, W, &obytes);
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    int rcg = ix->d_q.grow(qbytes);
    if (!rcg) rcg = ix->d_out.grow(obytes);
    if (rcg) return rcg;
  }
  const size_t nreq = (size_t)count * keep;
  size_t sort_bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)nreq, 0, 32, ix->stream));
  const size_t req_bytes = (nreq * 4 + 255) & ~(size_t)255;
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    int rcg = ix->d_wirebuf.grow(4 * req_bytes + sort_bytes + 256);
    if (rcg) return rcg;
  }
  SearchOutputs beams = lay_out_slab(ix->d_out.ptr, count, W);  // the beams: distances | node ids | counts | evaluations
  beams.nhops = nullptr;
  // the new nodes' vectors are the queries (Index.h:371: beamSearch(data, entry, ef_construction)); dense rows
  if (!ix->tail_bytes) {
    HIP_TRY(hipMemcpy2DAsync(ix->d_q.ptr, qrow, ix->d_vectors + first_node * (uint64_t)ix->row_bytes, ix->row_bytes, qrow,
                             count, hipMemcpyDeviceToDevice, ix->stream));
  } else {  // split rows: the main table's part of every row, then what the side table holds of it
    const size_t main_part = std::min<size_t>(qrow, ix->row_bytes), tail_part = qrow - main_part;
    HIP_TRY(hipMemcpy2DAsync(ix->d_q.ptr, qrow, ix->d_vectors + first_node * (uint64_t)ix->row_bytes, ix->row_bytes, main_part,
                             count, hipMemcpyDeviceToDevice, ix->stream));
    if (tail_part)
      HIP_TRY(hipMemcpy2DAsync(ix->d_q.as<uint8_t>() + main_part, qrow, ix->tails() + first_node * (uint64_t)ix->tail_bytes,
                               ix->tail_bytes, tail_part, count, hipMemcpyDeviceToDevice, ix->stream));
  }
  SearchOptions opt;
  opt.node_ids = true;
  int rc = search_device_impl(ix, ix->d_q.ptr, count, W, W, num_initializations, beams, ix->stream, opt);
  if (rc) return rc;

  std::lock_guard<std::mutex> lock(ix->mu);
  WireParams w;
  memset(&w, 0, sizeof(w));
  uint8_t* wb = ix->d_wirebuf.as<uint8_t>();
  uint32_t* req_target = (uint32_t*)wb;
  uint32_t* req_index = (uint32_t*)(wb + req_bytes);
  uint32_t* sorted_target = (uint32_t*)(wb + 2 * req_bytes);
  uint32_t* sorted_req = (uint32_t*)(wb + 3 * req_bytes);
  void* sort_tmp = wb + 4 * req_bytes;
  w.vectors = ix->d_vectors;
  w.tails = ix->tails();
  w.links = ix->d_links;
  w.req_target = req_target;
  w.sorted_target = sorted_target;
  w.sorted_req = sorted_req;
  w.beam_dist = beams.dist;
  w.beam_ids = beams.labels;
  w.beam_count = beams.count;
  w.dispenser = ix->d_dispenser;
  w.first_node = (uint32_t)first_node;
  w.count = (uint32_t)count;
  w.W = (uint32_t)W;
  w.M = ix->M;
  w.keep = keep;
  w.row_bytes = ix->row_bytes;
  const RowGeometry g = row_geometry(ix);
  w.nchunks = g.nchunks;
  w.tail_chunks = g.tail_chunks;
  w.q_chunks = g.q_chunks;
  w.cap = std::max<uint32_t>((uint32_t)W, 4 * ix->M);  // connect prunes row + up to cap - M requesters at a time
  auto align16 = [](uint32_t v) { return (v + 15u) & ~15u; };
  uint32_t off = 0;
  w.off_q = off;
  off = align16(off + w.q_chunks * 16);
  uint32_t* offs[] = {&w.off_ckey, &w.off_cid, &w.off_okey, &w.off_oid, &w.off_alive, &w.off_kept, &w.off_sel};
  for (uint32_t* f : offs) {
    *f = off;
    off = align16(off + (w.cap + 1) * 4);  // + a write-only bin slot
  }
  w.off_stage_ids = off;
  off = align16(off + (WAVE + 1) * 4);
  w.off_stage_idx = off;
  off = align16(off + (WAVE + 1) * 4);
  const uint32_t lds_bytes = off;
  if (lds_bytes > 160u * 1024u) return fail(FNV_ERR_INVALID, "ef_construction too large for the on-chip wiring state");
  wire_fn kernels[2] = {pick_wire_kernel(ix->dtype, ix->metric, g.cfg, g.full),
                        pick_connect_kernel(ix->dtype, ix->metric, g.cfg, g.full)};
  for (int phase = 0; phase < 2; phase++) {
    wire_fn kern = kernels[phase];
    HIP_TRY(raise_lds_limit((const void*)kern, ix->device, lds_bytes));
    int bpc = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, (const void*)kern, WAVE, lds_bytes));
    if (bpc < 1) bpc = 1;
    // select: one unit of work per new node; connect: per 64 positions of the sorted request list
    const uint64_t units = phase == 0 ? count : (nreq + WAVE - 1) / WAVE;
    const uint32_t nslots = (uint32_t)std::min<uint64_t>(units, (uint64_t)bpc * (uint64_t)ix->num_cus);
    HIP_TRY(hipMemsetAsync(ix->d_dispenser, 0, sizeof(uint32_t), ix->stream));
    hipLaunchKernelGGL(kern, dim3(nslots), dim3(WAVE), lds_bytes, ix->stream, w);
    HIP_TRY(hipGetLastError());
    if (phase == 0) {  // group the batch's back-link requests by target (stable: insertion order within a target)
      hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((nreq + 255) / 256)), dim3(256), 0, ix->stream, req_index, (uint32_t)nreq);
      HIP_TRY(hipGetLastError());
      size_t tmp = sort_bytes;
      HIP_TRY(hipcub::DeviceRadixSort::SortPairs(sort_tmp, tmp, (const uint32_t*)req_target, sorted_target,
                                                 (const uint32_t*)req_index, sorted_req, (int)nreq, 0, 32, ix->stream));
    }
  }
  std::vector<uint64_t> nd;
  if (evals_out) {
    nd.resize(count);
    HIP_TRY(hipMemcpyAsync(nd.data(), beams.ndist, count * 8, hipMemcpyDeviceToHost, ix->stream));
  }
  HIP_TRY(hipStreamSynchronize(ix->stream));
  if (evals_out) {
    uint64_t total = 0;
    for (uint64_t e : nd) total += e;
    *evals_out = total;
  }
  rc = check_device_status(ix, "raise spill_entries");
  if (rc) return rc;
  ix->n_nodes = first_node + count;
  return FNV_OK;
}

int fnv_index_read_links(fnv_index_t ix, uint64_t first_node, uint64_t count, uint32_t* out_rows) {
  if (!ix || (!out_rows && count)) return fail(FNV_ERR_INVALID, "null argument");
  if (first_node > ix->capacity || count > ix->capacity - first_node)
    return fail(FNV_ERR_INVALID, "node range outside the device index");
  if (count == 0) return FNV_OK;
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  HIP_TRY(hipMemcpy(out_rows, ix->d_links + first_node * (uint64_t)ix->M, count * 4ull * ix->M, hipMemcpyDeviceToHost));
  return FNV_OK;
}

// The handle whose events / counters describe the most recent launch of `ix`: a hidden lane if that served the last host-buffer call.
static fnv_index_s* last_launcher(fnv_index_t ix) {
  fnv_index_s* lane = ix->last_served.load();
  return lane ? lane : ix;
}

int fnv_last_kernel_ms(fnv_index_t ix, float* ms) {
  if (!ix || !ms) return fail(FNV_ERR_INVALID, "null argument");
  ix = last_launcher(ix);
  if (!ix->launched) return fail(FNV_ERR_RUNTIME, "no search has been launched on this index");
  ON_DEVICE(ix->device);
  HIP_TRY(hipEventSynchronize(ix->ev1));
  HIP_TRY(hipEventElapsedTime(ms, ix->ev0, ix->ev1));
  return FNV_OK;
}

#ifdef FNV_PHASE_TIMING
int fnv_debug_heap_microbench(int size, int iters, int blocks, uint64_t out[4]) {
  unsigned long long* d = nullptr;
  HIP_TRY(hipMalloc(&d, 4 * sizeof(unsigned long long)));
  hipLaunchKernelGGL(heap_microbench_kernel, dim3(blocks), dim3(WAVE), (size + 4) * 8 + 64, 0, size, iters, d);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipFree(d));
  return FNV_OK;
}
// Profiling builds only: cumulative shader cycles per kernel phase (and reset).
int fnv_debug_phase_cycles(fnv_index_t ix, uint64_t out[16]) {
  if (!ix || !out) return fail(FNV_ERR_INVALID, "null argument");
  ON_DEVICE(ix->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, ix->d_phase, NPHASE * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(ix->d_phase, 0, NPHASE * sizeof(uint64_t)));
  return FNV_OK;
}
#endif

#ifdef FNV_SPEC_STATS
// Developer builds only (-DFNV_SPEC_STATS): {hops whose node was the runner-up guessed one hop ahead, hops} of the last launch's
// queries that finished in the merged-beam kernel.
int fnv_debug_spec_stats(fnv_index_t ix, uint64_t out[2]) {
  if (!ix || !out) return fail(FNV_ERR_INVALID, "null argument");
  ix = last_launcher(ix);
  ON_DEVICE(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->last_stream));
  uint32_t w[2];
  HIP_TRY(hipMemcpy(w, ix->d_dispenser + 11, sizeof(w), hipMemcpyDeviceToHost));
  out[0] = w[0];
  out[1] = w[1];
  return FNV_OK;
}
#endif

int fnv_last_replayed_queries(fnv_index_t ix, uint64_t out[5]) {
  if (!ix || !out) return fail(FNV_ERR_INVALID, "null argument");
  for (int i = 0; i < 5; i++) out[i] = 0;
  ix = last_launcher(ix);
  if (!ix->launched) return FNV_OK;
  ON_DEVICE(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->last_stream));
  uint32_t w[5];
  HIP_TRY(hipMemcpy(w, ix->d_dispenser + 3, sizeof(w), hipMemcpyDeviceToHost));
  for (int i = 0; i < 5; i++) out[i] = w[i];
  return FNV_OK;
}

int fnv_last_handover_stats(fnv_index_t ix, uint64_t out[4]) {
  if (!ix || !out) return fail(FNV_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; i++) out[i] = 0;
  ix = last_launcher(ix);
  if (!ix->launched) return FNV_OK;
  ON_DEVICE(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->last_stream));
  uint32_t w[8];
  HIP_TRY(hipMemcpy(w, ix->d_dispenser + 3, sizeof(w), hipMemcpyDeviceToHost));
  out[0] = w[5];         // queries resumed from their hand-over log
  out[1] = w[6];         // hops taken from the logs
  out[2] = w[7];         // hops the merged-beam passes of those queries had made
  out[3] = w[0] - w[5];  // queries searched again from scratch
  return FNV_OK;
}

int fnv_lane_info(fnv_index_t ix, uint64_t info[16]) {
  if (!ix || !info) return fail(FNV_ERR_INVALID, "null argument");
  for (int i = 0; i < fnv_index_s::kMaxLanes; i++) {
    const fnv_index_s* l = i == 0 ? ix : ix->lanes[i].load();
    info[2 * i] = l ? (uint64_t)l->ws_bytes.load() : 0;
    info[2 * i + 1] = l ? l->explored_launches.load() : 0;
  }
  return FNV_OK;
}

int fnv_last_launch_geometry(fnv_index_t ix, uint64_t geom[8]) {
  if (!ix || !geom) return fail(FNV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(ix->mu);
  for (int i = 0; i < 8; i++) geom[i] = ix->geom[i];
  return FNV_OK;
}

}  // extern "C"
#pragma GCC visibility pop
