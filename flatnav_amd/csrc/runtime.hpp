// runtime.hpp -- the internal header of the host runtime (never installed): the MI355X (gfx950 / CDNA4) implementation of
// flatnav's batched k-NN search and of the C ABI declared in include/flatnav_hip.h, in the units that include it:
//   index.hip         handles: creation, views, options, upload and incremental writes, the half-width mirror
//   launch.hip        kernel lookup, the launch plan, one search launch (graph search and exhaustive scan), device entry points
//   host_search.hip   host-buffer searches: staging, the hidden lanes and their admission, host entry points
//   multi.hip         several GPUs behind one call
//   tune.hip          fnv_tune, measurement aids and the fnv_last_* reporting calls
//   device_build.hip  the device builder (fnv_index_insert_batch)
// Here: what they share -- error reporting, the device scope, the handle (fnv_index_s, with THE LOCK ORDER), what a launch
// is given, and the declarations of exactly the functions that cross a unit boundary.
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
// the whole shape of a graph-search launch (shape_search), the exhaustive scan's tiles, segments, grouping arrays and routing,
// K0's tile, the workspace's sizes: every decision that is arithmetic -- lives in launch_plan.hpp, free of HIP
// (tests/test_launch_plan.py runs it on the CPU; tests/test_gpu_scan_shape.py holds launches against it).  So does the adaptive
// choice (measurements.hpp, which the planner includes): what a handle has measured and every rule that changes it (the class
// Measurements), and fnv_tune's tournament over a measuring object (tests/test_adaptive_choice.py runs both on the CPU;
// tests/test_gpu_tune_replay.py replays a real tune's log through them).  These units own the HIP runtime around it: handles,
// buffers, streams and events, kernel lookup, the occupancy queries and LDS limits the planner asks for, the timed launches
// the adaptive choice is fed with, the launches and the C ABI.
//
// Also theirs: incremental construction (fnv_index_write_nodes / write_links / insert_batch: Index::add,
// include/flatnav/index/Index.h:353-378 with selectNeighbors :714-763 and connectNeighbors :765-834 as the
// wire_select / wire_connect kernels of wire.hpp); the merged-beam search kernel is merged_beam.hpp.
#pragma once
#include <hip/hip_runtime.h>
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

using namespace fnv_dev;

// ---- errors: the calling thread's last message (index.hip defines both) ------------------------------------------
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);

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
  bool timed = false;               // bracket the launch with the handle's events (fnv_tune, the host-buffer entry points)
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

// THE LOCK ORDER of a handle: who may hold what (the comments at each site refer here).
//   mu        launch configuration + workspace growth.  A launch reads the options and the measurements under it, an option
//             changes under it, and a buffer that grows on demand grows under it.  Two handles' mu: the SOURCE first, then its
//             replica or lane (sync_lane, fnv_replica_refresh, fnv_search_batch_multi).
//   host_mu   one host-buffer caller per lane for the whole call: the lane's d_q / d_out, staging areas, stream and workspace are
//             its caller's (the handle itself is lane 0).
//   lane_mu   admission, reservation and creation of the hidden lanes.  Taken BEFORE a lane's host_mu, and that by try_lock only
//             -- except in fnv_tune and fnv_index_insert_batch (HoldAllLanes): they take the handle's host_mu, lane_mu and then
//             every lane's host_mu, blocking, so that no host-buffer search runs on a lane meanwhile and none is created (a caller
//             that wants one waits on lane_mu, holding nothing).  Their thread sets t_holds_lanes_of: release_idle_lanes then frees
//             with the locks it already has -- try_lock on a std::mutex the calling thread owns is undefined behaviour.
//   A thread never waits for the handle (its host_mu) while it holds a lane: it lets the lane go first (search_batch_host), because
//   those two calls take them in the other order.
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
  bool last_half = false;  // the most recent launch read the mirror
  uint32_t* d_links = nullptr;
  int32_t* d_labels = nullptr;
  std::string gcn_arch;  // hipDeviceProp_t::gcnArchName: replicas on the same GPU model inherit the source's measurements
  uint64_t options_version = 0;
  PlannedLaunch plan;
  // The adaptive choice ("sorted_beam" = 2): the layouts fnv_tune measured, each variant's best time, the launch between
  // ev0 / ev1 that is a sample still to be harvested, the row mode they were measured in, and the epoch by which lanes and
  // replicas notice a change -- one object that keeps these consistent (measurements.hpp); the units only call it.  Whoever
  // records ev0 / ev1 for anything but a graph search calls drop_pending().
  Measurements measured;
  int last_variant = 0;         // what the most recent launch ran: 0 two-heap kernel, 1 merged beam, 2-4 with exact tail
  bool last_exploratory = false;  // ... and whether the adaptive choice was still sampling (not its final pick)
  bool last_shadow = false;       // ... and whether every query had an exact shadow (small launches)
  // host-buffer searches: steady-clock time of launch / of completion (atomic: every lane's caller reports into the handle)
  std::atomic<uint64_t> t_enqueue_ns{0}, t_complete_ns{0};
  // TWO dispenser blocks of 16 words, kDispenserStride words apart.  A block: [0] dispenser, [1] status, [3] queries a merged-beam
  // launch handed to the exact search, [4..7] by reason, [8] of them resumed from their log, [9] hops taken from logs, [10] hops
  // of those queries.  A search launch owns ONE block and zeroes the OTHER one from its kernel (kernels.hpp
  // clear_next_dispenser); the next launch on the handle takes that other block, so that a call enqueues no memset of its own.
  // THE RULE (next_dispenser_block, launch.hip): the kernel-side clear is ordered against the next launch only by stream order,
  // so it counts only while `zeroed_block` names a block and the new launch is on `last_stream`; every other launch -- the
  // first one, one on another stream, one after an exhaustive search (which memsets the block it reports its status in and
  // resets zeroed_block) -- memsets the block it takes, as every launch once did.  The device builder's wiring kernels and
  // gather_ceiling write words of their own behind the two blocks (kBuilderWord).  Each handle, view and hidden lane has its
  // own allocation.  Whoever reads a launch's status word or counters reads `last_block`, the block of that launch.
  static constexpr uint32_t kDispenserStride = 32;  // (128 bytes: the two blocks never share a cache line)
  static constexpr uint32_t kBuilderWord = 64;      // the device builder's own dispenser word; [+1]: gather_ceiling's sink
  static constexpr uint32_t kDispenserWords = 80;
  uint32_t* d_dispenser = nullptr;
  uint32_t* last_block = nullptr;  // the block of the most recent launch (record_launch); before any: d_dispenser
  int zeroed_block = -1;           // 0 / 1: the block the most recent launch's kernel zeroes on last_stream; -1: none
  // ev0 / ev1 bracket a launch only when somebody will read them: a sample of the adaptive choice, fnv_tune's launches, the
  // host-buffer entry points (fnv_last_kernel_ms after fnv_search_batch works as ever), and -- device-buffer entry points --
  // once "launch_timing" is set or fnv_last_kernel_ms has been called on the handle (which arms it for the launches after).
  std::atomic<bool> time_launches{false};
  bool last_timed = false;         // ev0 / ev1 bracket the most recent launch
  unsigned long long* d_phase = nullptr;  // profiling builds only
  // The launch workspace, per query slot: what search_device_impl grows, free_lane_workspace gives back and ws_bytes counts.
  struct Workspace {
    DeviceBuf bitmap;  // uint32 [nslots][bitmap_words]: the visited set's HBM part
    DeviceBuf ovf;     // uint32 [nslots][ovf_cap] ids whose bitmap words need clearing (big indexes)
    DeviceBuf spill;   // uint64 [nslots][spill_entries]: what the candidates heap does not keep in LDS
    DeviceBuf tielog;  // uint64, merged-beam kernel: [nslots][log_entries] hand-over log (round 5)
    DeviceBuf scan;    // uint64, exhaustive search: [nq][segments][K] partial lists (scan.hpp)
    DeviceBuf group;   // uint32, grouped exhaustive search: the grouping arrays (GroupArrays), O(nq + n_filters); routed filtered
                       // graph searches: the same for their scan stage, and the nq route words
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
  std::mutex mu, host_mu;  // (the lock order: above)
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
  std::mutex lane_mu;            // (the lock order: above)
  std::atomic<fnv_index_s*> last_served{nullptr};  // the lane that ran the handle's most recent launch (null: the handle itself):
                                                   // fnv_last_kernel_ms / _replayed_queries / _handover_stats read ITS events and counters
  // (on a lane: its owner's measured.epoch() and options_version when it last copied them; it copies again when either lags)
  uint64_t lane_epoch = ~0ull, lane_options = ~0ull;
  // (on a replica, round 6) the handle fnv_replica_refresh last copied options from, that handle's options_version then, and
  // its measured.epoch() whose measurements this replica holds: fnv_search_batch_multi hands newer measurements over (pointer
  // compared, never followed, outside calls that were given the source itself)
  const fnv_index_s* replica_of = nullptr;
  uint64_t replica_options = ~0ull, replica_epoch = ~0ull;
};

// The live nodes a launch on `ix` sees: a view (or hidden lane) follows its source's growth.
inline uint64_t live_nodes(const fnv_index_s* ix) { return ix->parent ? ix->parent->n_nodes.load() : ix->n_nodes.load(); }
// What every graph search checks of its sizes (Index.h:847-849).
inline int check_search_sizes(int K, int ef_search, int num_initializations) {
  if (num_initializations <= 0) return fail(FNV_ERR_INVALID, "num_initializations must be greater than 0.");
  if (K <= 0 || ef_search <= 0) return fail(FNV_ERR_INVALID, "K and ef_search must be positive");
  return FNV_OK;
}

// ---- what crosses a unit boundary (everything else is static in its unit) ----------------------------------------------
// index.hip
const fnv_index_s* rows_source(const fnv_index_s* ix);
int half_rows_build(fnv_index_s* ix, int* built);
// launch.hip
hipError_t raise_lds_limit(const void* kern, int device, uint32_t bytes);
wire_fn pick_wire_kernel(int dtype, int metric, int cfg, bool full);
wire_fn pick_connect_kernel(int dtype, int metric, int cfg, bool full);
bool half_rows_possible(const fnv_index_s* ix);
int check_status(int32_t st, const char* advice = "raise the spill_entries option");
int check_device_status(fnv_index_s* ix, const char* advice = "raise the spill_entries option");
size_t routed_workspace_bytes(fnv_index_s* ix, const SearchFilter& f, uint64_t nq, int K);
int search_device_impl(fnv_index_t ix, const void* d_queries, uint64_t nq, int K, int ef_search, int num_initializations,
                       const SearchOutputs& out, void* hip_stream, const SearchOptions& opt = SearchOptions());
int check_filter_args(const void* allowed_bits, uint64_t n_bits);
int check_exhaustive_args(fnv_index_t ix, int K, int use_filter, const void* allowed_bits, uint64_t n_bits);
int check_grouped_args(const void* filters, uint64_t n_filters, uint64_t stride, uint64_t n_bits, const int32_t* query_filter,
                       uint64_t nq, SearchFilter* out);
// host_search.hip
struct HoldAllLanes {  // fnv_tune / fnv_index_insert_batch: every lane of the handle, for the whole call (the lock order: fnv_index_s)
  std::lock_guard<std::mutex> host_lock, no_new_lanes;
  std::vector<std::unique_lock<std::mutex>> lane_locks;
  const fnv_index_s* before;
  explicit HoldAllLanes(fnv_index_s* ix);
  ~HoldAllLanes();
};
size_t release_idle_lanes(fnv_index_s* ix, const fnv_index_s* keep);
int check_search_args(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                      const float* out_dist, const int32_t* out_labels);
