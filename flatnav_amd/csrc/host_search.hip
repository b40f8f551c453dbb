// host_search.hip -- host-buffer searches of the host runtime (runtime.hpp): staging through pinned memory, the hidden
// lanes of concurrent callers and their admission, and the entry points that take host buffers with their argument checks.
#include "runtime.hpp"

// While fnv_tune / fnv_index_insert_batch run, their thread holds the handle's host_mu and lane_mu AND every lane's host_mu,
// taken up front (the lock order: fnv_index_s, runtime.hpp); release_idle_lanes then frees with the locks it already has.
static thread_local const fnv_index_s* t_holds_lanes_of = nullptr;
HoldAllLanes::HoldAllLanes(fnv_index_s* ix) : host_lock(ix->host_mu), no_new_lanes(ix->lane_mu), before(t_holds_lanes_of) {
  for (std::atomic<fnv_index_s*>& slot : ix->lanes)
    if (fnv_index_s* l = slot.load()) lane_locks.emplace_back(l->host_mu);
  t_holds_lanes_of = ix;
}
HoldAllLanes::~HoldAllLanes() { t_holds_lanes_of = before; }

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
size_t release_idle_lanes(fnv_index_s* ix, const fnv_index_s* keep) {
  if (t_holds_lanes_of == ix) return release_idle_lanes_locked(ix, keep, /*all_held=*/true);
  std::unique_lock<std::mutex> lanes_lock(ix->lane_mu, std::try_to_lock);
  if (!lanes_lock.owns_lock()) return 0;
  return release_idle_lanes_locked(ix, keep);
}

// HBM a launch of `nq` queries needs as per-slot workspace on a handle of this index (slot_workspace, launch_plan.hpp).
static size_t launch_workspace_bytes(fnv_index_s* ix, uint64_t nq) {
  std::lock_guard<std::mutex> lock(ix->mu);
  const int per_cu = ix->plan.valid ? std::max(ix->plan.bpc, ix->plan.sbpc) : 32;  // (no plan yet: the hardware's 32 waves per CU)
  const uint64_t slots = std::min<uint64_t>(2 * nq, (uint64_t)per_cu * (uint64_t)ix->num_cus);  // (small launches: a shadow per query)
  // (the plan's own formula -- plan.sorted is unset while the plan runs the two-heap kernel only; no plan yet: the largest automatic log)
  const uint64_t log_entries = ix->plan.valid ? log_entries_for(ix, ix->plan.B) : (ix->tie_replay ? std::max<uint64_t>(16384u, (uint64_t)ix->tie_log_entries) : 0u);
  return (size_t)(slots * slot_workspace(ix, log_entries).bytes());
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
  opt.timed = true;  // (a host-buffer call waits for its launch anyway: fnv_last_kernel_ms works after it as ever)
  const bool grouped = host_filter && host_filter->grouped;
  // (filter routing: a routed call's scan stage writes whole rows a second time -- it takes the staged copies, as grouped calls do)
  const bool staged_only = grouped || (host_filter && !exhaustive && filter_routing_on(ix));
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
  if (!pinned && ix->host_zero_copy != 0 && !staged_only) {  // (grouped and routed calls: always the staged copies)
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
  if (pinned && nq <= (uint64_t)ix->host_zero_copy && !staged_only) {
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
    HIP_TRY(hipMemcpyAsync(status, ix->last_block + 1, sizeof(int32_t), hipMemcpyDeviceToHost, ix->stream));  // (that launch's block)
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

int check_search_args(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search,
                             int num_initializations, const float* out_dist, const int32_t* out_labels) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (int rc = check_search_sizes(K, ef_search, num_initializations)) return rc;
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
  if (lane->lane_epoch == ix->measured.epoch() && lane->lane_options == ix->options_version) return;
  static_cast<IndexOptions&>(*lane) = static_cast<const IndexOptions&>(*ix);
  lane->measured.copy_from(ix->measured, true);
  lane->options_version++;  // (the lane's plan is made again)
  lane->lane_epoch = ix->measured.epoch();
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
    // test, and a batch that fits no lane (large index, FLATNAV_LANE_BUDGET_MB=0) creates none.  (The lock order: fnv_index_s.)
    // (a routed filtered search: its node bitmaps -- the grouped call's own among them --, grouping arrays, route words and partial lists)
    const size_t routed_need = host_filter && !exhaustive ? routed_workspace_bytes(ix, *host_filter, nq, K) : 0;
    const size_t need = launch_workspace_bytes(ix, nq) +
                        (routed_need ? routed_need : host_filter && host_filter->grouped ? filter_rows_bytes(ix, host_filter->rows()) : 0);
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
    host_lock.unlock();  // (never hold a lane while waiting for the handle: the lock order, fnv_index_s)
    host_lock = std::unique_lock<std::mutex>(ix->host_mu);
    lane = ix;
    rc = search_host_enqueue(ix, queries, nq, K, ef_search, num_initializations, out, host_filter, exhaustive);
  }
  if (rc) return rc;
  rc = search_host_finish(lane);
  if (lane != ix) {  // what fnv_last_launch_info / _geometry report for the handle: the most recent call, whichever lane
    std::lock_guard<std::mutex> l1(ix->mu);  // served it -- the whole record, under the handle's mutex (source, then lane)
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

// (host entry points: the array is theirs to read before anything is launched)
static int check_query_filter_values(const int32_t* query_filter, uint64_t nq, uint64_t n_filters) {
  for (uint64_t q = 0; q < nq; q++)
    if (query_filter[q] < -1 || (int64_t)query_filter[q] >= (int64_t)n_filters)
      return fail(FNV_ERR_INVALID, "query_filter[" + std::to_string(q) + "] = " + std::to_string(query_filter[q]) +
                                       " is neither -1 nor a filter of the table (n_filters = " + std::to_string(n_filters) + ")");
  return FNV_OK;
}

// Only the C ABI is exported (the library is built with -fvisibility=hidden).
#pragma GCC visibility push(default)
extern "C" {

int fnv_search_batch(fnv_index_t ix, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                     float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist,
                     uint64_t* out_nhops) {
  return search_batch_host(ix, queries, nq, K, ef_search, num_initializations,
                           SearchOutputs{out_dist, out_labels, out_count, out_ndist, out_nhops}, nullptr);
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

int fnv_search_batch_exhaustive(fnv_index_t ix, const void* queries, uint64_t nq, int K, int use_filter, const void* allowed_bits,
                                uint64_t n_bits, float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist) {
  int rc = check_exhaustive_args(ix, K, use_filter, allowed_bits, n_bits);
  if (rc) return rc;
  const SearchFilter f{(const uint8_t*)allowed_bits, n_bits};
  return search_batch_host(ix, queries, nq, K, /*ef_search=*/1, /*num_initializations=*/1,
                           SearchOutputs{out_dist, out_labels, out_count, out_ndist, nullptr}, use_filter ? &f : nullptr, true);
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

}  // extern "C"
#pragma GCC visibility pop
