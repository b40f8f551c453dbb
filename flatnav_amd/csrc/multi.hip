// multi.hip -- several GPUs behind one call, part of the host runtime (runtime.hpp): replicas of an index,
// their refresh over xGMI, and one batch sharded over them.
#include "runtime.hpp"

// What the source measured -- kernel variant per (beam width, batch class), LDS layout per beam width -- holds for a replica
// on the same GPU model under the same options (round 6; before, a refresh cleared it and each of the seven replicas of an
// 8-GPU run re-explored for up to 18 launches of its own).  Another GPU model starts empty and measures for itself.
// Both handles' mutexes are held by the caller (source first).
static void inherit_measurements(const fnv_index_s* src, fnv_index_s* r) {
  const bool same_model = r->num_cus == src->num_cus && r->gcn_arch == src->gcn_arch;
  // (another model: what the replica held was measured under the old options -- a stale table size could even change the kernel
  //  mode; the same model: a replica without the source's mirror discards the copy at its first launch.  The replica's plan is
  //  made again and its own lanes re-copy: copy_from sees to both.)
  r->measured.copy_from(src->measured, same_model);
  r->replica_epoch = src->measured.epoch();
}

// Only the C ABI is exported (the library is built with -fvisibility=hidden).
#pragma GCC visibility push(default)
extern "C" {

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
    if (r->replica_options == src->options_version && r->replica_epoch != src->measured.epoch()) inherit_measurements(src, r);
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

}  // extern "C"
#pragma GCC visibility pop
