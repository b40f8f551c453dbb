// flatnav/index/DeviceMirror.h -- the copy of a host node store that lives in HBM (header-only C++17, own code).
//
// flatnav::Index keeps its nodes on the host and answers every search on a GPU.  This class owns what lies between: the C-ABI
// handle of the copy on the primary GPU (flatnav_hip.h), the record of what the host changed since that copy was last brought
// up to date, the replicas on further GPUs, and the decision which calls follow which host mutation.  None of it depends on the
// index's distance or label type, so it is one plain class; Index hands it a StoreView when it asks for a sync.
//
// The promise: never a silently diverged device graph.  Host changes are either tracked (appended nodes, marked link rows: the
// next sync ships just those) or the mirror is declared untracked (markRebuild(): the next sync ships the whole store), and a
// write that fails half-way declares it untracked before its exception goes up.  tests/cpp/test_device_mirror.cpp pins the
// resulting call sequences against a recording C ABI, without a GPU.
//
// Nothing here locks: callers hold mutex() around every method but the three marks, which builder threads call while no
// search runs (markRow from any of them).
#pragma once

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <flatnav_hip.h>

namespace flatnav::detail {

// Maps a C-ABI status to the exception the reference throws at the same point.
inline void throwOnDeviceError(int rc) {
  if (rc == FNV_OK) return;
  std::string msg = fnv_last_error();
  if (rc == FNV_ERR_INVALID) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

// Which link rows the host builder has changed since the device mirror was last brought up to date (one byte
// per node, set from any thread), so that the next search ships those rows instead of the whole index.
class DirtyRows {
  std::unique_ptr<std::atomic<uint8_t>[]> _flags;
  std::atomic<uint64_t> _count{0};
  size_t _n = 0;

 public:
  void reset(size_t n) {
    _flags.reset(new std::atomic<uint8_t>[n]);
    for (size_t i = 0; i < n; ++i) _flags[i].store(0, std::memory_order_relaxed);
    _count.store(0);
    _n = n;
  }
  void mark(uint32_t node) {
    if (!_flags[node].exchange(1, std::memory_order_relaxed)) _count.fetch_add(1, std::memory_order_relaxed);
  }
  uint64_t count() const { return _count.load(); }
  // ids < limit that are marked, ascending; clears every mark
  std::vector<uint32_t> drain(size_t limit) {
    std::vector<uint32_t> ids;
    if (_count.load() != 0)
      for (size_t i = 0; i < _n; ++i)
        if (_flags[i].load(std::memory_order_relaxed)) {
          _flags[i].store(0, std::memory_order_relaxed);
          if (i < limit) ids.push_back(static_cast<uint32_t>(i));
        }
    _count.store(0);
    return ids;
  }
};

// What the mirror has to know of the host store to copy it: node records of node_size bytes, [data][M links][label].
struct StoreView {
  const char* base;
  size_t node_size, data_size, M;
  size_t cur_nodes, max_nodes;
  int data_type, metric;  // FNV_DTYPE_*, FNV_METRIC_*
  uint32_t dim;
  const char* node(size_t n) const { return base + static_cast<uint64_t>(n) * node_size; }
  const char* links(size_t n) const { return node(n) + data_size; }
};

class DeviceMirror {
  std::mutex _guard;
  fnv_index_t _handle = nullptr;
  size_t _capacity = 0;   // rows allocated on the device
  bool _stale = true;     // the mirror misses host-side changes (new nodes and / or dirty link rows)
  bool _rebuild = true;   // ... and they are not tracked: the whole store must be shipped again
  size_t _synced = 0;     // nodes [0, this) have their records on the device
  DirtyRows _dirty;       // link rows of synced nodes that changed since
  int64_t _filter_scan_max = 0;  // setFilterRouting: re-applied whenever the mirror is created anew
  bool _filter_scan_on_overflow = false;
  // several GPUs: the mirror on _ordinal is the primary; replicas of it live on the other devices of _devices (filled by peer
  // copies, refreshed whenever the primary changes); batches are sharded over all of them
  int _ordinal = 0;
  std::vector<int> _devices;        // empty: not decided yet (FLATNAV_DEVICES, else the primary GPU alone)
  bool _devices_defaulted = false;  // FLATNAV_DEVICES=all: "every visible GPU", whatever that turns out to be
  std::vector<fnv_index_t> _replicas;
  bool _replicas_stale = true;

  // The primary now holds exactly the host's n nodes and link rows; replicas on other GPUs do not yet.
  void inStep(size_t n) {
    _dirty.drain(0);
    _synced = n;
    _stale = _rebuild = false;
    _replicas_stale = true;
  }

  void applyFilterRouting() {
    throwOnDeviceError(fnv_set_option(_handle, "filter_scan_max", _filter_scan_max));
    throwOnDeviceError(fnv_set_option(_handle, "filter_scan_on_overflow", _filter_scan_on_overflow ? 1 : 0));
  }

  // The appended node records (fnv_index_write_nodes) and the link rows the builder touched (fnv_index_write_links).
  void shipIncrement(const StoreView& s) {
    // The marks are drained before the writes: if a write fails they are gone, so the mirror is declared untracked
    // (next call ships the whole store) before the error goes up -- never a silently diverged device graph.
    std::vector<uint32_t> ids = _dirty.drain(_synced);
    try {
      if (s.cur_nodes > _synced)
        throwOnDeviceError(fnv_index_write_nodes(_handle, _synced, s.cur_nodes - _synced, s.node(_synced), s.node_size, s.data_size));
      if (!ids.empty()) {
        std::vector<uint32_t> rows(ids.size() * s.M);
        for (size_t t = 0; t < ids.size(); ++t) std::memcpy(rows.data() + t * s.M, s.links(ids[t]), s.M * sizeof(uint32_t));
        throwOnDeviceError(fnv_index_write_links(_handle, ids.data(), rows.data(), ids.size()));
      }
      throwOnDeviceError(fnv_index_set_live_nodes(_handle, s.cur_nodes));
    } catch (...) {
      markRebuild();
      throw;
    }
  }

  void shipWhole(const StoreView& s) {
    if (_handle) {
      fnv_index_free(_handle);
      _handle = nullptr;
      dropReplicas();
    }
    if (s.cur_nodes == s.max_nodes) {  // complete: exactly as many rows as nodes
      throwOnDeviceError(fnv_index_upload(s.base, s.node_size, s.data_size, static_cast<uint32_t>(s.M), s.cur_nodes, s.data_type,
                                          s.metric, s.dim, _ordinal, &_handle));
      _capacity = s.cur_nodes;
    } else {  // still growing: room for every node the store can hold, so that later additions are appended
      throwOnDeviceError(fnv_index_alloc(static_cast<uint32_t>(s.M), s.max_nodes, s.data_type, s.metric, s.dim, _ordinal, &_handle));
      _capacity = s.max_nodes;
      throwOnDeviceError(fnv_index_write_nodes(_handle, 0, s.cur_nodes, s.base, s.node_size, s.data_size));
      throwOnDeviceError(fnv_index_set_live_nodes(_handle, s.cur_nodes));
    }
    if (_filter_scan_max != 0 || _filter_scan_on_overflow) applyFilterRouting();  // (a new handle starts with the library's defaults)
  }

  // The GPUs this index spreads its batches over: setDevices(), else the FLATNAV_DEVICES environment variable
  // ("0,1,2,3" -- an ordinal may repeat: tests put two replicas on one GPU -- or "all" = every visible device), else
  // the primary GPU alone: a library must not allocate a full index copy on every GPU of the node, nor move work to
  // devices the caller did not name, unasked.
  void resolveDevices() {
    if (!_devices.empty()) return;
    if (const char* env = std::getenv("FLATNAV_DEVICES")) {
      if (std::string(env) == "all") {  // the primary first, then every other visible GPU
        int count = 1;
        if (fnv_device_count(&count) != FNV_OK || count < 1) count = 1;
        _devices.push_back(_ordinal);
        for (int d = 0; d < count; ++d)
          if (d != _ordinal) _devices.push_back(d);
        _devices_defaulted = true;  // a replication failure falls back to the primary with a warning
      } else {
        std::stringstream ss(env);
        for (std::string tok; std::getline(ss, tok, ',');)
          if (!tok.empty()) _devices.push_back(std::stoi(tok));
      }
    }
    if (_devices.empty()) _devices.push_back(_ordinal);  // nobody asked for more: the primary GPU only
    _ordinal = _devices[0];
  }

 public:
  ~DeviceMirror() {
    dropReplicas();
    if (_handle) fnv_index_free(_handle);
  }

  std::mutex& mutex() { return _guard; }
  fnv_index_t handle() const { return _handle; }
  int ordinal() const { return _ordinal; }

  // ---- what the host builder reports ---------------------------------------------------------
  void resetRows(size_t max_nodes) { _dirty.reset(max_nodes); }  // a new store
  void markStale() { _stale = true; }                            // appended nodes / marked rows: tracked
  void markRebuild() { _stale = _rebuild = true; }               // anything else (reorder, graph import)
  void markRow(uint32_t node) { _dirty.mark(node); }

  // Brings the mirror up to date.  One that already holds a prefix of the nodes receives only what changed, unless that is
  // most of the index anyway; otherwise the store is shipped whole.
  void sync(const StoreView& s) {
    if (_handle && !_stale) return;
    resolveDevices();
    const bool incremental = _handle && !_rebuild && _capacity >= s.cur_nodes && _synced > 0 && _synced <= s.cur_nodes &&
                             _dirty.count() <= s.cur_nodes / 4;
    if (incremental) shipIncrement(s);
    else shipWhole(s);
    inStep(s.cur_nodes);
  }

  // ... with room for every node the store can hold: what the device-assisted builder appends to.  (A store that is not full
  // is always mirrored at full capacity; a full one leaves nothing to append.)
  void syncAtCapacity(const StoreView& s) {
    if (_handle && _capacity != s.max_nodes) markRebuild();
    sync(s);
  }

  // The scope of a builder that writes host store and mirror side by side: searches answer with node ids while it lasts, and a
  // scope left before complete() -- a device call threw mid-batch, leaving the two out of step in ways nothing tracks -- has the
  // mirror rebuilt from the host store by the next sync.
  class BuildScope {
    DeviceMirror& _mirror;
    bool _completed = false;

   public:
    explicit BuildScope(DeviceMirror& mirror) : _mirror(mirror) {
      throwOnDeviceError(fnv_set_option(_mirror._handle, "output_node_ids", 1));
    }
    void complete(size_t n) {  // both sides were kept in step up to n nodes
      _mirror.inStep(n);
      _completed = true;
    }
    ~BuildScope() {
      if (!_completed) _mirror.markRebuild();
      fnv_set_option(_mirror._handle, "output_node_ids", 0);
    }
  };

  // ---- placement -----------------------------------------------------------------------------
  void setDevices(const std::vector<int>& ordinals) {
    _devices_defaulted = false;
    if (ordinals == _devices) return;
    dropReplicas();
    if (ordinals[0] != _ordinal || _devices.empty()) markRebuild();
    _devices = ordinals;
    _ordinal = ordinals[0];
  }
  const std::vector<int>& devices() {
    resolveDevices();
    return _devices;
  }

  // The replicas, brought in line with the (up-to-date) primary; empty when there is one device, or none could be made.
  const std::vector<fnv_index_t>& replicas() {
    resolveDevices();
    if (_devices.size() <= 1) return _replicas;
    if (!_replicas_stale && _replicas.size() + 1 == _devices.size()) return _replicas;
    if (_replicas.size() + 1 != _devices.size()) {
      dropReplicas();
      _replicas.resize(_devices.size() - 1, nullptr);
      const int rc = fnv_replicate(_handle, static_cast<int>(_replicas.size()), _devices.data() + 1, _replicas.data());
      if (rc != FNV_OK) {
        _replicas.clear();
        if (_devices_defaulted) {  // nobody asked for the other GPUs: serve from the primary alone, say so once
          std::fprintf(stderr, "flatnav: replicating the index over %zu visible GPUs failed (%s); searching on device %d only\n",
                       _devices.size(), fnv_last_error(), _ordinal);
          _devices.assign(1, _ordinal);
          _replicas_stale = false;
          return _replicas;
        }
        throwOnDeviceError(rc);
      }
    } else {
      const int rc = fnv_replica_refresh(_handle, static_cast<int>(_replicas.size()), _replicas.data());
      if (rc != FNV_OK) {  // e.g. the primary was re-created with another capacity: start over
        dropReplicas();
        return replicas();
      }
    }
    _replicas_stale = false;
    return _replicas;
  }
  void dropReplicas() {
    for (fnv_index_t r : _replicas) fnv_index_free(r);
    _replicas.clear();
    _replicas_stale = true;
  }

  // Applies to the mirror now if there is one, and to every mirror made later.
  void setFilterRouting(int64_t scan_max_allowed, bool scan_on_overflow) {
    _filter_scan_max = scan_max_allowed;
    _filter_scan_on_overflow = scan_on_overflow;
    if (_handle) applyFilterRouting();
  }
};

}  // namespace flatnav::detail
