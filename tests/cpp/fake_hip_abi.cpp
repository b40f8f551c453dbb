// A recording stand-in for the C-ABI functions that include/flatnav/index/{Index,DeviceMirror}.h call (flatnav_hip.h), so that
// the host index links with plain g++ and no HIP library: tests/cpp/test_device_mirror.cpp drives the index and this file
// writes down what reached the device library.  The linker names any function that is missing here.
//
// Every call prints one line on stdout: its name, the handle's ordinal (#1, #2, ... in creation order) and every scalar
// argument; payloads (node records, link ids and rows, device lists) appear as a 64-bit FNV-1a checksum of their bytes, and
// pointers only as 0 / 1 (null or not) -- never an address.  Searches answer count = K, ndist = 5 per query, distances
// 0, 1, 2, ... and labels / node ids 0, 1, 2, ...; fnv_index_read_links answers empty (self-loop) rows.
// fake_fail_next(name) makes the next call with that line name print " -> FAIL" and return FNV_ERR_RUNTIME without effect.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <string>

#include <flatnav_hip.h>

struct fnv_index_s {
  int ordinal;
  uint32_t M;
};

namespace {

int g_handles = 0;
std::string g_fail_name, g_error = "no error";
const uint64_t kNdistPerQuery = 5;

uint64_t fnv1a(const void* bytes, uint64_t n) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char* p = static_cast<const unsigned char*>(bytes);
  for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

fnv_index_t newHandle(uint32_t M) { return new fnv_index_s{++g_handles, M}; }

// Prints the line; returns the status the call has to return.
int record(const char* name, const char* fmt, ...) {
  char line[1024];
  va_list args;
  va_start(args, fmt);
  std::vsnprintf(line, sizeof line, fmt, args);
  va_end(args);
  const bool fail = g_fail_name == name;
  std::printf("%s%s%s%s\n", name, line[0] ? " " : "", line, fail ? " -> FAIL" : "");
  if (!fail) return FNV_OK;
  g_error = "injected failure in " + g_fail_name;
  g_fail_name.clear();
  return FNV_ERR_RUNTIME;
}

void answer(uint64_t nq, int K, float* dist, int32_t* labels, int32_t* count, uint64_t* ndist) {
  for (uint64_t q = 0; q < nq; ++q) {
    for (int j = 0; j < K; ++j) {
      dist[q * K + j] = static_cast<float>(j);
      labels[q * K + j] = j;
    }
    if (count) count[q] = K;
    if (ndist) ndist[q] = kNdistPerQuery;
  }
}

std::string ordinals(fnv_index_t* handles, int n) {
  std::string s;
  for (int i = 0; i < n; ++i) s += (i ? ",#" : "#") + std::to_string(handles[i]->ordinal);
  return s;
}

}  // namespace

extern "C" {

void fake_fail_next(const char* name) { g_fail_name = name; }
void fake_note(const char* line) { std::printf("%s\n", line); }

const char* fnv_last_error(void) { return g_error.c_str(); }

int fnv_device_count(int* count) {
  *count = 3;
  return record("device_count", "-> 3");
}

int fnv_index_upload(const void* aos_blob, uint64_t node_size_bytes, uint64_t data_size_bytes, uint32_t M, uint64_t n_nodes,
                     int data_type, int metric, uint32_t dim, int device, fnv_index_t* out) {
  const int rc = record("upload", "#%d node_size=%" PRIu64 " data_size=%" PRIu64 " M=%u n=%" PRIu64 " dtype=%d metric=%d dim=%u device=%d bytes=%016" PRIx64,
                        g_handles + 1, node_size_bytes, data_size_bytes, M, n_nodes, data_type, metric, dim, device,
                        fnv1a(aos_blob, node_size_bytes * n_nodes));
  if (rc == FNV_OK) *out = newHandle(M);
  return rc;
}

int fnv_index_alloc(uint32_t M, uint64_t n_nodes, int data_type, int metric, uint32_t dim, int device, fnv_index_t* out) {
  const int rc = record("alloc", "#%d M=%u n=%" PRIu64 " dtype=%d metric=%d dim=%u device=%d", g_handles + 1, M, n_nodes, data_type,
                        metric, dim, device);
  if (rc == FNV_OK) *out = newHandle(M);
  return rc;
}

int fnv_index_free(fnv_index_t index) {
  const int rc = record("free", "#%d", index->ordinal);
  if (rc == FNV_OK) delete index;
  return rc;
}

int fnv_index_set_live_nodes(fnv_index_t index, uint64_t n_live) {
  return record("set_live", "#%d n=%" PRIu64, index->ordinal, n_live);
}

int fnv_index_write_nodes(fnv_index_t index, uint64_t first_node, uint64_t count, const void* aos_rows, uint64_t node_size_bytes,
                          uint64_t data_size_bytes) {
  return record("write_nodes", "#%d first=%" PRIu64 " count=%" PRIu64 " node_size=%" PRIu64 " data_size=%" PRIu64 " bytes=%016" PRIx64,
                index->ordinal, first_node, count, node_size_bytes, data_size_bytes, fnv1a(aos_rows, count * node_size_bytes));
}

int fnv_index_write_links(fnv_index_t index, const uint32_t* node_ids, const uint32_t* link_rows, uint64_t count) {
  bool ascending = true;
  for (uint64_t i = 1; i < count; ++i) ascending = ascending && node_ids[i - 1] < node_ids[i];
  return record("write_links", "#%d count=%" PRIu64 " ascending=%d max_id=%u ids=%016" PRIx64 " rows=%016" PRIx64, index->ordinal, count,
                ascending ? 1 : 0, count ? node_ids[count - 1] : 0u, fnv1a(node_ids, count * sizeof(uint32_t)),
                fnv1a(link_rows, count * index->M * sizeof(uint32_t)));
}

int fnv_index_insert_batch(fnv_index_t index, uint64_t first_node, uint64_t count, int ef_construction, int num_initializations,
                           uint64_t* evals_out) {
  const int rc = record("insert_batch", "#%d first=%" PRIu64 " count=%" PRIu64 " ef=%d n_init=%d evals=%d", index->ordinal, first_node,
                        count, ef_construction, num_initializations, evals_out ? 1 : 0);
  if (rc == FNV_OK && evals_out) *evals_out = 7 * count;
  return rc;
}

int fnv_index_read_links(fnv_index_t index, uint64_t first_node, uint64_t count, uint32_t* out_rows) {
  const int rc = record("read_links", "#%d first=%" PRIu64 " count=%" PRIu64, index->ordinal, first_node, count);
  for (uint64_t i = 0; rc == FNV_OK && i < count * index->M; ++i) out_rows[i] = static_cast<uint32_t>(first_node + i / index->M);
  return rc;
}

int fnv_set_option(fnv_index_t index, const char* name, int64_t value) {
  return record("set_option", "#%d %s=%" PRId64, index->ordinal, name, value);
}

int fnv_search_batch(fnv_index_t index, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                     float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist, uint64_t* out_nhops) {
  const int rc = record("search", "#%d nq=%" PRIu64 " K=%d ef=%d n_init=%d queries=%d count=%d ndist=%d nhops=%d", index->ordinal, nq, K,
                        ef_search, num_initializations, queries ? 1 : 0, out_count ? 1 : 0, out_ndist ? 1 : 0, out_nhops ? 1 : 0);
  if (rc == FNV_OK) answer(nq, K, out_dist, out_labels, out_count, out_ndist);
  return rc;
}

int fnv_search_batch_filtered(fnv_index_t index, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                              const void* allowed_bits, uint64_t n_bits, float* out_dist, int32_t* out_labels, int32_t* out_count,
                              uint64_t* out_ndist, uint64_t* out_nhops) {
  const int rc = record("search_filtered", "#%d nq=%" PRIu64 " K=%d ef=%d n_init=%d queries=%d bits=%d n_bits=%" PRIu64 " count=%d ndist=%d nhops=%d",
                        index->ordinal, nq, K, ef_search, num_initializations, queries ? 1 : 0, allowed_bits ? 1 : 0, n_bits,
                        out_count ? 1 : 0, out_ndist ? 1 : 0, out_nhops ? 1 : 0);
  if (rc == FNV_OK) answer(nq, K, out_dist, out_labels, out_count, out_ndist);
  return rc;
}

int fnv_search_batch_exhaustive(fnv_index_t index, const void* queries, uint64_t nq, int K, int use_filter, const void* allowed_bits,
                                uint64_t n_bits, float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist) {
  const int rc = record("search_exhaustive", "#%d nq=%" PRIu64 " K=%d use_filter=%d queries=%d bits=%d n_bits=%" PRIu64 " count=%d ndist=%d",
                        index->ordinal, nq, K, use_filter, queries ? 1 : 0, allowed_bits ? 1 : 0, n_bits, out_count ? 1 : 0,
                        out_ndist ? 1 : 0);
  if (rc == FNV_OK) answer(nq, K, out_dist, out_labels, out_count, out_ndist);
  return rc;
}

int fnv_search_batch_filtered_grouped(fnv_index_t index, const void* queries, uint64_t nq, int K, int ef_search, int num_initializations,
                                      const void* filters, uint64_t n_filters, uint64_t filter_stride_bytes, uint64_t n_bits,
                                      const int32_t* query_filter, float* out_dist, int32_t* out_labels, int32_t* out_count,
                                      uint64_t* out_ndist, uint64_t* out_nhops) {
  const int rc = record("search_filtered_grouped",
                        "#%d nq=%" PRIu64 " K=%d ef=%d n_init=%d queries=%d filters=%d n_filters=%" PRIu64 " stride=%" PRIu64 " n_bits=%" PRIu64
                        " query_filter=%016" PRIx64 " count=%d ndist=%d nhops=%d",
                        index->ordinal, nq, K, ef_search, num_initializations, queries ? 1 : 0, filters ? 1 : 0, n_filters,
                        filter_stride_bytes, n_bits, fnv1a(query_filter, nq * sizeof(int32_t)), out_count ? 1 : 0, out_ndist ? 1 : 0,
                        out_nhops ? 1 : 0);
  if (rc == FNV_OK) answer(nq, K, out_dist, out_labels, out_count, out_ndist);
  return rc;
}

int fnv_search_batch_exhaustive_grouped(fnv_index_t index, const void* queries, uint64_t nq, int K, const void* filters,
                                        uint64_t n_filters, uint64_t filter_stride_bytes, uint64_t n_bits, const int32_t* query_filter,
                                        float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist) {
  const int rc = record("search_exhaustive_grouped",
                        "#%d nq=%" PRIu64 " K=%d queries=%d filters=%d n_filters=%" PRIu64 " stride=%" PRIu64 " n_bits=%" PRIu64
                        " query_filter=%016" PRIx64 " count=%d ndist=%d",
                        index->ordinal, nq, K, queries ? 1 : 0, filters ? 1 : 0, n_filters, filter_stride_bytes, n_bits,
                        fnv1a(query_filter, nq * sizeof(int32_t)), out_count ? 1 : 0, out_ndist ? 1 : 0);
  if (rc == FNV_OK) answer(nq, K, out_dist, out_labels, out_count, out_ndist);
  return rc;
}

int fnv_replicate(fnv_index_t src, int n_devices, const int* devices, fnv_index_t* out) {
  std::string list;
  for (int i = 0; i < n_devices; ++i) list += (i ? "," : "") + std::to_string(devices[i]);
  const int rc = record("replicate", "#%d n=%d devices=%s list=%016" PRIx64 " first=#%d", src->ordinal, n_devices, list.c_str(),
                        fnv1a(devices, n_devices * sizeof(int)), g_handles + 1);
  for (int i = 0; rc == FNV_OK && i < n_devices; ++i) out[i] = newHandle(src->M);
  return rc;
}

int fnv_replica_refresh(fnv_index_t src, int n_replicas, fnv_index_t* replicas) {
  return record("refresh", "#%d n=%d replicas=%s", src->ordinal, n_replicas, ordinals(replicas, n_replicas).c_str());
}

int fnv_search_batch_multi(fnv_index_t* indexes, int n_indexes, const void* queries, uint64_t nq, int K, int ef_search,
                           int num_initializations, float* out_dist, int32_t* out_labels, int32_t* out_count, uint64_t* out_ndist,
                           uint64_t* out_nhops) {
  const int rc = record("multi", "%d handles=%s nq=%" PRIu64 " K=%d ef=%d n_init=%d queries=%d count=%d ndist=%d nhops=%d", n_indexes,
                        ordinals(indexes, n_indexes).c_str(), nq, K, ef_search, num_initializations, queries ? 1 : 0,
                        out_count ? 1 : 0, out_ndist ? 1 : 0, out_nhops ? 1 : 0);
  if (rc == FNV_OK) answer(nq, K, out_dist, out_labels, out_count, out_ndist);
  return rc;
}

}  // extern "C"
