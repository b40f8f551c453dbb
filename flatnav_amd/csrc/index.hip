// index.hip -- handles of the host runtime (runtime.hpp): creation, views, adoption and release, options, upload and
// incremental writes of nodes and links, the half-width mirror (half_rows.hpp) -- with the kernels only these launch.
#include "runtime.hpp"

namespace fnv_dev {

// ---------------------------------------------------------------------------------------------
// U1: AoS -> SoA re-layout of a staged block of nodes.  One thread per (node, 4-byte word) when
// everything is word aligned, else per byte.  Links: ids >= n_nodes are flagged; duplicates inside
// a row are replaced by the node's own id (== already visited, see header comment).
// ---------------------------------------------------------------------------------------------
__global__ void relayout_vectors_kernel(const uint8_t* __restrict__ aos, uint64_t node_size, uint64_t data_size,
                                        uint32_t row_bytes, uint32_t tail_bytes, uint64_t first_node, uint64_t count,
                                        uint8_t* __restrict__ vectors, uint8_t* __restrict__ tails, int word_ok) {
  // split rows (distance.hpp): bytes [0, row_bytes) of a row go to the main table, [row_bytes, row_bytes + tail_bytes) to the
  // side table; zero from data_size on in either
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t row_all = row_bytes + tail_bytes;
  if (word_ok) {
    const uint32_t wpr = row_all / 4;
    const uint64_t node = tid / wpr;
    const uint32_t b = (uint32_t)(tid % wpr) * 4u;
    if (node >= count) return;
    uint32_t val = 0;
    if ((uint64_t)b < data_size) val = *reinterpret_cast<const uint32_t*>(aos + node * node_size + b);
    uint8_t* dst = b < row_bytes ? vectors + (first_node + node) * row_bytes + b : tails + (first_node + node) * tail_bytes + (b - row_bytes);
    *reinterpret_cast<uint32_t*>(dst) = val;
  } else {
    const uint64_t node = tid / row_all;
    const uint32_t b = (uint32_t)(tid % row_all);
    if (node >= count) return;
    uint8_t* dst = b < row_bytes ? vectors + (first_node + node) * row_bytes + b : tails + (first_node + node) * tail_bytes + (b - row_bytes);
    *dst = b < data_size ? aos[node * node_size + b] : (uint8_t)0;
  }
}

// The half-width mirror (half_rows.hpp) of rows [first, first + count) of the float32 table: one thread per 16-byte mirror unit
// (two float32 chunks in, eight binary16 values out).  A value that binary16 does not hold exactly raises *lossy_flag.
__global__ __launch_bounds__(256) void half_rows_kernel(const uint8_t* __restrict__ vectors, uint32_t row_bytes, uint64_t first,
                                                        uint64_t count, uint32_t G, uint32_t CU, uint8_t* __restrict__ mirror,
                                                        int* lossy_flag) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t units = row_bytes / 32;  // per row
  const uint64_t row = tid / units;
  const uint32_t u = (uint32_t)(tid % units);
  if (row >= count) return;
  const uint32_t ca = half_first_chunk_of_unit(u, G, CU);
  const uint8_t* src = vectors + (first + row) * row_bytes;
  const uint4 a = *reinterpret_cast<const uint4*>(src + ca * 16u), b = *reinterpret_cast<const uint4*>(src + (ca + G) * 16u);
  const uint32_t f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t h[8];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    h[k] = half_bits_trunc(f[k]);
    ok = ok && half_bits_widen((uint16_t)h[k]) == f[k];
  }
  *reinterpret_cast<uint4*>(mirror + (first + row) * (uint64_t)(row_bytes / 2) + u * 16u) =
      make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
  if (!ok) atomicOr(lossy_flag, 1);
}

__global__ void relayout_links_kernel(const uint8_t* __restrict__ aos, uint64_t node_size, uint64_t data_size,
                                      uint32_t M, uint64_t first_node, uint64_t count, uint64_t n_nodes,
                                      uint32_t* __restrict__ links, int32_t* __restrict__ labels, int* bad_flag) {
  const uint64_t node = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= count) return;
  const uint8_t* base = aos + node * node_size + data_size;
  const uint32_t self = (uint32_t)(first_node + node);
  uint32_t* out = links + (first_node + node) * M;
  for (uint32_t i = 0; i < M; i++) {
    uint32_t id;
    memcpy(&id, base + (uint64_t)i * 4, 4);
    if ((uint64_t)id >= n_nodes) {
      atomicExch(bad_flag, 1);
      id = self;
    }
    for (uint32_t j = 0; j < i; j++) {
      uint32_t prev;
      memcpy(&prev, base + (uint64_t)j * 4, 4);
      if (prev == id) {
        id = self;
        break;
      }
    }
    out[i] = id;
  }
  int32_t lab;
  memcpy(&lab, base + (uint64_t)M * 4, 4);
  labels[first_node + node] = lab;
}

// Incremental construction: overwrite the link rows of `count` scattered nodes (same normalisation as above).
__global__ void scatter_links_kernel(const uint32_t* __restrict__ node_ids, const uint32_t* __restrict__ rows,
                                     uint64_t count, uint32_t M, uint64_t id_limit, uint32_t* __restrict__ links,
                                     int* bad_flag) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= count) return;
  const uint32_t self = node_ids[r];
  if ((uint64_t)self >= id_limit) {
    atomicExch(bad_flag, 1);
    return;
  }
  const uint32_t* in = rows + r * M;
  uint32_t* out = links + (uint64_t)self * M;
  for (uint32_t i = 0; i < M; i++) {
    uint32_t id = in[i];
    if ((uint64_t)id >= id_limit) {
      atomicExch(bad_flag, 1);
      id = self;
    }
    for (uint32_t j = 0; j < i; j++)
      if (in[j] == id) {
        id = self;
        break;
      }
    out[i] = id;
  }
}

}  // namespace fnv_dev

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

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
  HIP_TRY(hipMalloc(&ix->d_dispenser, fnv_index_s::kDispenserWords * sizeof(uint32_t)));
  HIP_TRY(hipMemset(ix->d_dispenser, 0, fnv_index_s::kDispenserWords * sizeof(uint32_t)));
  ix->last_block = ix->d_dispenser;
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

// The handle whose mirror a launch on `ix` reads: a view's / hidden lane's source, else the handle itself.
const fnv_index_s* rows_source(const fnv_index_s* ix) { return ix->parent ? ix->parent : ix; }
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
  info[3] = live_nodes(ix);
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
  // Under the handle's mutex (round 5): a launch reads the options and the measurements under it, and a concurrent
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
  else if (n == "filter_scan_max") ix->filter_scan_max = value;  // (read per filtered launch, like the next)
  else if (n == "filter_scan_on_overflow") ix->filter_scan_on_overflow = value != 0;
  else if (n == "half_rows") ix->half_rows = value;  // (read per launch; the mirror's launches are another kernel's: measurements go)
  else if (n == "launch_timing") ix->time_launches = value != 0;  // (read per launch)
  else return fail(FNV_ERR_INVALID, "unknown option: " + n);
  // What fnv_tune measured (kernel variant, LDS layout) stays valid across options that change neither the launch plan
  // nor the kernel choice: Index.h::addBatchDevice flips output_node_ids around every device build, and a tune costs
  // dozens of launches.  (output_node_ids is read per launch; shadow_exact per launch; tune_layout by fnv_tune itself.)
  const bool keeps_tuning = n == "output_node_ids" || n == "shadow_exact" || n == "tune_layout" || n == "visited_direct" || n == "host_zero_copy" || n == "scan_segment_rows" ||
                            n == "filter_scan_max" || n == "filter_scan_on_overflow" || n == "launch_timing";  // (filtered launches never touch the measurements)
  // (either way the epoch goes up: the hidden lanes of the host entry point re-copy options and measurements)
  if (keeps_tuning) ix->measured.touch();
  else {
    ix->options_version++;
    ix->measured.forget();
  }
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

}  // extern "C"
#pragma GCC visibility pop
