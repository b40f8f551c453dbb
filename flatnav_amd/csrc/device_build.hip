// device_build.hip -- the device builder of the host runtime (runtime.hpp): fnv_index_insert_batch, Index::add
// (include/flatnav/index/Index.h:353-378) for a batch of new nodes -- their beams by one search launch, selectNeighbors :714-763
// and connectNeighbors :765-834 as the wire_select / wire_connect kernels of wire.hpp, the back-link requests grouped by
// target with hipcub's radix sort.  The only unit that includes hipcub.
#include <hipcub/hipcub.hpp>

#include "runtime.hpp"

namespace fnv_dev {

__global__ void iota_kernel(uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

}  // namespace fnv_dev

// Only the C ABI is exported (the library is built with -fvisibility=hidden).
#pragma GCC visibility push(default)
extern "C" {

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
  w.dispenser = ix->d_dispenser + fnv_index_s::kBuilderWord;  // (a word of the builder's own: no search launch's block)
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
    HIP_TRY(hipMemsetAsync(w.dispenser, 0, sizeof(uint32_t), ix->stream));
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

}  // extern "C"
#pragma GCC visibility pop
