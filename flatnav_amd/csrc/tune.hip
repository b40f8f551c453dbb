// tune.hip -- measuring and reporting calls of the host runtime (runtime.hpp): fnv_tune (the adaptive kernel choice and the
// LDS layout, taken in one go), the gather ceiling, the developer builds' debug calls and what the fnv_last_* calls report
// of the most recent launch -- with the measurement kernels only these launch.
#include "runtime.hpp"

namespace fnv_dev {

#if defined(FNV_PHASE_TIMING) || defined(FNV_MICROBENCH)
// Developer micro-benchmark (profiling builds only): cycles per cooperative heap operation on an
// LDS heap of `size` entries, `blocks` single-wave workgroups running concurrently.
__global__ __launch_bounds__(WAVE) void heap_microbench_kernel(int size, int iters, unsigned long long* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  LdsHeap h{reinterpret_cast<unsigned long long*>(smem + 8)};
  PhaseTimer ph;
  ph.start();
  uint32_t rng = 12345u + blockIdx.x;
  int n = 0;
  for (int i = 0; i < size; i++) {
    rng = rng * 1664525u + 1013904223u;
    coop_push(h, n, fnv_stl::Entry{(float)(rng >> 8), (uint32_t)i}, lane, ph, 15);
    n++;
  }
  __syncthreads();
  unsigned long long t0 = clock64();
  for (int it = 0; it < iters; it++) {
    rng = rng * 1664525u + 1013904223u;
    coop_push(h, n, fnv_stl::Entry{(float)(rng >> 8), (uint32_t)it}, lane, ph, 15);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  unsigned long long t1 = clock64();
  for (int it = 0; it < iters; it++) {
    coop_pop<true>(h, n + 1, lane, ph, 12);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  unsigned long long t2 = clock64();
  // plain dependent LDS round trips for reference
  int idx = lane;
  for (int it = 0; it < iters; it++) idx = (int)(h.p[idx & 63] & 63);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  unsigned long long t3 = clock64();
  if (lane == 0 && blockIdx.x == 0) {
    out[0] = (t1 - t0) / iters;
    out[1] = (t2 - t1) / iters;
    out[2] = (t3 - t2) / iters;
    out[3] = (unsigned long long)idx;
  }
}
#endif

// ---------------------------------------------------------------------------------------------
// Gather ceiling (measurement aid, fnv_gather_ceiling): what the search kernel's access pattern reaches on THIS index's
// vector table with no other work -- random rows, read as 16-byte chunks by G-lane groups (whole 128-byte lines),
// PU x CU loads in flight per lane, exactly the (G, CU, passes) the search kernel uses for this row width.  The rate
// it reaches is the practical bound of roofline.achieved for this (row bytes, table size): part of a small table is
// served by the 256 MiB Infinity Cache, rows that are not whole lines pay for the lines they straddle.
// ---------------------------------------------------------------------------------------------
template <int G, int CU>
__global__ __launch_bounds__(WAVE) void gather_ceiling_kernel(const uint8_t* __restrict__ base, uint64_t n_rows,
                                                              uint32_t row_bytes, int iters, uint32_t* out) {
  constexpr int PU = passes<G, CU>();
  const int lane = threadIdx.x, g = lane % G;
  uint32_t rng = (blockIdx.x * WAVE + lane / G * G) * 2654435761u + 12345u;  // same within a G-lane group
  uint32_t acc = 0;
  const int nchunks = (int)(row_bytes / 16);
  for (int it = 0; it < iters; it++) {
    const uint8_t* rowp[PU];
#pragma unroll
    for (int pu = 0; pu < PU; pu++) {
      rng = rng * 1664525u + 1013904223u;
      const uint64_t row = ((uint64_t)(rng >> 4) * n_rows) >> 28;
      rowp[pu] = base + row * row_bytes;
    }
    for (int c0 = 0; c0 < nchunks; c0 += G * CU) {
      uint4 y[PU][CU];
#pragma unroll
      for (int pu = 0; pu < PU; pu++)
#pragma unroll
        for (int cu = 0; cu < CU; cu++) {
          const int c = c0 + cu * G + g;
          y[pu][cu] = *reinterpret_cast<const uint4*>(rowp[pu] + (uint32_t)(c < nchunks ? c : nchunks - 1) * 16u);
        }
#pragma unroll
      for (int pu = 0; pu < PU; pu++)
#pragma unroll
        for (int cu = 0; cu < CU; cu++) acc ^= y[pu][cu].x ^ y[pu][cu].y ^ y[pu][cu].z ^ y[pu][cu].w;
    }
  }
  if (acc == 0x12345678u) out[0] = acc;
}

}  // namespace fnv_dev

// The handle whose events / counters describe the most recent launch of `ix`: a hidden lane if that served the last host-buffer call.
static fnv_index_s* last_launcher(fnv_index_t ix) {
  fnv_index_s* lane = ix->last_served.load();
  return lane ? lane : ix;
}

// What fnv_tune measures with: its launches on the handle's stream, their times, the candidate layouts, the log.  The
// tournament itself -- which layout wins, then the variant pass on it -- is tune_layout / tune_variants (measurements.hpp)
// over this object.
struct TuneMeter {
  fnv_index_s* ix;
  // The batch twice in a row: a launch on rows [off, off + nq) searches the same queries in a rotated order.  Which
  // queries tie -- and so which ones are stragglers of the last round -- is a property of the queries: timing several
  // rotations and averaging measures a variant's EXPECTED time, not its luck with one order.
  const uint8_t* dq2;
  uint64_t nq;
  int K, ef_search, num_initializations;
  SearchOutputs scratch;  // distances | labels, nothing else
  const int B = std::max(ef_search, K);
  std::vector<LayoutChoice> cands{1};  // [0]: the rules' (fnv_tune adds their neighbours once the probing launch has planned)
  const bool tune_log = getenv("FLATNAV_TUNE_LOG") != nullptr;  // developer aid: every measurement on stderr
  int launch(int variant, uint64_t rotate = 0) {
    SearchOptions opt;
    opt.force_variant = variant;
    opt.timed = true;  // (time reads ev0 / ev1)
    const size_t qrow_bytes = (size_t)ix->dim * dtype_size(ix->dtype);
    return search_device_impl(ix, dq2 + (rotate % nq) * qrow_bytes, nq, K, ef_search, num_initializations, scratch, ix->stream, opt);
  }
  // Every timed launch starts from cold caches: the SAME queries visit the same nodes launch after launch, so the index
  // rows and -- above all -- the words of the per-slot HBM visited bitmaps they touch would sit in the 256 MiB Infinity
  // Cache by the second launch, which flatters exactly the layouts that spill most (small visited tables); a caller's
  // consecutive batches are different queries.  (Measured: without this the layout choice for 100-d rows at ef=200
  // flipped between boxes to a 4096-slot table that is 10 % slower under the bench protocol.)
  struct Flush {
    void* p = nullptr;
    size_t bytes = 768u << 20;
    void open() {
      const char* flush_env = getenv("FLATNAV_TUNE_FLUSH");  // developer knob: 0 = time warm launches
      if (flush_env && flush_env[0] == '0') p = nullptr;
      else if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;  // (no room: tune warm, as before)
      (void)hipGetLastError();
    }
    ~Flush() { if (p) (void)hipFree(p); }
  } flush;
  // mean of `reps` timed launches of one variant, each on another rotation of the batch (after a cold launch), ms per query
  int time(int v, int reps, float* out) {
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
  }
  void use_layout(size_t li) {
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->measured.set_layout(B, li == 0 ? nullptr : &cands[li]);
  }
  bool multi_round() const { return multi_round_launch(ix, ix->plan, nq); }
  // (each line ends with the per-query values it compared as hex floats: a replay is exact, not rounded to four decimals)
  void log_layout(size_t li, float t1, float t4) const {
    if (tune_log)
      fprintf(stderr, "fnv_tune B=%d layout %zu (heap in LDS %d, table %u): merged %.4f ms, 75%% tail exact %.4f ms -> %u slots, %d per CU [%a %a, %u heap entries]\n", B,
              li, (int)cands[li].cand_lds, cands[li].vis_slots, t1 * (float)nq, t4 * (float)nq, (unsigned)ix->geom[4], (int)ix->geom[3], t1, t4, (unsigned)ix->geom[5]);
  }
  void log_duel(int rounds, size_t li, float sum_c, size_t holder, float sum_b, bool wins) const {
    if (tune_log) fprintf(stderr, "fnv_tune B=%d duel (%d round%s): layout %zu %.4f ms against layout %zu %.4f ms -> %s [%a %a]\n", B, rounds, rounds == 1 ? "" : "s",
                          li, sum_c / (float)rounds * (float)nq, holder, sum_b / (float)rounds * (float)nq,
                          wins ? "challenger" : "holder", sum_c / (float)rounds, sum_b / (float)rounds);
  }
  void log_variant(int v, float t) const {
    if (tune_log) fprintf(stderr, "fnv_tune B=%d variant %d: %.4f ms [%a]\n", B, v, t * (float)nq, t);
  }
};

// Only the C ABI is exported (the library is built with -fvisibility=hidden).
#pragma GCC visibility push(default)
extern "C" {

// ---- the adaptive kernel choice, taken in one go --------------------------------------------------------------------
// Runs every variant the adaptive choice ("sorted_beam" = 2) would try for this (beam width, batch size class) on the
// caller's queries -- a cold launch plus three timed ones each -- and settles the choice, so that the caller's own
// launches never are exploratory ones.  Results are discarded (scratch buffers of the index).
int fnv_tune(fnv_index_t ix, const void* queries, uint64_t nq, int queries_on_device, int K, int ef_search,
             int num_initializations) {
  if (!ix) return fail(FNV_ERR_INVALID, "index is null");
  if (int rc = check_search_sizes(K, ef_search, num_initializations)) return rc;
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
  uint8_t* dq2 = ix->d_q.as<uint8_t>();  // (the batch twice in a row: TuneMeter)
  HIP_TRY(hipMemcpy(dq2, queries, qbytes, queries_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dq2 + qbytes, dq2, qbytes, hipMemcpyDeviceToDevice));
  SearchOutputs scratch;
  scratch.dist = ix->d_out.as<float>();
  scratch.labels = (int32_t*)(ix->d_out.as<uint8_t>() + o_lab);
  TuneMeter gpu{ix, dq2, nq, K, ef_search, num_initializations, scratch};
  // what kind of launch is this?  (one probing launch of the merged-beam kernel tells: plan, round size)
  const int B = gpu.B;
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->measured.forget(B);  // (whatever follows -- including the early return below -- lanes drop their copy of the old choice)
  }
  int rc = gpu.launch(1);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ix->stream));
  if (ix->geom[6] == MODE_HEAPS || ix->sorted_beam != 2 || ix->sorted_variant >= 0 || nq < 2048) return FNV_OK;  // nothing to choose
  // (from the plan, not from the probing launch's geometry record: a DIRECT launch reports its bitmap's bits there)
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    const SearchParams& rules = ix->plan.sorted;
    gpu.cands = tune_layout_candidates(ix, rules.vis_slots, rules.vis_w, rules.cand_slots != 0);
  }
  gpu.flush.open();
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
      if (gpu.time(1, 1, &t) != FNV_OK) break;
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
      if (gpu.tune_log) fprintf(stderr, "fnv_tune B=%d settling: %.4f ms (at %.2f s)\n", B, t * (float)nq, waited);
      if ((waited > 0.5 && prev > 0.f && fabsf(t - prev) < 0.02f * prev) || waited > 2.0) break;
      prev = t;
    }
  }
  // ---- 1. the LDS layout
  const bool try_tail = ix->sorted_tail_exact_pct < 0;
  gpu.use_layout(tune_layout(gpu, gpu.cands.size(), try_tail));
  rc = gpu.launch(1);  // re-plan with the chosen layout
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ix->stream));
  // ---- 2. the kernel variant on that layout
  const bool multi_round = gpu.multi_round();
  Tuner t;
  rc = tune_variants(gpu, multi_round, try_tail, ix->shadow_exact != 0, &t);
  if (rc) return rc;
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->measured.settle(tuner_key(B, multi_round), t);
  }
  return check_device_status(ix);
}

// Measurement aid: the rate (GB/s of row bytes) a pure gather of random rows of this index's vector table reaches with
// the search kernel's own load pattern for this row width (gather_ceiling_kernel, above) at `waves_per_cu`
// resident waves (0: 16).  ~20-40 ms of GPU time.
int fnv_gather_ceiling(fnv_index_t ix, int waves_per_cu, double* gbps_out) {
  if (!ix || !gbps_out) return fail(FNV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(ix->mu);
  ON_DEVICE(ix->device);
  const uint64_t n_rows = live_nodes(ix);
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
  uint32_t* d_sink = ix->d_dispenser + fnv_index_s::kBuilderWord + 1;  // an unused word of the workspace
  hipLaunchKernelGGL(kGather[cfg], dim3(blocks), dim3(WAVE), 0, ix->stream, ix->d_vectors, n_rows, ix->row_bytes, iters / 8 + 1, d_sink);  // warm
  HIP_TRY(hipEventRecord(ix->ev0, ix->stream));
  hipLaunchKernelGGL(kGather[cfg], dim3(blocks), dim3(WAVE), 0, ix->stream, ix->d_vectors, n_rows, ix->row_bytes, iters, d_sink);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ix->ev1, ix->stream));
  HIP_TRY(hipEventSynchronize(ix->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
  ix->measured.drop_pending();  // ev0 / ev1 no longer bracket a search launch
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

int fnv_last_kernel_ms(fnv_index_t ix, float* ms) {
  if (!ix || !ms) return fail(FNV_ERR_INVALID, "null argument");
  // ev0 / ev1 bracket a launch only where somebody reads them (runtime.hpp, time_launches): asking arms the handle's
  // device-buffer launches from here on; the launch that was not timed has no duration to report
  ix->time_launches = true;
  ix = last_launcher(ix);
  if (!ix->launched) return fail(FNV_ERR_RUNTIME, "no search has been launched on this index");
  if (!ix->last_timed)
    return fail(FNV_ERR_RUNTIME, "the most recent launch was not timed: fnv_search_batch_device records its events once \"launch_timing\" is set "
                                 "or fnv_last_kernel_ms has been called (timing is armed for the launches that follow)");
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
  HIP_TRY(hipMemcpy(w, ix->last_block + 11, sizeof(w), hipMemcpyDeviceToHost));
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
  HIP_TRY(hipMemcpy(w, ix->last_block + 3, sizeof(w), hipMemcpyDeviceToHost));  // (the most recent launch's block)
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
  HIP_TRY(hipMemcpy(w, ix->last_block + 3, sizeof(w), hipMemcpyDeviceToHost));
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
