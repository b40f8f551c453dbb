// adaptive_choice_harness.cpp -- test infrastructure (tests/test_adaptive_choice.py and tests/test_gpu_tune_replay.py compile it
// with g++ and load it with ctypes; the product never does): the adaptive choice of flatnav_amd/csrc/measurements.hpp on the
// CPU -- the class Measurements call by call, and fnv_tune's tournament over a measuring object whose times come from a script.
#include <deque>
#include <map>
#include <utility>
#include <vector>

#include "../flatnav_amd/csrc/launch_plan.hpp"

using namespace fnv_dev;

namespace {

// The scripted measuring object: per (layout, variant) a queue of (rc, ms per query), so that repeated measurements of one
// layout can differ; per layout whether the batch is more than one round.  Every request is recorded: rows of four ints
// {kind, a, b, c} and two floats.
//   0 use_layout(a)            1 time(variant b, reps c) under layout a; floats: the answer's ms and rc
//   2 log_layout(a; t1, t4)    3 log_duel(challenger a, holder b, rounds c, negative when the holder stays; sum_c, sum_b)
//   4 log_variant(a; t)
constexpr int kExhausted = -999;  // a request the script has no answer for
struct Scripted {
  std::map<std::pair<int, int>, std::deque<std::pair<int, float>>> queues;
  std::vector<int> multi;
  std::vector<int32_t> ints;
  std::vector<float> floats;
  int layout = -1;
  bool exhausted = false;
  void record(int kind, int a, int b, int c, float x, float y) {
    for (int v : {kind, a, b, c}) ints.push_back(v);
    floats.push_back(x);
    floats.push_back(y);
  }
  int time(int v, int reps, float* out) {
    auto& q = queues[{layout, v}];
    int rc = kExhausted;
    float ms = 0.f;
    if (q.empty()) exhausted = true;
    else rc = q.front().first, ms = q.front().second, q.pop_front();
    record(1, layout, v, reps, ms, (float)rc);
    if (rc == 0) *out = ms;
    return rc;
  }
  void use_layout(size_t li) {
    layout = (int)li;
    record(0, layout, 0, 0, 0.f, 0.f);
  }
  bool multi_round() const { return multi[(size_t)layout] != 0; }
  void log_layout(size_t li, float t1, float t4) { record(2, (int)li, 0, 0, t1, t4); }
  void log_duel(int rounds, size_t li, float sum_c, size_t holder, float sum_b, bool wins) {
    record(3, (int)li, (int)holder, wins ? rounds : -rounds, sum_c, sum_b);
  }
  void log_variant(int v, float t) { record(4, v, 0, 0, t, 0.f); }
};

}  // namespace

extern "C" {

// ---- the class ------------------------------------------------------------------------------------------------------
void* ach_new() { return new Measurements(); }
void ach_free(void* m) { delete (Measurements*)m; }
void ach_touch(void* m) { ((Measurements*)m)->touch(); }
void ach_forget(void* m) { ((Measurements*)m)->forget(); }
void ach_forget_beam(void* m, int B) { ((Measurements*)m)->forget(B); }
void ach_set_layout(void* m, int B, int install, int cand_lds, uint32_t vis_slots) {
  LayoutChoice lc;
  lc.cand_lds = cand_lds;
  lc.vis_slots = vis_slots;
  ((Measurements*)m)->set_layout(B, install ? &lc : nullptr);
}
void ach_settle(void* m, int key, const float* best, const int* samples) {
  Tuner t;
  for (int v = 0; v < kNumVariants; v++) t.best[v] = best[v], t.samples[v] = samples[v];
  ((Measurements*)m)->settle(key, t);
}
int ach_rows_changed(void* m, int half_rows) { return ((Measurements*)m)->rows_changed(half_rows != 0); }
void ach_expect(void* m, int key, int variant, uint64_t nq) { ((Measurements*)m)->expect(key, variant, nq); }
void ach_drop_pending(void* m) { ((Measurements*)m)->drop_pending(); }
void ach_harvest(void* m, float ms) { ((Measurements*)m)->harvest(ms); }
void ach_copy_from(void* m, const void* src, int same_model) { ((Measurements*)m)->copy_from(*(const Measurements*)src, same_model != 0); }
// reads.  state: epoch, layouts_version, has_pending, measured_half
void ach_state(const void* m, int64_t* out) {
  const Measurements* s = (const Measurements*)m;
  out[0] = (int64_t)s->epoch(), out[1] = (int64_t)s->layouts_version(), out[2] = s->has_pending(), out[3] = s->measured_half();
}
int ach_layout(const void* m, int B, int64_t* out) {
  const LayoutChoice* lc = ((const Measurements*)m)->layout(B);
  if (lc) out[0] = lc->cand_lds, out[1] = lc->vis_slots;
  return lc != nullptr;
}
int ach_find(const void* m, int key, float* best, int* samples) {
  const Tuner* t = ((const Measurements*)m)->find(key);
  for (int v = 0; t && v < kNumVariants; v++) best[v] = t->best[v], samples[v] = t->samples[v];
  return t != nullptr;
}
int ach_tuner_key(int B, int multi_round) { return tuner_key(B, multi_round != 0); }
int ach_num_variants() { return kNumVariants; }

// ---- the tournament -------------------------------------------------------------------------------------------------
// fnv_tune's steps 1 and 2 as tune.hip runs them (tune_layout, the winner installed, tune_variants under it), over `n_script`
// scripted answers {layout, variant, rc} with their ms in `script_ms`, each appended to its (layout, variant) queue, and
// multi[n_cands].  Fills the trace (at most max_rows rows; returns the rows there were) and result: {layout, rc, multi_round,
// the script ran dry, owner_final_variant of the Tuner (-1 when rc != 0)}, best[7], samples[7].
int ach_tournament(int n_cands, const int* multi, int try_tail, int shadows_on, const int32_t* script, const float* script_ms, int n_script,
                   int32_t* trace_ints, float* trace_floats, int max_rows, int32_t* result, float* best, int* samples) {
  Scripted m;
  m.multi.assign(multi, multi + n_cands);
  for (int i = 0; i < n_script; i++) m.queues[{script[3 * i], script[3 * i + 1]}].push_back({script[3 * i + 2], script_ms[i]});
  const size_t winner = tune_layout(m, (size_t)n_cands, try_tail != 0);
  m.use_layout(winner);
  const bool multi_round = m.multi_round();
  Tuner t;
  const int rc = tune_variants(m, multi_round, try_tail != 0, shadows_on != 0, &t);
  result[0] = (int32_t)winner, result[1] = rc, result[2] = multi_round, result[3] = m.exhausted;
  result[4] = rc ? -1 : owner_final_variant(t, multi_round, try_tail != 0, shadows_on != 0);
  for (int v = 0; v < kNumVariants; v++) best[v] = t.best[v], samples[v] = t.samples[v];
  const int rows = (int)(m.ints.size() / 4);
  for (int i = 0; i < rows && i < max_rows; i++) {
    for (int j = 0; j < 4; j++) trace_ints[4 * i + j] = m.ints[4 * (size_t)i + j];
    for (int j = 0; j < 2; j++) trace_floats[2 * i + j] = m.floats[2 * (size_t)i + j];
  }
  return rows;
}

}  // extern "C"
