// measurements.hpp -- part of the gfx950 search engine's launch planner (launch_plan.hpp includes it): the adaptive choice, in
// plain C++ (no HIP header; compiles with g++).  Two things:
//   Measurements    what a handle has measured -- the LDS layout per beam width, the best time of each kernel variant per
//                   tuner_key, the launch whose timing is still to be harvested, the row mode all of it was measured in -- and
//                   the epoch by which hidden lanes and replicas notice that it changed.  Every change is a method that keeps
//                   these consistent by itself; the host units (runtime.hpp) hold one per handle and only call it.
//   tune_layout /   fnv_tune's tournament over a measuring object: which layout wins (margin, duel, re-timing of the rules'
//   tune_variants   layout) and the variant pass on it.  tune.hip measures on the GPU; tests/test_adaptive_choice.py drives the
//                   same procedure with scripted times (tests/adaptive_choice_harness.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>

namespace fnv_dev {

// Kernel variants of one launch: 0 the exact two-heap kernel, 1 the merged-beam kernel, 2-5 the merged-beam kernel with
// the last 50 / 75 / 100 / 25 % of a round of queries sent straight to the exact search, 6 (round 4) the merged-beam kernel
// for every query plus exact shadows of the last ones on the slots the drain leaves idle (search_types.h).
constexpr int kNumVariants = 7;
constexpr int kVariantTailShadows = 6;
constexpr int kTailPct[kNumVariants] = {0, 0, 50, 75, 100, 25, 0};
inline bool variant_allowed(int v, bool multi_round, bool try_tail, bool shadows_on, bool pinned_only = false) {
  if (v < 2) return true;
  // (tail shadows: measured in round 4 -- 0.5-3 % better than the merged-beam kernel alone, behind the best exact tail on every configuration:
  //  a shadow can only start when a slot falls idle, which is too late for the ties that end a launch -- so the variant can
  //  be pinned for A/B runs but is not part of the adaptive choice)
  if (v == kVariantTailShadows) return shadows_on && pinned_only;
  return multi_round && try_tail;  // an exact tail needs more than one round of queries
}

// adaptive kernel choice ("sorted_beam" = 2): per beam width, the best time per query seen for each variant
struct Tuner {
  // ms per query: [0] two-heap kernel, [1] merged-beam kernel, [2..5] merged-beam kernel whose last 50 / 75 / 100 / 25 %
  // of a round of queries go straight to the exact search ("sorted_tail_exact_pct"; launches of more than one round)
  float best[kNumVariants] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};
  int samples[kNumVariants] = {0, 0, 0, 0, 0, 0, 0};
};
// Per beam width: the LDS layout fnv_tune measured to be the fastest (absent: the rules of configure_launch).
struct LayoutChoice {
  int cand_lds = -1;       // where the exact search keeps its candidates heap: -1 = by rule, 0 = HBM, 1 = LDS
  uint32_t vis_slots = 0;  // visited-table slots: 0 = by rule
};
// The adaptive choice keeps its measurements per (beam width, batch class: more than one round of queries or not).
inline int tuner_key(int B, bool multi_round) { return 2 * B + (multi_round ? 1 : 0); }

// What one handle has measured.  Guarded by the handle's mutex (runtime.hpp, the lock order), like the options.
//   epoch             goes up whenever a layout or a variant's time changes (and on touch()): a hidden lane or a replica that
//                     holds a copy compares the epoch it copied at and copies again when it lags.  Never the pending sample
//                     alone: that belongs to this handle's events and is not copied.
//   layouts_version   goes up whenever the layouts may have changed: the cached launch plan (launch.hip, ensure_plan) was made
//                     under one version and is made again under another.
class Measurements {
 public:
  const LayoutChoice* layout(int B) const {  // null: the rules
    const auto it = layouts_.find(B);
    return it == layouts_.end() ? nullptr : &it->second;
  }
  const Tuner* find(int key) const {  // null: nothing measured
    const auto it = tuner_.find(key);
    return it == tuner_.end() ? nullptr : &it->second;
  }
  uint64_t epoch() const { return epoch_; }
  uint64_t layouts_version() const { return layouts_version_; }
  bool has_pending() const { return pending_variant_ >= 0; }
  int measured_half() const { return measured_half_; }  // rows_changed's state: 1 / 0 the mirror's rows / the table's, -1 none yet

  // An option changed that keeps the measurements: lanes and replicas still copy again (the options travel with them).
  void touch() { epoch_++; }
  // Everything measured goes (an option that changes the plan or the kernel choice; the other row mode).
  void forget() {
    tuner_.clear();
    layouts_.clear();
    changed(true);
  }
  // fnv_tune, before its probe: what was measured for beam width B, and nothing else.
  void forget(int B) {
    layouts_.erase(B);
    tuner_.erase(tuner_key(B, false));
    tuner_.erase(tuner_key(B, true));
    epoch_++;
    layouts_version_++;
  }
  // The layout of beam width B: `lc`, or the rules again (null).
  void set_layout(int B, const LayoutChoice* lc) {
    if (lc) layouts_[B] = *lc;
    else layouts_.erase(B);
    epoch_++;
    layouts_version_++;
  }
  // A finished variant pass of fnv_tune.  (ev0 / ev1 bracketed its launches: no sample is pending any more.)
  void settle(int key, const Tuner& t) {
    tuner_[key] = t;
    changed(false);
  }
  // The rows this launch reads: the half-width mirror's or the table's.  Launches with and without the mirror run different
  // kernels, so what was measured in the other mode is discarded; true: it was (the first call has nothing to discard).
  bool rows_changed(bool half_rows) {
    const bool flipped = measured_half_ >= 0 && measured_half_ != (int)half_rows;
    if (flipped) forget();
    measured_half_ = (int)half_rows;
    return flipped;
  }
  // The launch just enqueued between the handle's events is a sample of `variant` for `key`, over `nq` queries ...
  void expect(int key, int variant, uint64_t nq) {
    pending_key_ = key;
    pending_variant_ = variant;
    pending_nq_ = nq;
  }
  // ... or the events bracket something else.
  void drop_pending() { pending_variant_ = -1; }
  // The pending sample's events were found complete after `ms` (<= 0: no time could be read).  The best of a variant is the
  // minimum per query; a sample is used once.
  void harvest(float ms) {
    if (pending_variant_ < 0) return;
    if (ms > 0.f) {
      Tuner& t = tuner_[pending_key_];
      const float per_q = ms / (float)pending_nq_;
      if (t.samples[pending_variant_] == 0 || per_q < t.best[pending_variant_]) t.best[pending_variant_] = per_q;
      t.samples[pending_variant_]++;
      epoch_++;
    }
    pending_variant_ = -1;
  }
  // Take over what `src` measured (a hidden lane from its owner, a replica from its source): everything on the same GPU
  // model; another model starts empty and measures for itself.  This handle's own pending sample is dropped either way.
  void copy_from(const Measurements& src, bool same_model) {
    if (same_model) {
      tuner_ = src.tuner_;
      layouts_ = src.layouts_;
      measured_half_ = src.measured_half_;
    } else {
      tuner_.clear();
      layouts_.clear();
      measured_half_ = -1;
    }
    changed(true);
  }

 private:
  void changed(bool layouts_too) {
    pending_variant_ = -1;
    epoch_++;
    if (layouts_too) layouts_version_++;
  }
  std::map<int, LayoutChoice> layouts_;  // per beam width
  std::map<int, Tuner> tuner_;           // per tuner_key
  int pending_key_ = 0, pending_variant_ = -1;  // the launch between ev0 / ev1 is a sample for this entry (-1: it is not)
  uint64_t pending_nq_ = 0;
  int measured_half_ = -1;
  uint64_t epoch_ = 0, layouts_version_ = 0;
};

// ---- fnv_tune's tournament ------------------------------------------------------------------------------------------
// Over a measuring object `m` (tune.hip: launches on the GPU; the CPU tests: scripted times):
//   int  m.time(variant, reps, &ms_per_query)   mean of `reps` timed launches of one variant under the layout in use (0: done)
//   void m.use_layout(index)                    candidate `index` is the layout of the launches that follow (0: the rules')
//   bool m.multi_round()                        ... and under it the batch is more than one round of the merged-beam kernel's slots
//   void m.log_layout(index, t1, t4) / m.log_duel(rounds, challenger, sum_c, holder, sum_b, wins) / m.log_variant(v, t)
// Every comparison is in float, a failed measurement never wins.

// 1. The LDS layout.  Resident queries, visited-table slots and the LDS home of the exact search's candidates heap trade
// against each other, and which trade wins depends on the data (how often queries tie, how many ids a query visits): rules
// cover the common cases (configure_launch), this measures the neighbours of the rules' choice (tune_layout_candidates, in
// that order) -- each with the merged-beam kernel alone and with 75 % of its last round straight to the exact search, the
// better of the two counting -- and returns the index of the fastest.
template <class Meter>
inline size_t tune_layout(Meter& m, size_t n_cands, bool try_tail) {
  auto time_layout = [&](size_t li, float* out) -> int {
    m.use_layout(li);
    float t1 = -1.f, t4 = -1.f;
    int r = m.time(1, 4, &t1);
    if (r) return r;
    if (m.multi_round() && try_tail && (r = m.time(3, 4, &t4)) != 0) return r;
    *out = (t4 > 0.f && t4 < t1) ? t4 : t1;
    m.log_layout(li, t1, t4);
    return 0;
  };
  size_t best_layout = 0;
  float best_layout_t = -1.f;
  bool won_by_duel = false;
  for (size_t li = 0; li < n_cands; li++) {
    float t = -1.f;
    if (time_layout(li, &t) != 0) continue;  // e.g. a layout that does not fit LDS: not a candidate
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
        if (time_layout(best_layout, &tb) != 0 || time_layout(li, &tc) != 0) wins = false;
        else wins = tc < tb * 0.99f;
        sum_b += tb;
        sum_c += tc;
      }
      m.log_duel(rounds, li, sum_c, best_layout, sum_b, wins);
      if (wins) {
        best_layout_t = sum_c / (float)rounds;
        best_layout = li;
        won_by_duel = true;
      }
    }
  }
  if (best_layout != 0 && !won_by_duel) {  // a neighbour won on one measurement: the rules' layout was timed first, so it is timed once more, now last
    float again = -1.f;
    if (time_layout(0, &again) == 0 && !(best_layout_t < again * 0.95f)) best_layout = 0;
  }
  return best_layout;
}

// 2. The kernel variant on that layout: every variant the adaptive choice would try, in ordinal order; the first failure ends it.
template <class Meter>
inline int tune_variants(Meter& m, bool multi_round, bool try_tail, bool shadows_on, Tuner* t) {
  for (int v = 0; v < kNumVariants; v++) {
    if (!variant_allowed(v, multi_round, try_tail, shadows_on)) continue;
    if (const int rc = m.time(v, 4, &t->best[v])) return rc;
    m.log_variant(v, t->best[v]);
    t->samples[v] = 4;  // settled: later launches neither explore nor sample
  }
  return 0;
}

}  // namespace fnv_dev
