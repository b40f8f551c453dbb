"""The adaptive choice (flatnav_amd/csrc/measurements.hpp) on the CPU: tests/adaptive_choice_harness.cpp is compiled with g++
and loaded with ctypes.

Two things are held.  The class Measurements -- what a handle has measured -- keeps its own invariants: the epoch by which
hidden lanes and replicas notice a change, the version by which the cached launch plan notices a changed layout, the pending
sample.  And fnv_tune's tournament (tune_layout / tune_variants) asks for exactly the measurements, in exactly the order, and
lands on exactly the layout and times that the procedure written out in fnv_tune did: named cases around every threshold, and
`model` below -- that procedure restated in numpy.float32 from tune.hip as it was before the tournament left it -- against the
C++ on random scripts of times drawn from around the thresholds, exact equalities included."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "adaptive_choice_harness.cpp")
F = np.float32
NV = 7  # kNumVariants
EXHAUSTED = -999  # the harness's answer to a request its script does not cover
USE, TIME, LOG_LAYOUT, LOG_DUEL, LOG_VARIANT = range(5)  # the kinds of a trace row
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="flatnav_adaptive_choice_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libadaptive_choice_harness.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.ach_new.restype = C.c_void_p
        for name, args in dict(ach_free=[], ach_touch=[], ach_forget=[], ach_forget_beam=[C.c_int],
                               ach_set_layout=[C.c_int, C.c_int, C.c_int, C.c_uint32], ach_settle=[C.c_int, C.c_void_p, C.c_void_p],
                               ach_rows_changed=[C.c_int], ach_expect=[C.c_int, C.c_int, C.c_uint64], ach_drop_pending=[],
                               ach_harvest=[C.c_float], ach_copy_from=[C.c_void_p, C.c_int], ach_state=[C.c_void_p],
                               ach_layout=[C.c_int, C.c_void_p], ach_find=[C.c_int, C.c_void_p, C.c_void_p]).items():
            getattr(L, name).argtypes = [C.c_void_p] + args
        L.ach_tournament.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.ach_num_variants() == NV
        _lib = L
    return _lib


# ---- the class ------------------------------------------------------------------------------------------------------
class Measurements:
    """One Measurements object of the harness."""

    def __init__(self):
        self.h = lib().ach_new()

    def __del__(self):
        lib().ach_free(self.h)

    def __getattr__(self, name):  # the mutators, by their C++ names
        f = getattr(lib(), "ach_" + name)
        return lambda *a: f(self.h, *a)

    def settle(self, key, best, samples):
        b, s = np.asarray(best, np.float32), np.asarray(samples, np.int32)
        lib().ach_settle(self.h, key, b.ctypes.data, s.ctypes.data)

    def copy_from(self, src, same_model):
        lib().ach_copy_from(self.h, src.h, int(same_model))

    def state(self):
        out = np.zeros(4, np.int64)
        lib().ach_state(self.h, out.ctypes.data)
        return dict(zip(("epoch", "layouts_version", "pending", "measured_half"), (int(v) for v in out)))

    def layout(self, B):
        out = np.zeros(2, np.int64)
        return (int(out[0]), int(out[1])) if lib().ach_layout(self.h, B, out.ctypes.data) else None

    def find(self, key):
        b, s = np.zeros(NV, np.float32), np.zeros(NV, np.int32)
        return (b.tolist(), s.tolist()) if lib().ach_find(self.h, key, b.ctypes.data, s.ctypes.data) else None


def key(B, multi_round):
    return lib().ach_tuner_key(B, int(multi_round))


SETTLED = ([0.5, 0.25, -1, 0.125, -1, -1, -1], [4, 4, 0, 4, 0, 0, 0])


def measured(beams=(64, 100)):
    m = Measurements()
    for B in beams:
        m.set_layout(B, 1, 1, 3072 + B)
        m.settle(key(B, True), *SETTLED)
        m.settle(key(B, False), *SETTLED)
    return m


def test_the_epoch_goes_up_on_every_change_and_never_down():
    """Every method that changes what a lane or a replica would copy -- and touch(), for the options that travel with it --
    raises the epoch.  The pending sample is this handle's own (its events): arming or dropping it leaves the epoch alone."""
    m, other = Measurements(), measured()
    m.rows_changed(0)
    changes = [lambda: m.touch(), lambda: m.set_layout(64, 1, 0, 4096), lambda: m.set_layout(64, 1, 1, 4096),
               lambda: m.set_layout(64, 0, 0, 0), lambda: m.settle(key(64, True), *SETTLED), lambda: m.forget_beam(64),
               lambda: (m.expect(key(64, True), 1, 4096), m.harvest(2.0)), lambda: m.rows_changed(1), lambda: m.forget(),
               lambda: m.copy_from(other, True), lambda: m.copy_from(other, False)]
    for i, change in enumerate(changes):
        before = m.state()["epoch"]
        change()
        assert m.state()["epoch"] > before, i
    for quiet in (lambda: m.expect(key(64, True), 1, 4096), lambda: m.drop_pending(), lambda: m.harvest(0.0), lambda: m.rows_changed(1)):
        before = m.state()["epoch"]
        quiet()
        assert m.state()["epoch"] == before


def test_forget_of_one_beam_width_leaves_the_others_alone():
    m = measured((64, 100))
    m.expect(key(100, True), 1, 4096)
    m.forget_beam(64)
    assert m.layout(64) is None and m.find(key(64, True)) is None and m.find(key(64, False)) is None
    assert m.layout(100) == (1, 3172) and m.find(key(100, True)) == SETTLED and m.find(key(100, False)) == SETTLED
    assert m.state()["pending"] == 1 and m.state()["measured_half"] == -1  # "and nothing else"
    m.forget()
    assert m.layout(100) is None and m.find(key(100, True)) is None and m.state()["pending"] == 0


def test_rows_changed_discards_on_a_flip_only():
    for first in (0, 1):
        m = measured()
        assert m.rows_changed(first) == 0 and m.layout(64) is not None  # the first call: nothing to discard
        assert m.rows_changed(first) == 0 and m.find(key(64, True)) == SETTLED
        m.expect(key(64, True), 1, 4096)
        v = m.state()["layouts_version"]
        assert m.rows_changed(1 - first) == 1
        s = m.state()
        assert m.layout(64) is None and m.find(key(64, True)) is None and m.layout(100) is None
        assert s["pending"] == 0 and s["layouts_version"] > v and s["measured_half"] == 1 - first
        assert m.rows_changed(1 - first) == 0


def test_harvest_keeps_the_minimum_and_counts_samples():
    m = Measurements()
    k = key(64, True)
    for i, (ms, best) in enumerate([(8.0, 8.0), (12.0, 8.0), (4.0, 4.0)]):
        m.expect(k, 3, 4096)
        assert m.state()["pending"] == 1
        m.harvest(ms)
        b, s = m.find(k)
        assert b[3] == float(F(best) / F(4096)) and s[3] == i + 1 and m.state()["pending"] == 0
        assert s[:3] + s[4:] == [0] * 6 and b[1] == -1.0
    m.harvest(1.0)  # nothing pending: nothing happens
    assert m.find(k)[1][3] == 3
    m.expect(key(100, False), 0, 2048)  # the first sample of an entry that does not exist yet
    m.harvest(1.0)
    assert m.find(key(100, False))[1] == [1, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("ms", [0.0, -1.0])
def test_harvest_ignores_a_time_that_is_not_positive_but_drops_the_sample(ms):
    m = Measurements()
    m.expect(key(64, True), 1, 4096)
    before = m.state()
    m.harvest(ms)
    assert m.find(key(64, True)) is None and m.state() == dict(before, pending=0)


def test_copy_from_the_same_model_and_from_another():
    src = measured()
    src.rows_changed(1)
    for same in (True, False):
        dst = measured((32,))
        dst.rows_changed(0)
        dst.expect(key(32, True), 1, 4096)
        before = dst.state()
        dst.copy_from(src, same)
        s = dst.state()
        assert s["pending"] == 0 and s["epoch"] > before["epoch"] and s["layouts_version"] > before["layouts_version"]
        assert dst.layout(32) is None and dst.find(key(32, True)) is None  # what it held is gone either way
        for B in (64, 100):
            assert dst.layout(B) == (src.layout(B) if same else None)
            for multi in (False, True):
                assert dst.find(key(B, multi)) == (src.find(key(B, multi)) if same else None)
        assert s["measured_half"] == (1 if same else -1)
    assert src.layout(64) == (1, 3136) and src.find(key(64, True)) == SETTLED  # the source is only read


def test_the_layouts_version_changes_with_every_installed_replaced_or_erased_layout():
    m = Measurements()
    seen = [m.state()["layouts_version"]]
    for install, lds, slots in [(1, 1, 4096), (1, 1, 6144), (1, 0, 6144), (0, 0, 0)]:
        m.set_layout(64, install, lds, slots)
        assert m.layout(64) == ((lds, slots) if install else None)
        seen.append(m.state()["layouts_version"])
    m.set_layout(64, 1, 1, 4096)
    for drop in (lambda: m.forget_beam(64), lambda: (m.set_layout(64, 1, 1, 4096), m.forget())[0]):
        drop()
        assert m.layout(64) is None
        seen.append(m.state()["layouts_version"])
    assert all(b > a for a, b in zip(seen, seen[1:])), seen
    # ... and with nothing else: a steady-state launch (arm, harvest, the same rows again) never plans again
    m.rows_changed(0)
    v = m.state()["layouts_version"]
    for _ in range(3):
        m.expect(key(64, True), 1, 4096)
        m.harvest(1.0)
        m.touch()
        m.drop_pending()
        m.settle(key(64, True), *SETTLED)
        assert m.rows_changed(0) == 0
    assert m.state()["layouts_version"] == v


# ---- the tournament -------------------------------------------------------------------------------------------------
def tournament(n_cands, multi, try_tail, shadows_on, layouts, variants, rcs, ms):
    """fnv_tune's steps 1 and 2 in C++ over a script: answer i is for (layouts[i], variants[i]) -- the answers of one pair
    form its queue, in this order -- and is (rcs[i], ms[i]).  -> (trace rows [(kind, a, b, c, float bits, float bits)], result)."""
    layouts, variants, rcs = (np.asarray(a, np.int32) for a in (layouts, variants, rcs))
    script = np.ascontiguousarray(np.stack([layouts, variants, rcs], axis=1)) if len(layouts) else np.zeros((0, 3), np.int32)
    ms = np.ascontiguousarray(ms, np.float32)
    multi = np.ascontiguousarray(multi, np.int32)
    cap = 4096
    ti, tf = np.zeros((cap, 4), np.int32), np.zeros((cap, 2), np.float32)
    res, best, samples = np.zeros(5, np.int32), np.zeros(NV, np.float32), np.zeros(NV, np.int32)
    rows = lib().ach_tournament(n_cands, multi.ctypes.data, int(try_tail), int(shadows_on), script.ctypes.data, ms.ctypes.data, len(ms),
                                ti.ctypes.data, tf.ctypes.data, cap, res.ctypes.data, best.ctypes.data, samples.ctypes.data)
    assert rows <= cap
    bits = tf[:rows].view(np.uint32)
    trace = [tuple(int(v) for v in ti[i]) + (int(bits[i, 0]), int(bits[i, 1])) for i in range(rows)]
    result = dict(layout=int(res[0]), rc=int(res[1]), multi_round=bool(res[2]), exhausted=bool(res[3]), final_variant=int(res[4]),
                  best=best.view(np.uint32).tolist(), samples=samples.tolist())
    return trace, result


def variant_allowed(v, multi_round, try_tail):
    return v < 2 or (v != 6 and multi_round and try_tail)  # (tail shadows: only when pinned, never in a tune)


def model(n_cands, multi, try_tail, shadows_on, layouts, variants, rcs, ms):
    """The same, restated from fnv_tune (tune.hip) as it stood when it held the tournament itself: float32 throughout, the
    constants as float32, the operands in its order."""
    ms, layouts, variants = np.asarray(ms, np.float32), np.asarray(layouts, np.int32), np.asarray(variants, np.int32)
    queues = {}
    trace, state = [], dict(layout=-1, exhausted=False)
    bits = lambda x: int(np.float32(x).view(np.uint32))

    def time(v, reps):
        pair = (state["layout"], v)
        if pair not in queues:  # the pair's answers, in the script's order
            queues[pair] = np.flatnonzero((layouts == pair[0]) & (variants == v)).tolist()
        q = queues[pair]
        if q:
            i = q.pop(0)
            rc, t = int(rcs[i]), ms[i]
        else:
            rc, t, state["exhausted"] = EXHAUSTED, F(0), True
        trace.append((TIME, state["layout"], v, reps, bits(t), bits(F(rc))))
        return rc, t

    def time_layout(li):
        state["layout"] = li
        trace.append((USE, li, 0, 0, 0, 0))
        t1 = t4 = F(-1)
        rc, t = time(1, 4)
        if rc:
            return rc, None
        t1 = t
        if multi[li] and try_tail:
            rc, t = time(3, 4)
            if rc:
                return rc, None
            t4 = t
        trace.append((LOG_LAYOUT, li, 0, 0, bits(t1), bits(t4)))
        return 0, (t4 if (t4 > F(0) and t4 < t1) else t1)

    best_layout, best_t, won_by_duel = 0, F(-1), False
    for li in range(n_cands):
        rc, t = time_layout(li)
        if rc:
            continue
        if best_t < F(0) or t < best_t * F(0.95):
            best_t, best_layout, won_by_duel = t, li, False
        elif t < best_t * F(0.985):
            sum_b = sum_c = F(0)
            wins, rounds = True, 0
            while rounds < 2 and wins:
                tb = tc = F(-1)
                rc_b, t = time_layout(best_layout)
                rc_c = None
                if rc_b == 0:
                    tb = t
                    rc_c, t = time_layout(li)
                    if rc_c == 0:
                        tc = t
                wins = bool(tc < tb * F(0.99)) if (rc_b == 0 and rc_c == 0) else False
                sum_b = F(sum_b + tb)
                sum_c = F(sum_c + tc)
                rounds += 1
            trace.append((LOG_DUEL, li, best_layout, rounds if wins else -rounds, bits(sum_c), bits(sum_b)))
            if wins:
                best_t, best_layout, won_by_duel = F(sum_c / F(rounds)), li, True
    if best_layout != 0 and not won_by_duel:
        rc, again = time_layout(0)
        if rc == 0 and not (best_t < again * F(0.95)):
            best_layout = 0
    state["layout"] = best_layout
    trace.append((USE, best_layout, 0, 0, 0, 0))
    multi_round = bool(multi[best_layout])
    best, samples, rc = [F(-1)] * NV, [0] * NV, 0
    for v in range(NV):
        if not variant_allowed(v, multi_round, try_tail):
            continue
        rc, t = time(v, 4)
        if rc:
            break
        best[v] = t
        trace.append((LOG_VARIANT, v, 0, 0, bits(t), 0))
        samples[v] = 4
    final = -1
    if rc == 0:  # owner_final_variant (launch_plan.hpp): the fastest, the merged-beam kernel winning a tie against the two-heap kernel
        final = 0
        for v in range(1, NV):
            if variant_allowed(v, multi_round, try_tail) and samples[v] > 0 and (best[v] < best[final] or (v == 1 and best[1] <= best[0])):
                final = v
    return trace, dict(layout=best_layout, rc=rc, multi_round=multi_round, exhausted=state["exhausted"], final_variant=final,
                       best=[bits(b) for b in best], samples=samples)


def run(n_cands, answers, multi=None, try_tail=True, shadows_on=True):
    """A named case: `answers` maps (layout, variant) to its queue of ms or (rc, ms).  Both implementations must agree; -> the
    time requests [(layout, variant, reps)], the result, the whole trace."""
    multi = [0] * n_cands if multi is None else multi
    layouts, variants, rcs, ms = [], [], [], []
    for (li, v), queue in answers.items():
        for a in queue:
            rc, t = a if isinstance(a, tuple) else (0, a)
            layouts.append(li), variants.append(v), rcs.append(rc), ms.append(t)
    args = (n_cands, multi, try_tail, shadows_on, layouts, variants, rcs, ms)
    trace, result = tournament(*args)
    assert (trace, result) == model(*args)
    assert not result["exhausted"], "the case's script covers every request"
    return [r[1:4] for r in trace if r[0] == TIME], result, trace


def f32(x):
    return float(F(x))


STEP2 = [0.5, 0.25]  # variants 0 and 1 of a single-round launch: the merged-beam kernel wins


def step2(layout, multi_round=False):
    """The answers step 2 asks for under `layout`, and its requests."""
    vs = [0, 1, 2, 3, 4, 5] if multi_round else [0, 1]
    return {(layout, v): [0.25 if v == 1 else 0.5] for v in vs}, [(layout, v, 4) for v in vs]


def merge(*dicts):
    out = {}
    for d in dicts:
        for k, q in d.items():
            out[k] = out.get(k, []) + list(q)  # (a pair's answers keep their order: step 1's first)
    return out


def test_one_candidate_only():
    a2, r2 = step2(0)
    req, res, _ = run(1, merge({(0, 1): [1.0]}, a2))
    assert req == [(0, 1, 4)] + r2 and res["layout"] == 0 and res["rc"] == 0 and res["samples"] == [4, 4, 0, 0, 0, 0, 0]
    assert res["final_variant"] == 1


def test_a_neighbour_wins_by_more_than_the_margin_and_the_second_look_confirms_it():
    a2, r2 = step2(1)
    req, res, _ = run(2, merge({(0, 1): [1.0, 1.0], (1, 1): [0.90]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4)] + r2 and res["layout"] == 1


def test_a_neighbour_wins_by_more_than_the_margin_and_the_second_look_reverses_it():
    a2, r2 = step2(0)
    req, res, _ = run(2, merge({(0, 1): [1.0, 0.92], (1, 1): [0.90]}, a2))  # 0.90 is not below 0.95 x 0.92
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4)] + r2 and res["layout"] == 0


def test_a_neighbour_at_exactly_the_margin_does_not_win_outright():
    edge = f32(F(1.0) * F(0.95))  # t < best * 0.95f is strict: this one goes to the duel, and loses its first round
    a2, r2 = step2(0)
    req, res, trace = run(2, merge({(0, 1): [1.0, 1.0], (1, 1): [edge, 1.0]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4), (1, 1, 4)] + r2 and res["layout"] == 0
    assert [r[1:4] for r in trace if r[0] == LOG_DUEL] == [(1, 0, -1)]
    below = f32(np.nextafter(F(edge), F(0)))  # one ulp less wins outright: no duel, the second look at the rules' layout
    a2, r2 = step2(1)
    req, res, trace = run(2, merge({(0, 1): [1.0, 1.0], (1, 1): [below]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4)] + r2 and res["layout"] == 1 and not [r for r in trace if r[0] == LOG_DUEL]


def test_a_neighbour_inside_the_margin_wins_both_rounds_of_the_duel():
    a2, r2 = step2(1)
    req, res, trace = run(2, merge({(0, 1): [1.0, 1.0, 1.0], (1, 1): [0.97, 0.98, 0.96]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4), (1, 1, 4), (0, 1, 4), (1, 1, 4)] + r2  # holder, challenger, twice; no second look
    assert res["layout"] == 1
    duel = [r for r in trace if r[0] == LOG_DUEL]
    assert [r[1:4] for r in duel] == [(1, 0, 2)]
    assert duel[0][4] == int((F(0.98) + F(0.96)).view(np.uint32)) and duel[0][5] == int(F(2.0).view(np.uint32))


def test_a_neighbour_inside_the_margin_loses_the_first_round():
    a2, r2 = step2(0)
    req, res, trace = run(2, merge({(0, 1): [1.0, 1.0], (1, 1): [0.97, f32(F(1.0) * F(0.99))]}, a2))  # exactly 1 %: not a win
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4), (1, 1, 4)] + r2 and res["layout"] == 0  # round 2 is not run
    assert [r[1:4] for r in trace if r[0] == LOG_DUEL] == [(1, 0, -1)]


def test_a_neighbour_inside_the_margin_wins_the_first_round_and_loses_the_second():
    a2, r2 = step2(0)
    req, res, trace = run(2, merge({(0, 1): [1.0, 1.0, 1.0], (1, 1): [0.97, 0.98, 0.995]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4)] + [(0, 1, 4), (1, 1, 4)] * 2 + r2 and res["layout"] == 0
    assert [r[1:4] for r in trace if r[0] == LOG_DUEL] == [(1, 0, -2)]


def test_a_neighbour_that_is_not_1_5_percent_faster_is_ignored():
    a2, r2 = step2(0)
    for t in (f32(F(1.0) * F(0.985)), 0.99, 1.0, 1.02):
        req, res, trace = run(2, merge({(0, 1): [1.0], (1, 1): [t]}, a2))
        assert req == [(0, 1, 4), (1, 1, 4)] + r2 and res["layout"] == 0 and not [r for r in trace if r[0] == LOG_DUEL]


def test_an_outright_winner_after_a_duel_winner_gets_the_second_look_again():
    a2, r2 = step2(2)
    req, res, _ = run(3, merge({(0, 1): [1.0, 1.0, 1.0, 1.0], (1, 1): [0.97, 0.98, 0.96], (2, 1): [0.80]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4)] + [(0, 1, 4), (1, 1, 4)] * 2 + [(2, 1, 4), (0, 1, 4)] + r2
    assert res["layout"] == 2
    # (without the later winner the duel's winner stands and the rules' layout is not timed again)
    a2, r2 = step2(1)
    req, res, _ = run(3, merge({(0, 1): [1.0, 1.0, 1.0], (1, 1): [0.97, 0.98, 0.96], (2, 1): [0.96]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4)] + [(0, 1, 4), (1, 1, 4)] * 2 + [(2, 1, 4)] + r2 and res["layout"] == 1


def test_a_layout_whose_first_measurement_fails_is_skipped():
    a2, r2 = step2(0)
    req, res, trace = run(3, merge({(0, 1): [1.0], (1, 1): [(2, 0.5)], (2, 1): [1.0]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (2, 1, 4)] + r2 and res["layout"] == 0
    assert [r[1] for r in trace if r[0] == LOG_LAYOUT] == [0, 2]
    # ... and so is one whose tail measurement fails
    a2, r2 = step2(0, True)
    req, res, _ = run(2, merge({(0, 1): [1.0], (0, 3): [0.9], (1, 1): [0.5], (1, 3): [(2, 0.4)]}, a2), multi=[1, 1])
    assert req == [(0, 1, 4), (0, 3, 4), (1, 1, 4), (1, 3, 4)] + r2 and res["layout"] == 0


def test_when_the_rules_layout_fails_the_next_success_holds_with_no_margin():
    # layout 1 holds although there was nothing to beat, layout 2 is no faster; the holder is a neighbour that won on one
    # measurement, so the rules' layout is timed again, now last -- and loses to it by more than the margin
    a2, r2 = step2(1)
    req, res, _ = run(3, merge({(0, 1): [(2, 0.0), 5.0], (1, 1): [3.0], (2, 1): [3.0]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (2, 1, 4), (0, 1, 4)] + r2 and res["layout"] == 1
    # ... or does not (3.0 is not 5 % below 2.0): the rules' layout it is
    a2, r2 = step2(0)
    req, res, _ = run(2, merge({(0, 1): [(2, 0.0), 2.0], (1, 1): [3.0]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4)] + r2 and res["layout"] == 0
    a2, r2 = step2(1)
    req, res, _ = run(2, merge({(0, 1): [(2, 0.0), (2, 0.0)], (1, 1): [3.0]}, a2))  # the second look fails too: the neighbour stays
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4)] + r2 and res["layout"] == 1


def test_a_failure_inside_a_duel_is_a_lost_round():
    a2, r2 = step2(0)
    # the holder fails in round 1: the challenger is not even timed
    req, res, trace = run(2, merge({(0, 1): [1.0, (2, 0.0)], (1, 1): [0.97]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4), (0, 1, 4)] + r2 and res["layout"] == 0
    assert [r[1:4] for r in trace if r[0] == LOG_DUEL] == [(1, 0, -1)]
    # the challenger fails in round 2
    req, res, trace = run(2, merge({(0, 1): [1.0, 1.0, 1.0], (1, 1): [0.97, 0.97, (2, 0.0)]}, a2))
    assert req == [(0, 1, 4), (1, 1, 4)] + [(0, 1, 4), (1, 1, 4)] * 2 + r2 and res["layout"] == 0
    assert [r[1:4] for r in trace if r[0] == LOG_DUEL] == [(1, 0, -2)]


def test_a_single_round_launch_never_times_a_tail():
    a2, r2 = step2(0)
    req, res, _ = run(2, merge({(0, 1): [1.0], (1, 1): [1.0]}, a2), multi=[0, 0])
    assert req == [(0, 1, 4), (1, 1, 4), (0, 0, 4), (0, 1, 4)] and res["samples"] == [4, 4, 0, 0, 0, 0, 0] and not res["multi_round"]
    # more than one round: the 75 % tail next to the merged-beam kernel alone, the better of the two counting; all six variants
    a2, r2 = step2(1, True)
    req, res, _ = run(2, merge({(0, 1): [1.0, 1.0], (0, 3): [1.1, 1.1], (1, 1): [1.0], (1, 3): [0.9]}, a2), multi=[1, 1])
    assert req == [(0, 1, 4), (0, 3, 4), (1, 1, 4), (1, 3, 4), (0, 1, 4), (0, 3, 4)] + r2
    assert res["layout"] == 1 and res["samples"] == [4, 4, 4, 4, 4, 4, 0] and res["multi_round"]


def test_a_pinned_tail_percentage_leaves_no_tail_variants():
    a2, r2 = step2(0)
    req, res, _ = run(2, merge({(0, 1): [1.0], (1, 1): [1.0]}, a2), multi=[1, 1], try_tail=False)  # sorted_tail_exact_pct >= 0
    assert req == [(0, 1, 4), (1, 1, 4), (0, 0, 4), (0, 1, 4)] and res["samples"] == [4, 4, 0, 0, 0, 0, 0] and res["multi_round"]


def test_a_failure_in_the_variant_pass_returns_its_code():
    req, res, _ = run(1, {(0, 1): [1.0, 0.25], (0, 3): [1.1], (0, 0): [0.5], (0, 2): [(5, 0.0)]}, multi=[1])
    assert req == [(0, 1, 4), (0, 3, 4), (0, 0, 4), (0, 1, 4), (0, 2, 4)] and res["rc"] == 5 and res["final_variant"] == -1
    assert res["samples"] == [4, 4, 0, 0, 0, 0, 0]
    req, res, _ = run(1, {(0, 1): [1.0], (0, 0): [(7, 0.0)]})
    assert req == [(0, 1, 4), (0, 0, 4)] and res["rc"] == 7 and res["samples"] == [0] * NV


RATIOS = [0.90, 0.94, 0.95, 0.96, 0.984, 0.985, 0.99, 1.0, 1.02]


def test_the_tournament_equals_its_restatement_on_random_scripts():
    """12 000 scripts: up to eight layouts whose times are the rules' times a ratio from around every threshold (as float32
    products, so that t == best * 0.95f and the like really occur), repeated measurements drifting by the same ratios or a few
    tenths of a per cent or not at all, tails better and worse and not positive, failures anywhere.  The whole trace -- every
    request with its answer, every logged value, bit for bit -- and the whole result must be equal."""
    rng = np.random.default_rng(20260117)
    depth, seen = 20, dict(duel=0, duel_won=0, failed=0, layouts=set())
    ratios = np.asarray(RATIOS, np.float32)
    li_of, v_of = (a.reshape(-1) for a in np.meshgrid(np.arange(8), np.arange(NV), np.arange(depth), indexing="ij")[:2])
    for case in range(12000):
        n = int(rng.integers(1, 9))
        base = F(rng.choice([1.0, 0.37, 3.0e-4]))
        first = base * ratios[rng.integers(0, len(ratios), (8, NV, 1))]  # float32 products of the rules' first time
        first[0, 1, 0] = base
        drift = np.where(rng.random((8, NV, depth)) < 0.5, F(1), ratios[rng.integers(0, len(ratios), (8, NV, depth))])
        jitter = (1 + (rng.random((8, NV, depth)) - 0.5) * 0.01).astype(np.float32)
        drift = np.where(rng.random((8, NV, depth)) < 0.3, jitter, drift).astype(np.float32)
        drift[:, :, 0] = 1
        ms = (first * np.cumprod(drift, axis=2, dtype=np.float32)).astype(np.float32)
        ms[:, 3, :] *= F(rng.choice([0.9, 0.97, 1.0, 1.05]))
        ms[:, 3, :][rng.random((8, depth)) < 0.02] = rng.choice([0.0, -1.0])
        rcs = np.where(rng.random((8, NV, depth)) < rng.choice([0.0, 0.02, 0.15]), 3, 0)
        multi = (rng.random(8) < rng.choice([0.0, 0.5, 1.0])).astype(np.int32)
        args = (n, multi, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), li_of, v_of, rcs.reshape(-1), ms.reshape(-1))
        got, want = tournament(*args), model(*args)
        assert got == want, case
        trace, res = got
        assert not res["exhausted"], case
        duels = [r for r in trace if r[0] == LOG_DUEL]
        seen["duel"] += len(duels)
        seen["duel_won"] += sum(r[3] > 0 for r in duels)
        seen["failed"] += any(r[0] == TIME and r[5] != 0 for r in trace)
        seen["layouts"].add(res["layout"])
    assert seen["duel"] > 2000 and seen["duel_won"] > 200 and seen["failed"] > 1000 and seen["layouts"] == set(range(8)), seen
