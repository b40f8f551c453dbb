"""The inputs of tests/test_gpu_batched_wiring.py, and what each must reach inside the wiring code (test infrastructure).

A case = one table of integer-valued rows, a seed graph of `first` nodes built by the oracle, and one or more insertion
batches.  `model(case, oracle_mod)` runs the CPU model over it once per process and keeps the result; `expect` names the
path counters of the model (tests/batched_wiring_ref.cpp) that the case exists for.  tests/test_batched_wiring_model.py
asserts them on the CPU, so that the inputs are known to reach each path before a GPU sees them."""
from __future__ import annotations

import zlib

import numpy as np

import batched_wiring_ref as bwr


class Case:
    def __init__(self, name, dtype="float32", metric="l2", dim=16, M=8, efc=16, first=40, counts=(700,), hi=4, expect=()):
        self.name, self.dtype, self.metric, self.dim, self.M, self.efc = name, dtype, metric, dim, M, efc
        self.first, self.counts, self.hi, self.expect = first, tuple(counts), hi, tuple(expect)

    def __repr__(self):
        return "%s: %s %s d=%d M=%d efc=%d first=%d counts=%s values 0..%d" % (
            self.name, self.dtype, self.metric, self.dim, self.M, self.efc, self.first, list(self.counts), self.hi - 1)


def _more(name, than=0):
    return (name, lambda c, case: c[name] > than, "%s > %d" % (name, than))


HUB = [_more("max_requesters", 64), _more("chunked_targets"), _more("block_crossing_runs"), _more("pruned_then_extended")]
ALL_SHORT = ("short_beam_nodes", lambda c, case: c["short_beam_nodes"] == sum(case.counts), "short_beam_nodes == count")
UNPRUNED = ("targets", lambda c, case: c["targets"] > c["pruned_targets"], "targets > pruned_targets")

CASES = []
# hub targets: 40 live nodes take the back-links of 700 new ones (values 0..3: ties everywhere)
for dt, metric in (("float32", "l2"), ("float32", "angular"), ("uint8", "l2"), ("int8", "l2")):
    CASES.append(Case("hub-%s-%s" % (dt, metric), dtype=dt, metric=metric, expect=HUB))
# pruned, then extended without a second prune: after a prune to k kept, the last round must bring at most M - k requesters.
# In 4 dimensions a prune keeps few, so about one chunked target in four ends that way (the hub cases above: one or two).
CASES.append(Case("pruned-then-extended", dtype="uint8", dim=4, first=100, hi=60,
                  expect=[_more("pruned_then_extended", 4), _more("chunked_targets", 9)]))
# block boundaries of the sorted request list.  M = 2 -> keep = 1, one request per new node, so the list's length is the
# batch's: 63 requests end one short of the first block's end, 64 fill it exactly, 65 put one request into a second block
# (these three pin the list's lengths around the boundary; with this data none of their runs crosses it); with 67 and 129 a
# target's run starts in one block and ends in the next.  M = 8: four requests per node, runs cross at every count.
ONE_EACH = ("requests", lambda c, case: c["requests"] == sum(case.counts), "requests == count")
for count in (63, 64, 65):
    CASES.append(Case("block-M2-count%d" % count, M=2, counts=(count,), expect=[ONE_EACH]))
for count in (67, 129):
    CASES.append(Case("block-M2-count%d" % count, M=2, counts=(count,), expect=[ONE_EACH, _more("block_crossing_runs")]))
for count in (63, 64, 65, 129):
    CASES.append(Case("block-M8-count%d" % count, M=8, counts=(count,), expect=[_more("block_crossing_runs")]))
CASES.append(Case("free-slots", M=32, efc=40, first=600, counts=(256,), hi=60, expect=[_more("shared_free_slots"), UNPRUNED]))
for efc in (100, 200):
    CASES.append(Case("wide-prunes-efc%d" % efc, M=16, efc=efc, first=800, counts=(128,), expect=[_more("wide_prunes")]))
# (those are the select step's; a hub whose row and requesters make a union of more than 64 reaches the connect step's)
CASES.append(Case("wide-prunes-connect", M=16, efc=100, first=40, counts=(300,), expect=[_more("wide_prunes_connect")]))
for first in (1, 2, 3):
    for M in (8, 16):
        CASES.append(Case("tiny-first%d-M%d" % (first, M), M=M, first=first, counts=(50,), expect=[ALL_SHORT]))
CASES.append(Case("short-beam-efc5-M16", M=16, efc=5, first=300, counts=(100,), hi=60, expect=[ALL_SHORT]))
for M in (1, 3, 48, 64):
    CASES.append(Case("row-width-M%d" % M, M=M, efc=40, first=300, counts=(300,), hi=60))
# row configurations of the distance code (100-d float32 / 200-d float16 / 410-d uint8: split rows; 768-d: query in registers)
for dt, dim, metric in (("float32", 7, "l2"), ("float32", 100, "angular"), ("float32", 768, "l2"), ("float16", 128, "angular"),
                        ("float16", 200, "l2"), ("uint8", 400, "l2"), ("uint8", 410, "angular")):
    CASES.append(Case("row-config-%s-d%d" % (dt, dim), dtype=dt, metric=metric, dim=dim, M=16, efc=40, first=300, counts=(200,),
                      hi=40))  # sums <= 768 * 39^2 < 2^24
CASES.append(Case("chained", dtype="uint8", metric="angular", first=60, counts=(1, 7, 64, 500, 3),
                  expect=[_more("equal_key_pops"), _more("chunked_targets")]))
BY_NAME = {c.name: c for c in CASES}

_done = {}


def data(case):
    rng = np.random.default_rng(zlib.crc32(("%s %d %d" % (case.dtype, case.dim, case.hi)).encode()))
    return bwr.integer_data(rng, case.first + sum(case.counts), case.dim, case.dtype, case.hi)


def model(case, oracle_mod):
    """-> (Batch after the last step, [(links, counters, evals)] per step, counters summed over the steps, max_requesters =
    the largest of them).  Computed once; nobody changes what it returns."""
    if case.name not in _done:
        b = bwr.Batch(oracle_mod, case.metric, case.dtype, case.dim, case.M, data(case), case.first, case.efc)
        steps = [b.insert(count) for count in case.counts]
        total = {k: (max if k == "max_requesters" else sum)(s[1][k] for s in steps) for k in bwr.COUNTERS}
        _done[case.name] = (b, steps, total)
    return _done[case.name]


def check_expectations(case, total):
    for name, ok, what in case.expect:
        assert ok(total, case), "%r does not reach its path: want %s, model counted %s" % (case, what, total)
