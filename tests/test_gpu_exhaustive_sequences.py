"""Random call sequences of the exhaustive search on ONE handle per index, held to numpy exactly (tests/exhaustive_sequences.py
draws them, tests/test_exhaustive_sequences_plan.py holds the draws to the kernels they must reach).  Nothing is reset between
steps: the workspaces grow and are reused at other sizes, the in-range count words move behind partial lists of another
size, the float engines' counters share the status block with the graph search.  After every step: labels, distance bits,
padding, count and n_dist equal the contract; the launch ran the kernel the planner names, as a range search or not; the
rescoring counters are the engine's.  Every tenth step a graph search and (float32) a filtered one return their first bytes."""
import numpy as np
import pytest

import exhaustive_sequences as seq
from test_gpu_exhaustive import _build, _dist64, _equal, _same_results
from test_gpu_filtered import _same

pytestmark = pytest.mark.gpu


def _call(dev, step, Q):
    if step.kind == "grouped":
        return dev.search_exhaustive_grouped(Q[:step.nq], step.K, step.filters, step.qf, stats=True)
    return dev.search_exhaustive(Q[:step.nq], step.K, allowed=step.filters[0] if step.kind == "one" else None, stats=True)


@pytest.mark.parametrize("ix", seq.indexes(), ids=seq.name_of)
def test_a_sequence_on_one_handle(oracle_mod, ix):
    X, Q, labels = seq.data(ix)
    steps = seq.sequence(ix)
    X, labels, dev = _build(oracle_mod, ix.metric, ix.dtype, X, labels, M=8, efc=16)  # (rows and labels in NODE order from here on)
    D = _dist64(X, Q, ix.metric)
    half = np.sort(labels)[::2]
    graph = lambda: dev.search(Q[:33], 10, 64, stats=True)  # noqa: E731
    graph_filtered = lambda: dev.search_filtered(Q[:33], 10, 64, half, stats=True)  # noqa: E731
    graph_first, filtered_first = graph(), graph_filtered() if ix.dtype == "float32" else None
    first = None
    for i, step in enumerate(steps):
        what, plan = (seq.name_of(ix), i, step.kind, step.nq, step.K, step.seg, step.radius_kind, step.own, step.grouped, step.block), seq.plan(ix, step)
        for name, value in seq.option_values(ix, step).items():
            dev.set_option(name, value)
        if plan.refused:  # (the planner refuses none at these row lengths; a sequence that holds one must see the call raise)
            with pytest.raises(ValueError):
                _call(dev, step, Q)
            continue
        got, geom, rescored = _call(dev, step, Q), dev.launch_geometry(), dev.scan_rescored()
        first = got if i == 0 else first
        cands = seq.row_candidates(step, labels)
        _equal(got, seq.expected(step, D, labels, cands), what)
        assert (geom["kernel_mode"], geom["range"]) == (plan.kernel_mode, int(step.radius is not None)), (what, geom, plan)
        assert geom["block_threads"] == 64 * max(1, plan.waves), (what, geom, plan)
        if plan.kernel_mode >= 5:  # a float engine: every (query, candidate) pair scored on the matrix cores, once
            assert rescored["scored"] == sum(len(c) for c in cands) and 0 <= rescored["rescored"] <= rescored["scored"], (what, rescored)
        else:
            assert rescored == {"scored": 0, "rescored": 0} and dev.replayed_queries()["total"] == 0, (what, rescored)
        if i % 10 == 9:  # the scan has left the graph search's status block and workspaces alone, and the reverse
            _same(graph(), graph_first, (what, "graph search"))
            if filtered_first is not None:
                _same(graph_filtered(), filtered_first, (what, "filtered graph search"))
    for name in ("scan_matrix", "scan_matrix_float", "scan_matrix_float32", "scan_matrix_grouped", "scan_matrix_block"):
        dev.set_option(name, 0)
    dev.set_option("scan_radius", -1)
    dev.set_option("scan_segment_rows", steps[0].seg)
    _same_results(_call(dev, steps[0], Q), first, (seq.name_of(ix), "the first step again, every option set back"))
    assert (dev.launch_geometry()["kernel_mode"], dev.launch_geometry()["range"]) == (3, 0)
