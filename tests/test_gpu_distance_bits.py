"""Every reported float distance against the lane-by-lane CPU model, bit for bit, on the GPU.

tests/distance_model.py restates batch_dists (csrc/distance.hpp) for one (query, row) pair -- each lane's chunks in its order, fused
multiply-adds where the kernels fuse, a.x + a.y, group_sum's butterfly, finish -- and tests/test_distance_model.py has checked
that model on the CPU.  Here every (element type, metric, row geometry class of tests/row_classes.py) gets one 600-row index
per data set: `real` (the float data of tests/test_gpu_row_classes.py, where order, fusing and widening all show in the last
bits), `edges` (distance_model.edge_case: random full-width mantissas over the finite exponent range, copies and negations of
queries, cancelling products, float32 and binary16 subnormals, -0), and for float32 L2 `overflow` (four rows at +inf).

1. the exhaustive scan: all 40 x 600 distances have the model's bits, the list is in (distance, node id) order;
2. the graph searches (default, K1, K0, K1f with everything allowed, mirror rows on and off): every reported (label, distance)
   has the model's bits for that (query, node) -- nothing about WHICH nodes are reported: on real-valued data the oracle may
   walk another path;
3. the grouped scan under two filters: the plain scan's bits.
No tolerance anywhere.  float16 IP is included since its chunk is eight v_fma_mix_f32: the v_dot2_f32_f16 it used before matched
none of the model's candidate semantics when it was read off the hardware through these very calls (profiles/distance_bits.md;
the recorded probe is tests/golden/probes/dot2_probe.npz, checked on the CPU by tests/test_distance_model.py), and missed the forward
error bound of f32 arithmetic on rows with binary16 subnormals."""
import numpy as np
import pytest

import distance_model as dm
import row_classes as rc
from test_gpu_exhaustive import _build
from test_gpu_row_classes import _is_the_class

pytestmark = pytest.mark.gpu
N, NQ, K, EF = rc.N_ROWS, dm.NQ, 10, 64
TYPES, METRICS = ("float32", "float16"), ("l2", "ip")
CASES = [(dtype, metric, name) for dtype in TYPES for metric in METRICS for name in rc.CASES]
MIRROR_CASES = ("8x2-full", "8x4-full", "16x4-full", "32x4-full", "64x4-full", "64x4-full-spans")  # five configurations
INF_BITS = 0x7F800000


class DataSet:
    """One index and what its (query, node) distances must be."""

    def __init__(self, oracle_mod, what, name, dtype, metric, X, Q):
        self.what, self.dtype, self.metric, self.Q = what + (name,), dtype, metric, Q
        self.X, self.labels, self.dev = _build(oracle_mod, metric, dtype, X, M=32)  # rows in node order; labels = row numbers
        self.node_of = np.empty(N, np.int64)
        self.node_of[self.labels] = np.arange(N)
        self.D = dm.dist64(self.X, Q, metric)
        self.model = dm.distances(dtype, metric, self.X, Q)
        self._scan = None

    def scan(self):
        """(distance bits by (query, node), distances, labels, stats) of the plain exhaustive scan, run once."""
        if self._scan is None:
            d, l, st = self.dev.search_exhaustive(self.Q, N, stats=True)
            assert (st["count"] == N).all() and (st["n_dist"] == N).all() and (np.sort(l, axis=1) == np.arange(N)).all(), self.what
            by_node = np.empty((NQ, N), np.uint32)
            np.put_along_axis(by_node, self.node_of[l.astype(np.int64)], d.view(np.uint32), 1)
            self._scan = (by_node, d, l, st)
        return self._scan

    def close(self):
        self.dev.close()


@pytest.fixture(scope="module", params=CASES, ids=lambda p: "-".join(p))
def sets(request, oracle_mod):
    dtype, metric, name = request.param
    klass, dim = _is_the_class(dtype, name)
    lossless = dtype == "float32" and name in MIRROR_CASES
    what = request.param + (dim,)
    real = DataSet(oracle_mod, what, "real", dtype, metric, *rc.float_case(dtype, metric, dim))
    edges = DataSet(oracle_mod, what, "edges", dtype, metric, *dm.edge_case(dtype, metric, dim, lossless))
    edges.lossless, edges.klass = lossless, klass
    for s in (real, edges):
        dm.assert_finite(s.D, s.what)  # before anything runs
    yield real, edges
    real.close()
    edges.close()


def _in_contract_order(d, l, node_of, what):
    """Ascending by (distance, node id)."""
    nodes = node_of[l.astype(np.int64)]
    assert (d[:, 1:] >= d[:, :-1]).all(), what
    assert (np.diff(nodes, axis=1)[d[:, 1:] == d[:, :-1]] > 0).all(), what


# ---- 1. the exhaustive scan -----------------------------------------------------------------------------------------------------------
def test_scan_reports_the_models_bits(sets):
    for s in sets:
        by_node, d, l, _ = s.scan()
        _in_contract_order(d, l, s.node_of, s.what)
        bad = np.argwhere(by_node != s.model)
        print("distance bits, scan: %s: %d of %d distances differ from the model" % (s.what, len(bad), by_node.size))
        assert not len(bad), s.what + ("first (query, node) %r: got %08x, model %08x" % (tuple(bad[0]), by_node[tuple(bad[0])], s.model[tuple(bad[0])]),)
        order = np.lexsort((np.broadcast_to(np.arange(N), (NQ, N)), s.model.view(np.float32)), axis=1)
        assert np.array_equal(l, s.labels[order]), s.what


# ---- 2. the graph searches -------------------------------------------------------------------------------------------------------------
def _pairs_carry(s, got, how):
    d, l, st = got
    real = np.arange(d.shape[1])[None, :] < np.asarray(st["count"]).astype(np.int64)[:, None]
    assert real.any() and (l[real] >= 0).all(), s.what + (how,)
    q = np.broadcast_to(np.arange(len(d))[:, None], d.shape)[real]
    want = s.model[q, s.node_of[l[real].astype(np.int64)]]
    bad = np.flatnonzero(d.view(np.uint32)[real] != want)
    assert not len(bad), s.what + (how, "%d of %d reported pairs; first: query %d label %d got %08x want %08x" % (
        len(bad), int(real.sum()), q[bad[0]], l[real][bad[0]], d.view(np.uint32)[real][bad[0]], want[bad[0]]))


def _graph_forms(s, tail, mirror):
    dev = s.dev

    def search(*a, **kw):
        got = dev.search(s.Q, K, EF, *a, stats=True, **kw)
        assert bool(dev.half_rows()["used_by_last_launch"]) == mirror, s.what + (mirror, dev.half_rows())
        return got

    _pairs_carry(s, search(), ("default", mirror))
    dev.set_option("sorted_beam", 0)
    _pairs_carry(s, search(), ("two heaps", mirror))
    assert dev.launch_geometry()["kernel"] == "two_heaps"
    dev.set_option("sorted_beam", 2)
    if not tail:  # K0: the host never runs it on split rows
        dev.set_option("entry_kernel", 1)
        _pairs_carry(s, search(), ("entry kernel", mirror))
        dev.set_option("entry_kernel", 0)
    _pairs_carry(s, dev.search_filtered(s.Q, K, EF, np.arange(N), stats=True), ("filtered, all allowed", mirror))


def test_graph_searches_report_the_models_bits(sets):
    real, edges = sets
    k = edges.klass
    eligible = edges.dtype == "float32" and k.full and not k.tail_chunks and k.CU % 2 == 0  # half_rows_eligible, csrc/half_rows.hpp
    assert eligible == edges.lossless and (edges.dev.half_rows()["state"] == "live") == eligible, edges.what + (edges.dev.half_rows(),)
    assert real.dev.half_rows()["state"] != "live", real.what  # random float32 rows are not binary16 values
    try:
        _graph_forms(real, k.tail_chunks, False)
        for half_rows in ((0, 1) if eligible else (1,)):
            edges.dev.set_option("half_rows", half_rows)
            _graph_forms(edges, k.tail_chunks, bool(eligible and half_rows))
    finally:
        for s in sets:
            for name, v in (("half_rows", 1), ("entry_kernel", 0), ("sorted_beam", 2)):
                s.dev.set_option(name, v)


# ---- 3. the grouped scan ---------------------------------------------------------------------------------------------------------------
def test_grouped_scan_has_the_plain_scans_bits(sets):
    _, s = sets
    rng = np.random.default_rng(N + s.X.shape[1])
    filters = [rng.choice(N, N // 2, replace=False), np.arange(N)]
    qf = (np.arange(NQ) % 2).astype(np.int32)
    d, l, st = s.dev.search_exhaustive_grouped(s.Q, N, filters, qf, stats=True)
    plain = s.scan()[0]
    for f, allowed in enumerate(filters):
        rows = np.flatnonzero(qf == f)
        m = len(allowed)
        assert (st["count"][rows] == m).all() and (st["n_dist"][rows] == m).all(), s.what + (f,)
        assert (np.sort(l[rows, :m], axis=1) == np.sort(allowed)).all() and (l[rows, m:] == -1).all(), s.what + (f,)
        nodes = s.node_of[l[rows, :m].astype(np.int64)]
        assert np.array_equal(d.view(np.uint32)[rows, :m], plain[rows[:, None], nodes]), s.what + (f,)
        _in_contract_order(d[rows, :m], l[rows, :m], s.node_of, s.what + (f,))
        assert np.array_equal(d.view(np.uint32)[rows, :m], s.model[rows[:, None], nodes]), s.what + (f,)


# ---- overflow: float32 L2, the scan only -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.CASES)
def test_scan_of_rows_that_overflow(oracle_mod, name):
    _, dim = _is_the_class("float32", name)
    X, Q = dm.edge_case("float32", "l2", dim, name in MIRROR_CASES)
    s = DataSet(oracle_mod, ("float32", "l2", name, dim), "overflow", "float32", "l2", dm.overflow_case(X), Q)
    try:
        over = s.node_of[list(dm.OVERFLOW_ROWS)]
        finite = np.setdiff1d(np.arange(N), over)
        dm.assert_finite(s.D[:, finite], s.what)
        assert (s.D[:, over] > 3e38).all() and (s.model[:, over] == INF_BITS).all(), s.what
        by_node, d, l, _ = s.scan()
        assert np.array_equal(by_node, s.model), s.what
        assert (by_node[:, over] == INF_BITS).all(), s.what
        assert np.array_equal(l[:, N - 4:], np.broadcast_to(s.labels[np.sort(over)], (NQ, 4))), s.what  # last, by node id
        _in_contract_order(d, l, s.node_of, s.what)
    finally:
        s.close()


# ---- the rows that read the two-element dot off the hardware ----------------------------------------------------------------------------
def test_float16_ip_on_the_rows_of_the_dot_probe(oracle_mod):
    """distance_model.dot2_case: a float16 IP index of dim 8 with products in elements 0, 1, 4 and 5 only -- sums that need more
    than 24 bits, binary16 subnormals times 2^13 .. 2^15 as the deciding (or only) product, integer operands up to 2048 with
    sums just below 2^24.  These calls showed what v_dot2_f32_f16 computes; the per-element kernel has the model's bits on them,
    the subnormal products arrive exactly, and the integers are exact."""
    X, Q = dm.dot2_case()
    s = DataSet(oracle_mod, ("float16", "ip", "dot2", 8), "dot2", "float16", "ip", X, Q)
    try:
        got = s.scan()[0]
        assert np.array_equal(got, s.model)
        X64, Q64 = s.X.astype(np.float64), Q.astype(np.float64)
        single = ((X64[None, :, :] * Q64[:, None, :]) != 0).sum(2) == 1
        sub_rows = s.node_of[np.arange(6, N - 10, 10)]
        assert single[30:, sub_rows].all()  # one product: a binary16 subnormal times 2^13 .. 2^15
        assert np.array_equal(got[30:, sub_rows], (1.0 - Q64[30:] @ X64[sub_rows].T).astype(np.float32).view(np.uint32))
        assert (got[30:, sub_rows] != np.float32(1.0).view(np.uint32)).all()
        ints = s.node_of[np.arange(N - 10, N)]
        want = (1.0 - Q64[28:30] @ X64[ints].T).astype(np.float32).view(np.uint32)
        assert np.array_equal(got[28:30][:, ints], want)
    finally:
        s.close()
