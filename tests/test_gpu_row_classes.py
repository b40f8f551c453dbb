"""Every reachable row geometry class through every search kernel family, on the GPU.

tests/row_classes.py derives the classes from the launch planner -- (row configuration, FULL or not, side-table chunks, one
span or several), 18 per element type over dims 1 .. 9000 -- and names each class's smallest dim, where the last chunk and the
row hold the most zero padding, and for the seven clamped classes the dense dim too, where the chunk that a clamped lane re-reads
is data instead of padding.  Here every (element type, metric, class) gets one small index of its own and runs the
exhaustive scan (KS), the grouped scan (KSg), the graph search's kernels (K1 / K2 in every beam form, K0), the filtered search
(K1f), its grouped form and the device builder's wiring.  The point is the geometry, not the workload: 600 rows, 40 queries.

On the integer-valued data every distance is an exact integer, so everything is compared exactly: distance bits, labels,
count, n_dist and n_hops -- against the plain numpy reference of tests/test_gpu_exhaustive.py, the CPU oracle, and the CPU
restatement of the filtered search.  float32 / float16 values are kept so small that every distance stays below 2^24 (asserted
on the float64 matrix); the exact integer distances of one-byte rows may exceed that: the contract there is the exact integer
correctly rounded, which is what float64 -> float32 gives.  Float data is held to DESIGN section 8's float bar against float64
with nothing left out, and to the graph search's own distance bits (tests/test_row_classes.py shows on the CPU that a float32
sum in any order stays inside that bar on these very inputs)."""
import numpy as np
import pytest

import filtered_ref
import row_classes as rc
from flatnav_amd import hip
from test_gpu_exhaustive import ATOL, RTOL, _build, _dist64, _equal, _topk
from test_gpu_filtered import _int_data, _pair, _same
from test_gpu_grouped_filters import GRAPH_KEYS, SCAN_KEYS, _rows_equal

pytestmark = pytest.mark.gpu
N, NQ, M, EFC = rc.N_ROWS, 40, 8, 24
SHIFT = 3  # labels are a permutation of SHIFT .. SHIFT + N - 1: never node ids
LONG_DIM = 5200  # float32: one query with its list exceeds the scan's 20 KB block budget
METRICS = ("l2", "ip")
# rc.CASES: each class at its smallest dim, the clamped classes at their dense dim as well
INT_CASES = [(dtype, metric, name) for dtype in rc.TYPES for metric in METRICS for name in rc.CASES]
FLOAT_CASES = [(dtype, metric, name) for dtype in ("float32", "float16") for metric in METRICS for name in rc.CASES]


@pytest.fixture(scope="module")
def flatnav():
    import flatnav_amd

    return flatnav_amd


class Case:
    """One index on integer-valued data and what every family's check needs of it."""

    def __init__(self, oracle_mod, dtype, metric, dim, klass=None):
        self.dtype, self.metric, self.dim = dtype, metric, dim
        self.what = (dtype, metric, klass, dim)
        seed = dim * 8 + list(rc.TYPES).index(dtype) * 2 + METRICS.index(metric)
        self.rng = rng = np.random.default_rng(seed)
        X, Q = _int_data(rng, N, NQ, dim, dtype, metric)
        if dtype in ("float32", "float16") and metric == "l2":  # every sum of squares of differences below 2^24
            top = int(np.sqrt((2 ** 24 - 1) / dim))
            X, Q = np.minimum(X, top), np.minimum(Q, top)
        self.rows, self.Q = X, Q
        labels = (rng.permutation(N) + SHIFT).astype(np.int32)
        self.o, self.dev = _pair(oracle_mod, metric, dtype, X, M=M, efc=EFC, labels=labels)
        o = self.o
        self.labels = np.asarray(o.blob())[: N * o.node_size].reshape(N, o.node_size)[:, o.node_size - 4:].copy().view(np.int32).ravel()
        row_of_label = np.empty(N + SHIFT, np.int64)
        row_of_label[labels] = np.arange(N)
        self.X = X[row_of_label[self.labels]]  # rows in node order: the contract breaks distance ties by node id
        self.Qo = Q.astype(np.float32) if dtype == "float16" else Q  # the oracle holds float16 indexes widened, exactly
        self.D = _dist64(self.X, Q, metric)
        if dtype in ("float32", "float16"):
            assert np.abs(self.D).max() < 2 ** 24 and (self.D == np.rint(self.D)).all(), self.what
        start = int(rng.integers(0, N // 2))
        # empty, a random 10 %, a contiguous half, all -- and one more for the graph form: a random 1 %
        self.filters = [np.zeros(0, np.int64), rng.choice(N, N // 10, replace=False) + SHIFT, np.arange(start, start + N // 2) + SHIFT,
                        np.arange(N) + SHIFT]
        self.one_pct = rng.choice(N, N // 100, replace=False) + SHIFT
        self.qf = (np.arange(NQ) % (len(self.filters) + 1) - 1).astype(np.int32)  # -1, 0, 1, 2, 3, -1, ...: every tile mixes
        self.nodes_of = {-1: np.arange(N)}
        for g, f in enumerate(self.filters):
            self.nodes_of[g] = np.flatnonzero(np.isin(self.labels, f))

    def close(self):
        self.dev.close()


def _is_the_class(dtype, case):
    """The case is what it claims: the library's own layout and the planner's geometry give the class's key."""
    c = rc.walk(dtype)[case[: -len("-dense")] if case.endswith("-dense") else case]
    dim = rc.dim_of(dtype, case)
    assert dim == (c.dense_dim if case.endswith("-dense") else c.dim)
    cfg, full, row_bytes, tail_bytes = (int(v[0]) for v in rc.geometry(dtype, [dim], N))
    assert hip.row_layout(dim, dtype, N) == (row_bytes, tail_bytes), (dtype, dim)
    assert (cfg, bool(full), tail_bytes // 16) == (c.cfg, c.full, c.tail_chunks), (dtype, dim)
    assert (-(-(row_bytes // 16) // (c.G * c.CU)) > 1) == c.multi_span, (dtype, dim)
    return c, dim


@pytest.fixture(scope="module", params=INT_CASES, ids=lambda p: "-".join(p))
def case(request, oracle_mod):
    dtype, metric, name = request.param
    klass, dim = _is_the_class(dtype, name)
    c = Case(oracle_mod, dtype, metric, dim, name)
    c.klass = klass
    yield c
    c.close()


def _scan_steps(c, segments=(0, 100), Ks=(1, 10, 100)):
    dev, allowed = c.dev, c.filters[1]
    try:
        for K in Ks:
            want_all = _topk(c.D, c.nodes_of[-1], c.labels, K)
            want_f = _topk(c.D[:, c.nodes_of[1]], c.nodes_of[1], c.labels, K)
            for seg in segments:  # automatic, and six segments with a real merge
                dev.set_option("scan_segment_rows", seg)
                _equal(dev.search_exhaustive(c.Q, K, stats=True), want_all, c.what + (K, seg, "all"))
                _equal(dev.search_exhaustive(c.Q, K, allowed=allowed, stats=True), want_f, c.what + (K, seg, "10 %"))
                assert dev.launch_geometry()["kernel"] == "exhaustive_scan"
    finally:
        dev.set_option("scan_segment_rows", 0)


def _grouped_scan_steps(c, segments=(0, 100), Ks=(1, 10, 100)):
    dev = c.dev
    try:
        for K in Ks:
            for seg in segments:
                dev.set_option("scan_segment_rows", seg)
                got = dev.search_exhaustive_grouped(c.Q, K, c.filters, c.qf, stats=True)
                assert dev.launch_geometry()["kernel"] == "exhaustive_scan"
                for g in range(-1, len(c.filters)):
                    rows, nodes = np.flatnonzero(c.qf == g), c.nodes_of[g]
                    sub = (got[0][rows], got[1][rows], {k: got[2][k][rows] for k in SCAN_KEYS})
                    _equal(sub, _topk(c.D[rows][:, nodes], nodes, c.labels, K), c.what + (K, seg, g))
    finally:
        dev.set_option("scan_segment_rows", 0)


# ---- KS: the exhaustive scan -----------------------------------------------------------------------------------------------------
def test_scan(case):
    _scan_steps(case)


# ---- KSg: the grouped scan ---------------------------------------------------------------------------------------------------------
def test_grouped_scan(case):
    _grouped_scan_steps(case)


# ---- K1 / K2 / K0: the graph search, every beam form --------------------------------------------------------------------------------
def _first(result, n):
    return tuple({k: v[:n] for k, v in x.items()} if isinstance(x, dict) else x[:n] for x in result)


def _graph_steps(c, mirror):
    """Every form of the graph search against the oracle; `mirror`: whether the launches read the half-width mirror rows (the
    f32h kernel objects, the mirror branch of batch_dists) or the index's own table."""
    dev, o = c.dev, c.o

    def search(Q, K, ef, n_init=100):
        got = dev.search(Q, K, ef, n_init, stats=True)
        assert dev.half_rows()["used_by_last_launch"] == mirror, c.what + (mirror,)
        return got

    want = {ef: o.search(c.Qo, 10, ef, stats=True) for ef in (16, 100, 200)}
    dev.set_option("sorted_beam", 0)
    _same(search(c.Q, 10, 100), want[100], c.what + (mirror, "two heaps"))
    assert dev.launch_geometry()["kernel"] == "two_heaps"
    dev.set_option("sorted_beam", 1)
    # beams of 16, 100 and 200 entries: one, two and four 64-entry register chunks (beam_form in csrc/search_types.h picks the R
    # form from the beam width alone; launch_geometry names the kernel family, not R)
    for ef in (16, 100, 200):
        _same(search(c.Q, 10, ef), want[ef], c.what + (mirror, "registers", ef))
        assert dev.launch_geometry()["kernel"] == "merged_beam_registers", ef
    dev.set_option("beam_registers", 0)
    _same(search(c.Q, 10, 100), want[100], c.what + (mirror, "beam in LDS"))
    assert dev.launch_geometry()["kernel"] == "merged_beam_lds"
    dev.set_option("beam_registers", 1)
    # Four queries: the launch leaves the GPU idle, so every query gets an exact shadow and -- the index being small and the
    # visited table's shape unpinned -- the visited set is the DIRECT bitmap (lay_out_direct in csrc/launch_plan.hpp).  The
    # shadow flag is reported; the DIRECT form is not reported by launch_geometry or launch_info, so it is not asserted.
    _same(search(c.Q[:4], 10, 100), _first(want[100], 4), c.what + (mirror, "4 queries"))
    assert dev.launch_geometry()["kernel"] == "merged_beam_registers" and dev.launch_info()["shadow"]
    if not c.klass.tail_chunks:  # K0, the batch scan for entry points: the host never runs it on split rows
        for sorted_beam in (0, 1):
            dev.set_option("sorted_beam", sorted_beam)
            for n_init in (100, 7):
                w = o.search(c.Qo, 10, 64, n_init, stats=True)
                dev.set_option("entry_kernel", 0)
                inline = search(c.Q, 10, 64, n_init)
                dev.set_option("entry_kernel", 1)
                _same(search(c.Q, 10, 64, n_init), inline, c.what + (mirror, "entry kernel", sorted_beam, n_init))
                _same(inline, w, c.what + (mirror, "entries inline", sorted_beam, n_init))
        dev.set_option("entry_kernel", 0)


def test_graph_search_kernels(case):
    """A float32 index of FULL rows with an even CU searches a half-width mirror of its rows by default (the integer values are
    lossless in binary16): other kernel objects, another branch of batch_dists.  There the steps run twice -- on the float32
    table ("half_rows" = 0), which is what this class's float32 kernels are, and on the mirror -- and every launch says which."""
    c, dev, k = case, case.dev, case.klass
    eligible = c.dtype == "float32" and k.full and not k.tail_chunks and k.CU % 2 == 0  # half_rows_eligible, csrc/half_rows.hpp
    assert (dev.half_rows()["state"] == "live") == eligible, c.what + (dev.half_rows(),)
    try:
        for half_rows in ((0, 1) if eligible else (1,)):
            dev.set_option("half_rows", half_rows)
            _graph_steps(c, bool(eligible and half_rows))
    finally:
        dev.set_option("half_rows", 1)
        dev.set_option("entry_kernel", 0)
        dev.set_option("beam_registers", 1)
        dev.set_option("sorted_beam", 2)


# ---- K1f: the filtered search ------------------------------------------------------------------------------------------------------
def test_filtered_search(case):
    c, dev, o = case, case.dev, case.o
    for K, ef in ((1, 16), (10, 64), (100, 100)):
        _same(dev.search_filtered(c.Q, K, ef, c.filters[3], stats=True), dev.search(c.Q, K, ef, stats=True), c.what + (K, "all allowed"))
    view = dev.view()
    try:
        view.set_option("spill_entries", 1 << 18)  # a 1 % filter explores the whole graph; FNV_ERR_CAPACITY would raise, not pass
        for handle, allowed, how in ((dev, c.filters[1], "10 %"), (view, c.one_pct, "1 %")):
            for K, ef in ((1, 16), (10, 64)):
                want = filtered_ref.search_oracle_index(o, c.Qo, K, ef, allowed)
                _same(handle.search_filtered(c.Q, K, ef, allowed, stats=True), want, c.what + (K, how))
    finally:
        view.close()


# ---- the grouped graph form ----------------------------------------------------------------------------------------------------------
def test_grouped_filtered_search(case):
    c, dev = case, case.dev
    for K, ef in ((1, 16), (10, 64)):
        got = dev.search_filtered_grouped(c.Q, K, ef, c.filters, c.qf, stats=True)
        for g in range(-1, len(c.filters)):
            rows = np.flatnonzero(c.qf == g)
            single = dev.search(c.Q[rows], K, ef, stats=True) if g < 0 else dev.search_filtered(c.Q[rows], K, ef, c.filters[g], stats=True)
            _rows_equal(got, rows, single, GRAPH_KEYS, c.what + (K, g))


# ---- the device builder: wire_select / wire_connect in this class ---------------------------------------------------------------------
def test_sequential_device_insertion(case, flatnav, oracle_mod):
    """One node per device batch is the reference's sequential insertion, so the first 150 rows give the oracle's
    single-threaded graph byte for byte (link rows and labels; a float16 index narrows the vectors, exactly)."""
    c, n = case, 150
    metric = "angular" if c.metric == "ip" else "l2"
    X = c.rows[:n]
    labels = (c.rng.permutation(n) * 3 + 11).astype(np.int32)
    host_t = "float32" if c.dtype == "float16" else c.dtype
    o = oracle_mod.OracleIndex.create(metric, c.dim, n, M, host_t)
    o.add(X.astype(np.float32) if c.dtype == "float16" else X, EFC, labels=labels)
    ix = flatnav.index.create(metric, c.dim, n, M, getattr(flatnav.data_type.DataType, c.dtype))
    ix.add(X, EFC, labels=labels.tolist(), device=True, device_max_batch=1, device_bootstrap=1)
    assert ix._cur_num_nodes == n
    want = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)
    got = np.asarray(ix._raw_blob()).reshape(n, -1)
    if c.dtype == "float16":
        assert np.array_equal(got[:, : 2 * c.dim].copy().view(np.float16), X)
        want, got = want[:, o.data_size:], got[:, 2 * c.dim:]
    bad = np.flatnonzero((want != got).any(axis=1))
    assert bad.size == 0, c.what + ("first differing node %d of %d differing" % (bad[0], bad.size),)


# ---- the longest rows: the scan's tile of one query ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_scan_of_rows_beyond_the_block_budget(oracle_mod, metric):
    assert rc.class_of("float32", LONG_DIM) == "64x4-clamped-spans"
    c = Case(oracle_mod, "float32", metric, LONG_DIM, "64x4-clamped-spans")
    try:
        _scan_steps(c)
        assert c.dev.launch_geometry()["lds_bytes"] > 20480
        _grouped_scan_steps(c)
        g = c.dev.launch_geometry()
        assert g["lds_bytes"] > 20480 and g["tile_queries"] == 1, g
    finally:
        c.close()


# ---- float data ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=FLOAT_CASES, ids=lambda p: "-".join(p))
def float_index(request, oracle_mod):
    dtype, metric, name = request.param
    klass, dim = _is_the_class(dtype, name)
    X, Q = rc.float_case(dtype, metric, dim)
    _, _, dev = _build(oracle_mod, metric, dtype, X, M=32)  # labels = row numbers; 32 links: (nearly) every random row gets an inbound one
    yield request.param + (dim,), X, Q, dev
    dev.close()


def test_float_same_distance_bits_as_the_graph_search(float_index):
    what, X, Q, dev = float_index
    gd, gl, gst = dev.search(Q, N, N, stats=True)
    ed, el = dev.search_exhaustive(Q, N)
    print("row classes, graph search bits: %s %s %s dim %d: %d .. %d of %d nodes per query" % (what + (gst["count"].min(), gst["count"].max(), N)))
    # the graph search reaches (nearly) every node, so the comparison is not vacuous -- except on 1-d unit rows, which are +-1: a
    # graph of two points with 300 duplicates each, where a tenth of the nodes is asked for
    assert (gst["count"] > (0.9 * N if what[3] > 1 else N // 10)).all(), what
    by_label = np.empty((len(Q), N), np.uint32)
    np.put_along_axis(by_label, el.astype(np.int64), ed.view(np.uint32), 1)
    for q in range(len(Q)):
        n = int(gst["count"][q])
        assert np.array_equal(by_label[q, gl[q, :n]], gd[q, :n].view(np.uint32)), what + (q,)


def test_float_bar_with_nothing_left_out(float_index):
    """Every distance of every (query, row) within rtol 1e-5 / atol 1e-6 of the float64 distance of the values the index holds,
    and the list in the contract's order."""
    what, X, Q, dev = float_index
    D = _dist64(X, Q, what[1])  # float64 of the float16 values for a float16 index: its own rounding is far below the bar
    d, l, st = dev.search_exhaustive(Q, N, stats=True)
    assert (st["count"] == N).all() and (st["n_dist"] == N).all() and (np.sort(l, axis=1) == np.arange(N)).all()
    own = np.take_along_axis(D, l.astype(np.int64), 1)
    tol = ATOL + RTOL * np.abs(own)
    err = np.abs(d.astype(np.float64) - own)
    print("row classes, float bar: %s %s %s dim %d: worst |error| / tolerance = %.4f" % (what + (float((err / tol).max()),)))
    assert (err <= tol).all(), what
    assert (np.diff(d, axis=1) >= 0).all(), what
    true_sorted = np.sort(D, axis=1)
    assert (np.abs(d.astype(np.float64) - true_sorted) <= ATOL + RTOL * np.abs(true_sorted)).all(), what
