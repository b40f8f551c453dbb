"""Filter routing on the GPU ("filter_scan_max" / "filter_scan_on_overflow"): inside one filtered graph call, a query whose
filter allows few nodes -- or whose candidates heap overflows -- is answered by the exhaustive scan.

Everything goes through the C ABI (flatnav_amd.hip).  The oracles are the EXISTING entry points with both options off, which
their own test files pin: a scanned row must hold the bytes of fnv_search_batch_exhaustive[_grouped] for that query and filter
(and n_hops = 0), a graph row the bytes of fnv_search_batch_filtered[_grouped] -- the same arithmetic, so no tolerance, for
integer and float data alike."""
import ctypes
import os
import threading

import numpy as np
import pytest

from flatnav_amd import datasets as ds
from flatnav_amd import hip
from test_gpu_filtered import _int_data, _pair

pytestmark = pytest.mark.gpu
N, M = 600, 16
COUNTS = (0, 1, 5, 60, 300, 600)  # live nodes the six filters allow


@pytest.fixture(scope="module")
def flatnav():
    import flatnav_amd

    return flatnav_amd


def _index(oracle_mod, rng, dtype="float32", metric="l2", dim=32, nq=64, float_data=False):
    """A 600-row index with labels that are not node ids -> (device index, queries, labels)."""
    if float_data:
        X, Q = ds.randn(N, nq, dim, seed=int(rng.integers(1 << 30)))
    else:
        X, Q = _int_data(rng, N, nq, dim, dtype, metric)
    labels = (rng.permutation(N) + 3).astype(np.int32)
    _, dev = _pair(oracle_mod, metric, dtype, X, M=M, efc=32, labels=labels)
    return dev, Q, labels


def _six_filters(rng, labels):
    """Label sets that allow 0, 1, 5, 60, 300 and 600 live nodes (labels are distinct: one node each)."""
    return [rng.choice(labels, c, replace=False).astype(np.int64) for c in COUNTS]


def _routing(dev, scan_max, on_overflow=0):
    dev.set_option("filter_scan_max", scan_max)
    dev.set_option("filter_scan_on_overflow", on_overflow)


def _check_rows(got, scanned, graph, scan, what):
    """Row by row: `scanned` rows are the scan oracle's with n_hops 0, the others the graph oracle's with at least one hop."""
    gd, gl, gst = got
    scanned = np.asarray(scanned, bool)
    for rows, want, keys in ((scanned, scan, ("count", "n_dist")), (~scanned, graph, ("count", "n_dist", "n_hops"))):
        assert np.array_equal(gl[rows], want[1][rows]), what
        assert np.array_equal(gd[rows].view(np.uint32), want[0][rows].view(np.uint32)), what
        for key in keys:
            assert np.array_equal(np.asarray(gst[key])[rows].astype(np.int64), np.asarray(want[2][key])[rows].astype(np.int64)), (what, key)
    hops = np.asarray(gst["n_hops"]).astype(np.int64)
    assert (hops[scanned] == 0).all(), what  # how a caller tells a scanned row ...
    assert (hops[~scanned] >= 1).all(), what  # ... from a graph row: a graph search expands its entry node


def _allowed_count(qf, counts):
    """Live nodes the filter row of each query allows: a -1 row counts every live node."""
    return np.where(qf < 0, N, np.asarray(counts)[np.maximum(qf, 0)])


# ---- 1. threshold routing, every element type and metric, split rows and long rows ---------------------------------------------
SHAPES = [(dtype, metric, 128, False) for dtype in ("float32", "float16", "uint8", "int8") for metric in ("l2", "ip")] + [
    ("float32", "l2", 100, False), ("float32", "l2", 768, False), ("float32", "l2", 64, True), ("float32", "ip", 64, True)]


@pytest.mark.parametrize("dtype,metric,dim,float_data", SHAPES)
def test_threshold_routing(oracle_mod, dtype, metric, dim, float_data):
    rng = np.random.default_rng(dim + 7 * len(dtype) + len(metric) + float_data)
    dev, Q, labels = _index(oracle_mod, rng, dtype, metric, dim, nq=70, float_data=float_data)
    filters = _six_filters(rng, labels)
    qf = rng.permutation(np.repeat(np.arange(-1, 6), 10)).astype(np.int32)  # ten queries per row, the -1 row rides along
    allowed = _allowed_count(qf, COUNTS)
    K, ef = 10, 32
    graph = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)  # both options off: the oracles
    geom = dev.launch_geometry()
    scan = dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)
    assert (np.asarray(graph[2]["n_hops"]) >= 1).all()
    for scan_max in (60, 59, 0, 600):  # rows at exactly the threshold scan; 0 is off; 600 sends every row, -1 included
        _routing(dev, scan_max)
        got = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
        want_scanned = (allowed <= scan_max) & (scan_max > 0)
        _check_rows(got, want_scanned, graph, scan, (dtype, metric, dim, float_data, scan_max))
        if scan_max == 0:
            assert dev.launch_geometry() == geom
    assert int(want_scanned.sum()) == len(qf)
    _routing(dev, 0)


# ---- 2. subset shapes that can go wrong ------------------------------------------------------------------------------------------
def test_subset_shapes(oracle_mod):
    rng = np.random.default_rng(202)
    dev, Qall, labels = _index(oracle_mod, rng, nq=64)
    few, many = rng.choice(labels, 5, replace=False), rng.choice(labels, 300, replace=False)
    filters = [few, many]
    K, ef = 10, 32
    dev.search_exhaustive_grouped(Qall[:33], K, filters, np.zeros(33, np.int32))
    tile = dev.launch_geometry()["tile_queries"]
    assert tile == 32
    nq = tile + 1
    Q = Qall[:nq]
    for n_scanned in (0, 1, tile, nq):  # the scanned subset: none, one, exactly a tile, all -- interleaved with graph queries
        qf = np.ones(nq, np.int32)
        qf[rng.choice(nq, n_scanned, replace=False)] = 0
        graph = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
        scan = dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)
        for segment_rows in (0, 64):  # 64: ten row segments on 600 rows, so the merge runs on the subset
            dev.set_option("scan_segment_rows", segment_rows)
            _routing(dev, 5)
            got = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
            _check_rows(got, qf == 0, graph, scan, ("subset", n_scanned, segment_rows))
            _routing(dev, 0)
        dev.set_option("scan_segment_rows", 0)
    # nq = 1, either way
    for g in (0, 1):
        qf = np.full(1, g, np.int32)
        graph = dev.search_filtered_grouped(Qall[:1], K, ef, filters, qf, stats=True)
        scan = dev.search_exhaustive_grouped(Qall[:1], K, filters, qf, stats=True)
        _routing(dev, 5)
        _check_rows(dev.search_filtered_grouped(Qall[:1], K, ef, filters, qf, stats=True), qf == 0, graph, scan, ("nq = 1", g))
        _routing(dev, 0)
    # K = 1, K above the candidate count (padding), K = 1024 (two queries per tile)
    qf = rng.permutation(np.repeat([0, 1, -1], 11)).astype(np.int32)
    for K in (1, 100, 1024):
        ef = max(K, 32)
        graph = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
        scan = dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)
        for segment_rows in (0, 64):
            dev.set_option("scan_segment_rows", segment_rows)
            _routing(dev, 300)
            got = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
            _check_rows(got, qf >= 0, graph, scan, ("K", K, segment_rows))
            _routing(dev, 0)
        dev.set_option("scan_segment_rows", 0)
        if K > 5:
            assert (got[2]["count"][qf == 0] == 5).all() and (got[1][qf == 0][:, 5:] == -1).all() and np.isposinf(got[0][qf == 0][:, 5:]).all()
    # K = 1025: the scan cannot take the call, so routing is not applied -- the plain graph call, its bytes, no error
    graph = dev.search_filtered_grouped(Q, 1025, 1025, filters, qf, stats=True)
    geom = dev.launch_geometry()
    _routing(dev, 600, 1)
    got = dev.search_filtered_grouped(Q, 1025, 1025, filters, qf, stats=True)
    _check_rows(got, np.zeros(nq, bool), graph, graph, "K = 1025")
    assert dev.launch_geometry() == geom
    _routing(dev, 0)


# ---- 3. the single-filter entry points, host and _device -------------------------------------------------------------------------
def _device_call(dev, Q, K, ef, run, graph_form=True):
    """Runs a _device entry point on torch buffers: run(pointers...) enqueues; -> (dist, labels, stats)."""
    import torch

    nq = len(Q)
    cuda = torch.device("cuda", dev.device)
    tq = torch.from_numpy(Q).to(cuda)
    td = torch.empty((nq, K), dtype=torch.float32, device=cuda)
    tl = torch.empty((nq, K), dtype=torch.int32, device=cuda)
    tc = torch.empty(nq, dtype=torch.int32, device=cuda)
    tnd = torch.zeros(nq, dtype=torch.int64, device=cuda)
    tnh = torch.full((nq,), 77, dtype=torch.int64, device=cuda)
    stream = torch.cuda.Stream(cuda)
    torch.cuda.synchronize(cuda)
    with torch.cuda.stream(stream):
        run(tq, td, tl, tc, tnd, tnh, stream.cuda_stream)
    stream.synchronize()
    dev.status()
    return td.cpu().numpy(), tl.cpu().numpy(), {"count": tc.cpu().numpy(), "n_dist": tnd.cpu().numpy(), "n_hops": tnh.cpu().numpy()}


@pytest.mark.parametrize("float_data", [False, True])
def test_single_filter_entry_points(oracle_mod, float_data):
    import torch

    rng = np.random.default_rng(303 + float_data)
    dev, Q, labels = _index(oracle_mod, rng, dim=64, nq=40, float_data=float_data)
    K, ef = 10, 32
    nq = len(Q)
    for count in (0, 5, 60):
        allowed = rng.choice(labels, count, replace=False).astype(np.int64)
        bits, n_bits = hip.pack_allowed(allowed)
        graph = dev.search_filtered(Q, K, ef, allowed, stats=True)
        scan = dev.search_exhaustive(Q, K, allowed, stats=True)
        tb = torch.from_numpy(bits).to(torch.device("cuda", dev.device)) if n_bits else None

        def on_device(tq, td, tl, tc, tnd, tnh, stream):
            dev.search_device_filtered(tq.data_ptr(), nq, K, ef, 100, tb.data_ptr() if tb is not None else 0, n_bits, td.data_ptr(),
                                       tl.data_ptr(), tc.data_ptr(), tnd.data_ptr(), tnh.data_ptr(), stream=stream)

        # the whole batch goes one way: the threshold above or at the filter's count (scan) or below it (graph; 0 is off)
        for scan_max in sorted({count + 1, count, max(count - 1, 0)}):
            _routing(dev, scan_max)
            want = np.full(nq, scan_max > 0 and count <= scan_max)
            _check_rows(dev.search_filtered(Q, K, ef, allowed, stats=True), want, graph, scan, ("host", count, scan_max))
            _check_rows(_device_call(dev, Q, K, ef, on_device), want, graph, scan, ("device", count, scan_max))
        _routing(dev, 0)
        _check_rows(dev.search_filtered(Q, K, ef, allowed, stats=True), np.zeros(nq, bool), graph, scan, ("off again", count))


# ---- 4. the _device grouped call with out-of-range query_filter values ----------------------------------------------------------
def test_device_grouped_call_with_out_of_range_values(oracle_mod):
    import torch

    rng = np.random.default_rng(404)
    dev, Q, labels = _index(oracle_mod, rng, nq=50)
    filters = _six_filters(rng, labels)
    table, n_bits = hip.pack_filters(filters)
    K, ef, nq = 10, 32, len(Q)
    qf = rng.permutation(np.resize(np.arange(-1, 6), nq)).astype(np.int32)
    bad_rows = np.array([0, 7, 23, 49])
    bad = qf.copy()
    bad[bad_rows] = [6, -2, 2**31 - 1, -2**31]  # just past the table on either side, and the ends of int32
    is_bad = np.isin(np.arange(nq), bad_rows)
    graph = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
    scan = dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)
    cuda = torch.device("cuda", dev.device)
    tt = torch.from_numpy(table).to(cuda)

    def run(values):
        tf = torch.from_numpy(np.ascontiguousarray(values, np.int32)).to(cuda)

        def on_device(tq, td, tl, tc, tnd, tnh, stream):
            dev.search_device_filtered_grouped(tq.data_ptr(), nq, K, ef, 100, tt.data_ptr(), len(filters), table.shape[1], n_bits,
                                               tf.data_ptr(), td.data_ptr(), tl.data_ptr(), tc.data_ptr(), tnd.data_ptr(), tnh.data_ptr(),
                                               stream=stream)

        return _device_call(dev, Q, K, ef, on_device)

    _routing(dev, 5)
    scanned = _allowed_count(qf, COUNTS) <= 5
    _check_rows(run(qf), scanned, graph, scan, "device entry point, values in range")
    got = run(bad)
    keep = ~is_bad
    _check_rows(tuple(x[keep] if not isinstance(x, dict) else {k: v[keep] for k, v in x.items()} for x in got), scanned[keep],
                tuple(x[keep] if not isinstance(x, dict) else {k: np.asarray(v)[keep] for k, v in x.items()} for x in graph),
                tuple(x[keep] if not isinstance(x, dict) else {k: np.asarray(v)[keep] for k, v in x.items()} for x in scan), "other rows")
    # the empty row counts 0 nodes: it is scanned, and comes back empty
    assert np.isposinf(got[0][is_bad]).all() and (got[1][is_bad] == -1).all()
    assert (got[2]["count"][is_bad] == 0).all() and (got[2]["n_dist"][is_bad] == 0).all() and (got[2]["n_hops"][is_bad] == 0).all()
    _routing(dev, 0)


# ---- 5. overflow routing ------------------------------------------------------------------------------------------------------------
def _overflow_index(oracle_mod):
    """600 rows in two far-apart clusters; the 1 % filter allows six nodes packed tightly inside the first.  A query next to them
    fills its beam of four at once and keeps a small candidates heap; a query in the other cluster walks that whole cluster
    first, every node of it a candidate.  (A sequential model of the filtered search on this data, K = ef = 4, puts the heap's
    peak at 13 - 28 entries for the near queries and 165 - 196 for the far ones, over several seeds and build orders: the
    capacity of 96 + 1 entries that the test forces lies far from both.)"""
    rng = np.random.default_rng(505)
    dim = 16
    A = rng.integers(0, 40, (300, dim))
    A[:6] = 20 + rng.integers(0, 2, (6, dim))  # the allowed six, within a unit cube
    B = 2000 + rng.integers(0, 40, (300, dim))
    X = np.concatenate([A, B]).astype(np.float32)
    labels = (rng.permutation(N) + 3).astype(np.int32)
    near = (20 + rng.integers(0, 2, (8, dim))).astype(np.float32)
    far = (2000 + rng.integers(0, 40, (8, dim))).astype(np.float32)
    Q = np.empty((16, dim), np.float32)
    Q[0::2], Q[1::2] = near, far  # interleaved
    _, dev = _pair(oracle_mod, "l2", "float32", X, M=M, efc=32, labels=labels)
    return dev, Q, labels[:6].astype(np.int64)


@pytest.mark.parametrize("scan_max", [0, 3])
def test_overflow_routing(oracle_mod, scan_max):
    dev, Q, allowed = _overflow_index(oracle_mod)
    K, ef, nq = 4, 4, len(Q)
    scan = dev.search_exhaustive(Q, K, allowed, stats=True)
    graph = dev.search_filtered(Q, K, ef, allowed, stats=True)  # default capacity: every query answered
    dev.set_option("cand_slots", 96)
    dev.set_option("spill_entries", 1)
    # the precondition, with the option off: the call fails, and single-query calls tell which queries overflow
    with pytest.raises(RuntimeError, match="spill"):
        dev.search_filtered(Q, K, ef, allowed)
    overflows = np.zeros(nq, bool)
    for q in range(nq):
        try:
            one = dev.search_filtered(Q[q:q + 1], K, ef, allowed, stats=True)
            assert np.array_equal(one[1], graph[1][q:q + 1])  # (an answered query is answered as with the default capacity)
        except RuntimeError:
            overflows[q] = True
    print("overflowing queries:", np.flatnonzero(overflows))
    assert overflows.any() and not overflows.all()
    # the option on (alone, or together with a threshold below the filter's six nodes): OK, and every row from the right engine
    _routing(dev, scan_max, 1)
    got = dev.search_filtered(Q, K, ef, allowed, stats=True)
    _check_rows(got, overflows, graph, scan, ("overflow routing", scan_max))
    # ... the grouped form and a threshold that pre-routes some rows: both routes in one call
    filters = [allowed, np.zeros(0, np.int64)]
    qf = np.zeros(nq, np.int32)
    qf[[2, 3]] = 1
    grouped = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
    same = qf == 0  # these rows: the single-filter call's, whichever engine answered them
    assert np.array_equal(grouped[1][same], got[1][same]) and np.array_equal(grouped[0][same].view(np.uint32), got[0][same].view(np.uint32))
    for key in ("count", "n_dist", "n_hops"):
        assert np.array_equal(np.asarray(grouped[2][key])[same], np.asarray(got[2][key])[same]), key
    assert (grouped[1][~same] == -1).all() and np.isposinf(grouped[0][~same]).all() and (grouped[2]["count"][~same] == 0).all()
    if scan_max:  # (the empty row counts 0 nodes: scanned before the search kernel sees it)
        assert (np.asarray(grouped[2]["n_hops"])[~same] == 0).all() and (np.asarray(grouped[2]["n_dist"])[~same] == 0).all()
    # off again: the capacity error is back
    _routing(dev, 0, 0)
    with pytest.raises(RuntimeError, match="spill"):
        dev.search_filtered(Q, K, ef, allowed)


# ---- 6. host threads on one handle --------------------------------------------------------------------------------------------------
def test_four_host_threads_on_one_handle(oracle_mod):
    rng = np.random.default_rng(606)
    dev, Q, labels = _index(oracle_mod, rng, nq=64)
    filters = _six_filters(rng, labels)
    K, ef = 10, 32
    qfs = [rng.permutation(np.resize(np.arange(-1, 6), len(Q))).astype(np.int32) for _ in range(3)]
    single = filters[2]
    _routing(dev, 60, 1)
    calls = [lambda qf=qf: dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True) for qf in qfs] + [
        lambda: dev.search_filtered(Q, K, ef, single, stats=True)]
    want = [c() for c in calls]  # serial
    for qf, w in zip(qfs, want):
        assert np.array_equal(np.asarray(w[2]["n_hops"]) == 0, _allowed_count(qf, COUNTS) <= 60)
    assert (np.asarray(want[3][2]["n_hops"]) == 0).all()
    errors = []

    def worker(i):
        try:
            for _ in range(5):
                got = calls[i]()
                assert np.array_equal(got[1], want[i][1]) and np.array_equal(got[0].view(np.uint32), want[i][0].view(np.uint32))
                for key in ("count", "n_dist", "n_hops"):
                    assert np.array_equal(got[2][key], want[i][2][key]), key
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    # fnv_lane_info: the hidden lanes together stay within their budget, an eighth of the device's memory unless the environment
    # says otherwise -- with the routed calls' bitmaps, grouping arrays, route words and partial lists counted
    import torch

    budget = torch.cuda.get_device_properties(dev.device).total_memory // 8
    if os.environ.get("FLATNAV_LANE_BUDGET_MB"):
        budget = int(os.environ["FLATNAV_LANE_BUDGET_MB"]) << 20
    used = hip.lane_workspaces(dev)
    assert sum(used[1:]) <= budget, (used, budget)
    _routing(dev, 0, 0)


# ---- 7. the Python surface ------------------------------------------------------------------------------------------------------------
def test_python_surface(flatnav):
    rng = np.random.default_rng(707)
    dim = 16
    X, Q = _int_data(rng, N, 32, dim, "float32", "l2")
    index = flatnav.index.create("l2", dim, N, M)
    index.set_num_threads(1)
    index.add(X, 32)
    filters = [rng.choice(N, c, replace=False) for c in COUNTS]
    qf = rng.permutation(np.resize(np.arange(-1, 6), len(Q))).astype(np.int32)
    dev = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)
    graph = dev.search_filtered_grouped(Q, 10, 32, filters, qf, stats=True)
    scan = dev.search_exhaustive_grouped(Q, 10, filters, qf, stats=True)
    index.set_filter_routing(scan_max_allowed=60)
    d, l = index.search_filtered_grouped(Q, 10, 32, filters, qf)
    want = dev.search_filtered_grouped(Q, 10, 32, filters, qf, stats=True)  # the C ABI on the same handle: the option is on there
    assert np.array_equal(l, want[1]) and np.array_equal(d.view(np.uint32), want[0].view(np.uint32))
    _check_rows(want, _allowed_count(qf, COUNTS) <= 60, graph, scan, "set_filter_routing")
    # overflow routing: no exception where one was raised before
    index.set_filter_routing()
    dev.set_option("cand_slots", 1)
    dev.set_option("spill_entries", 1)
    with pytest.raises(RuntimeError):
        index.search_filtered_grouped(Q, 10, 10, filters, qf)
    with pytest.raises(RuntimeError):
        index.search_filtered(Q, 10, 10, filters[1])
    index.set_filter_routing(scan_on_overflow=True)
    d, l = index.search_filtered_grouped(Q, 10, 10, filters, qf)
    d1, l1 = index.search_filtered(Q, 10, 10, filters[1])
    one = dev.search_exhaustive(Q, 10, filters[1])
    assert np.array_equal(l1, one[1])  # (a beam of ten never fills from one allowed node: every query overflows and is scanned)
    index.set_filter_routing()
    with pytest.raises(RuntimeError):
        index.search_filtered(Q, 10, 10, filters[1])
