"""Grouped filters on the GPU (fnv_search_batch_{filtered,exhaustive}_grouped[_device], DeviceIndex.search_*_grouped, _core):
one allowed set per query in one launch.

The rule under test: row q of a grouped call holds exactly the bytes the single-filter call writes for that query with filter
query_filter[q] (the unfiltered call for -1) -- labels, distance bits and counters.  So the yardsticks are the single-filter
calls themselves, which their own test files pin; the exhaustive form is also held to the plain-numpy reference of
test_gpu_exhaustive, and one selective group of the graph form to the CPU restatement of the filtered search."""
import ctypes
import threading

import numpy as np
import pytest

import filtered_ref
from flatnav_amd import datasets as ds
from flatnav_amd import hip
from test_gpu_exhaustive import _build, _dist64, _equal, _topk
from test_gpu_filtered import _int_data, _pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def flatnav():
    import flatnav_amd

    return flatnav_amd


def _rows_equal(got, rows, want, keys, what):
    """Rows `rows` of the grouped result `got` are the single call's result `want` on those queries, bit for bit."""
    assert np.array_equal(got[1][rows], want[1]), what
    assert np.array_equal(got[0][rows].view(np.uint32), want[0].view(np.uint32)), what
    for key in keys:
        assert np.array_equal(np.asarray(got[2][key])[rows].astype(np.int64), np.asarray(want[2][key]).astype(np.int64)), (what, key)


GRAPH_KEYS = ("count", "n_dist", "n_hops")
SCAN_KEYS = ("count", "n_dist")


def _five_filters(rng, n, shift):
    """Label sets over the labels shift .. shift + n - 1: 50 % random, 10 % contiguous, one label, none, all."""
    start = int(rng.integers(0, n - n // 10))
    return [rng.choice(n, n // 2, replace=False) + shift, np.arange(start, start + n // 10) + shift,
            np.array([int(rng.integers(n)) + shift]), np.zeros(0, np.int64), np.arange(n) + shift]


def _mixed_query_filter(rng, nq, F):
    """Every value of -1 .. F - 1 at least once, in shuffled order."""
    qf = np.concatenate([np.arange(-1, F), rng.integers(-1, F, nq - F - 1)])
    return rng.permutation(qf).astype(np.int32)


def _graph_single(dev, Q, rows, K, ef, filters, g):
    if g < 0:
        return dev.search(Q[rows], K, ef, stats=True)
    return dev.search_filtered(Q[rows], K, ef, filters[g], stats=True)


def _scan_single(dev, Q, rows, K, filters, g):
    return dev.search_exhaustive(Q[rows], K, allowed=None if g < 0 else filters[g], stats=True)


# ---- 1. every kernel shape, graph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "uint8", "int8"])
@pytest.mark.parametrize("dim", [7, 100, 128, 200, 768])
def test_every_kernel_shape_graph(oracle_mod, dtype, metric, dim):
    rng = np.random.default_rng(dim * 13 + len(dtype) + len(metric))
    n = 1500 if dim >= 200 else 2500
    X, Q = _int_data(rng, n, 48, dim, dtype, metric)
    labels = (rng.permutation(n) + 3).astype(np.int32)
    o, dev = _pair(oracle_mod, metric, dtype, X, labels=labels)
    filters = _five_filters(rng, n, 3)
    qf = _mixed_query_filter(rng, len(Q), len(filters))
    for K, ef in ((1, 16), (10, 64), (100, 100)):
        got = dev.search_filtered_grouped(Q, K, ef, filters, qf, stats=True)
        for g in range(-1, len(filters)):
            rows = np.flatnonzero(qf == g)
            _rows_equal(got, rows, _graph_single(dev, Q, rows, K, ef, filters, g), GRAPH_KEYS, (dtype, metric, dim, K, g))
        if dtype != "float16":  # one selective group against the restatement: the yardstick is not only the product
            rows = np.flatnonzero(qf == 1)
            wd, wl, wst = filtered_ref.search_oracle_index(o, Q[rows], K, ef, filters[1])
            _rows_equal(got, rows, (wd, wl, wst), GRAPH_KEYS, (dtype, metric, dim, K, "restatement"))


# ---- 2. every kernel shape, exhaustive ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "uint8", "int8"])
@pytest.mark.parametrize("dim", [7, 100, 128, 200, 768])
def test_every_kernel_shape_exhaustive(oracle_mod, dtype, metric, dim):
    rng = np.random.default_rng(dim * 17 + len(dtype) + len(metric))
    n = 1500 if dim >= 200 else 2500
    X, Q = _int_data(rng, n, 48, dim, dtype, metric)
    labels = (rng.permutation(n) + 3).astype(np.int32)
    X, labels, dev = _build(oracle_mod, metric, dtype, X, labels, efc=32)
    filters = _five_filters(rng, n, 3)
    qf = _mixed_query_filter(rng, len(Q), len(filters))
    D = _dist64(X, Q, metric)
    nodes_of = {-1: np.arange(n)}
    for g, f in enumerate(filters):
        nodes_of[g] = np.flatnonzero(np.isin(labels, f))
    for K in (1, 10, 100):
        results = []
        for seg in (0, 256):
            dev.set_option("scan_segment_rows", seg)
            got = dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)
            results.append(got)
            for g in range(-1, len(filters)):
                rows = np.flatnonzero(qf == g)
                sub = (got[0][rows], got[1][rows], {k: got[2][k][rows] for k in SCAN_KEYS})
                _equal(sub, _topk(D[rows][:, nodes_of[g]], nodes_of[g], labels, K), (dtype, metric, dim, K, seg, g))
                _rows_equal(got, rows, _scan_single(dev, Q, rows, K, filters, g), SCAN_KEYS, (dtype, metric, dim, K, seg, g, "single"))
        _rows_equal(results[0], np.arange(len(Q)), results[1], SCAN_KEYS, (dtype, metric, dim, K, "segments"))
    dev.set_option("scan_segment_rows", 0)


# ---- 3. edges of tiles and of bits ----------------------------------------------------------------------------------------------
def _check_scan(dev, X, labels, Q, D, K, filters, qf, what, n_live=None):
    got = dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)
    live = len(X) if n_live is None else n_live
    for g in np.unique(qf):
        rows = np.flatnonzero(qf == g)
        nodes = np.arange(live) if g < 0 else np.flatnonzero(np.isin(labels[:live], filters[g]))
        sub = (got[0][rows], got[1][rows], {k: got[2][k][rows] for k in SCAN_KEYS})
        _equal(sub, _topk(D[rows][:, nodes], nodes, labels, K), (what, K, int(g)))
    return got


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 2049])
def test_edges_of_tiles_and_bits(oracle_mod, n):
    rng = np.random.default_rng(300 + n)
    X, Qall = _int_data(rng, n, 257, 32, "float32", "l2")
    labels = (rng.permutation(n) + 3).astype(np.int32)
    X, labels, dev = _build(oracle_mod, "l2", "float32", X, labels, M=8, efc=16)
    Dall = _dist64(X, Qall, "l2")
    word = labels[32:64] if n >= 64 else labels[: min(32, n)]  # every bit of one 32-node word (and none of the next)
    filters = [labels[:1], labels[n - 1:], word, rng.choice(labels, max(1, n // 2), replace=False), labels.copy(),
               np.zeros(0, np.int64)]
    sizes = [1, 31, 32, 33, 64, 96]  # around the tile of 32 queries
    qf257 = rng.permutation(np.repeat(np.arange(6), sizes)).astype(np.int32)
    for K in sorted({1, min(n, 1024), 1024}):  # K > candidates in most groups: padding and counts
        got = _check_scan(dev, X, labels, Qall, Dall, K, filters, qf257, ("groups", n))
        geom = dev.launch_geometry()
        assert geom["kernel"] == "exhaustive_scan" and geom["queue_ids"] == 256 and geom["lds_bytes"] <= 20 * 1024, geom
        tile = geom["tile_queries"]
        assert tile == (32 if K == 1 else tile) and 1 <= tile <= 32
        bound = min(257, -(-257 // tile) + 8)
        assert geom["grid_blocks"] == bound * geom["segments"], geom
        for g in range(6):  # ... and the bytes of the single-filter call
            rows = np.flatnonzero(qf257 == g)
            _rows_equal(got, rows, _scan_single(dev, Qall, rows, K, filters, g), SCAN_KEYS, (n, K, g))
        own = [rng.choice(labels, int(rng.integers(0, n + 1)), replace=False) for _ in range(257)]
        _check_scan(dev, X, labels, Qall, Dall, K, own, np.arange(257, dtype=np.int32), ("own filter each", n))
        for nq in (1, 3, 257):
            Q, D = Qall[:nq], Dall[:nq]
            if nq < 257:
                _check_scan(dev, X, labels, Q, D, K, own[:nq], np.arange(nq, dtype=np.int32), ("own filter each", n, nq))
            _check_scan(dev, X, labels, Q, D, K, filters, np.full(nq, 3, np.int32), ("all in one", n, nq))
            _check_scan(dev, X, labels, Q, D, K, filters, np.full(nq, -1, np.int32), ("all unfiltered", n, nq))
            _check_scan(dev, X, labels, Q, D, K, [], np.full(nq, -1, np.int32), ("no filters at all", n, nq))
    # the graph form on the same groups: the bytes of the single-filter calls
    K, ef = min(n, 10), 32
    got = dev.search_filtered_grouped(Qall, K, ef, filters, qf257, stats=True)
    for g in range(6):
        rows = np.flatnonzero(qf257 == g)
        _rows_equal(got, rows, _graph_single(dev, Qall, rows, K, ef, filters, g), GRAPH_KEYS, ("graph", n, g))
    got = dev.search_filtered_grouped(Qall[:3], K, ef, [], np.full(3, -1, np.int32), stats=True)
    _rows_equal(got, np.arange(3), dev.search(Qall[:3], K, ef, stats=True), GRAPH_KEYS, ("graph, no filters at all", n))


# ---- 4. labels and live count ---------------------------------------------------------------------------------------------------
def test_labels_and_live_count(oracle_mod):
    rng = np.random.default_rng(41)
    n, nq, dim, M = 3000, 60, 32, 16
    X, Q = _int_data(rng, n, nq, dim, "float32", "l2")
    o, _ = _pair(oracle_mod, "l2", "float32", X, M=M, efc=32)
    blob = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size).copy()
    Xn = blob[:, : o.data_size].copy().view(np.float32)  # rows in node order
    labels = rng.integers(0, 40, n).astype(np.int32)      # many nodes share a label
    labels[rng.choice(n, 300, replace=False)] = -rng.integers(1, 9, 300).astype(np.int32)  # negative labels
    labels[rng.choice(n, 100, replace=False)] = 1000      # far beyond every filter's bits
    blob[:, o.node_size - 4:] = labels.view(np.uint8).reshape(n, 4)
    dev = hip.DeviceIndex.upload(blob.reshape(-1), o.node_size, o.data_size, M, n, "float32", "l2", dim)
    D = _dist64(Xn, Q, "l2")
    filters = [np.array([0, 1, 2]), np.arange(10, 30), np.array([39]), np.array([7, 63])]  # n_bits = 64 < 1000
    qf = _mixed_query_filter(rng, nq, len(filters))

    def check(handle, live, what):
        got = _check_scan(handle, Xn, labels, Q, D, 50, filters, qf, what, n_live=live)
        filtered = qf >= 0
        assert (got[1][filtered] >= -1).all() and (got[1][filtered] != 1000).all()  # (-1 is the padding)
        assert (got[1][~filtered] < -1).any() and (got[1][~filtered] == 1000).any()  # candidates when there is no filter
        ggot = handle.search_filtered_grouped(Q, 10, 64, filters, qf, stats=True)
        for g in range(-1, len(filters)):
            rows = np.flatnonzero(qf == g)
            _rows_equal(got, rows, _scan_single(handle, Q, rows, 50, filters, g), SCAN_KEYS, (what, "scan", g))
            if g >= 0 or live == n:  # (an unfiltered graph search of a graph cut below its wiring follows links past the live count)
                _rows_equal(ggot, rows, _graph_single(handle, Q, rows, 10, 64, filters, g), GRAPH_KEYS, (what, "graph", g))
        assert (ggot[1][qf >= 0] >= -1).all() and (ggot[1][qf >= 0] != 1000).all()
        return got, ggot

    whole = check(dev, n, "whole")
    dev.set_live_nodes(n // 2 + 7)  # (not a multiple of 32: the last live word is partly dead)
    half = check(dev, n // 2 + 7, "live half")
    view = dev.view()
    via_view = check(view, n // 2 + 7, "view")
    for a, b in zip(half, via_view):
        _rows_equal(a, np.arange(nq), b, tuple(a[2]), "view: the same bytes")
    view.close()
    dev.set_live_nodes(n)
    _rows_equal(whole[0], np.arange(nq), dev.search_exhaustive_grouped(Q, 50, filters, qf, stats=True), SCAN_KEYS, "whole again")
    dev.set_option("output_node_ids", 1)
    ids = np.arange(n, dtype=np.int32)
    got = dev.search_exhaustive_grouped(Q, 50, filters, qf, stats=True)
    for g in range(-1, len(filters)):
        rows = np.flatnonzero(qf == g)
        nodes = np.arange(n) if g < 0 else np.flatnonzero(np.isin(labels, filters[g]))
        sub = (got[0][rows], got[1][rows], {k: got[2][k][rows] for k in SCAN_KEYS})
        _equal(sub, _topk(D[rows][:, nodes], nodes, ids, 50), ("node ids", g))
    ggot = dev.search_filtered_grouped(Q, 10, 64, filters, qf, stats=True)
    for g in range(-1, len(filters)):
        rows = np.flatnonzero(qf == g)
        _rows_equal(ggot, rows, _graph_single(dev, Q, rows, 10, 64, filters, g), GRAPH_KEYS, ("node ids, graph", g))


# ---- 5. float data: the same arithmetic, so the same bits ---------------------------------------------------------------------
def test_float_data_equals_the_single_filter_calls(oracle_mod):
    n, nq = 5000, 200
    X, Q = ds.randn(n, nq, 64, seed=29)
    _, dev = _pair(oracle_mod, "l2", "float32", X)
    rng = np.random.default_rng(5)
    filters = [rng.choice(n, n // 2, replace=False), np.arange(1000, 1500), rng.choice(n, 50, replace=False), np.arange(n)]
    qf = _mixed_query_filter(rng, nq, len(filters))
    graph = dev.search_filtered_grouped(Q, 10, 64, filters, qf, stats=True)
    scan = dev.search_exhaustive_grouped(Q, 10, filters, qf, stats=True)
    for g in range(-1, len(filters)):
        rows = np.flatnonzero(qf == g)
        _rows_equal(graph, rows, _graph_single(dev, Q, rows, 10, 64, filters, g), GRAPH_KEYS, ("graph", g))
        _rows_equal(scan, rows, _scan_single(dev, Q, rows, 10, filters, g), SCAN_KEYS, ("scan", g))


# ---- 6. device-pointer entry points -----------------------------------------------------------------------------------------------
def test_device_entry_points(oracle_mod):
    import torch

    rng = np.random.default_rng(61)
    n, nq, K = 3000, 100, 10
    X, Q = _int_data(rng, n, nq, 64, "float32", "l2")
    _, dev = _pair(oracle_mod, "l2", "float32", X, efc=32)
    filters = [rng.choice(n, n // 10, replace=False), np.arange(500, 900), np.arange(n)]
    table, n_bits = hip.pack_filters(filters)
    qf = _mixed_query_filter(rng, nq, len(filters))
    cuda = torch.device("cuda", dev.device)
    tq, tt = torch.from_numpy(Q).to(cuda), torch.from_numpy(table).to(cuda)
    stream = torch.cuda.Stream(cuda)

    def run(qf_values, graph):
        tf = torch.from_numpy(np.ascontiguousarray(qf_values, np.int32)).to(cuda)
        td = torch.empty((nq, K), dtype=torch.float32, device=cuda)
        tl = torch.empty((nq, K), dtype=torch.int32, device=cuda)
        tc = torch.empty(nq, dtype=torch.int32, device=cuda)
        tnd = torch.zeros(nq, dtype=torch.int64, device=cuda)
        tnh = torch.zeros(nq, dtype=torch.int64, device=cuda)
        torch.cuda.synchronize(cuda)
        with torch.cuda.stream(stream):
            if graph:
                dev.search_device_filtered_grouped(tq.data_ptr(), nq, K, 64, 100, tt.data_ptr(), len(filters), table.shape[1], n_bits,
                                                   tf.data_ptr(), td.data_ptr(), tl.data_ptr(), tc.data_ptr(), tnd.data_ptr(),
                                                   tnh.data_ptr(), stream=stream.cuda_stream)
            else:
                dev.search_device_exhaustive_grouped(tq.data_ptr(), nq, K, tt.data_ptr(), len(filters), table.shape[1], n_bits,
                                                     tf.data_ptr(), td.data_ptr(), tl.data_ptr(), tc.data_ptr(), tnd.data_ptr(),
                                                     stream=stream.cuda_stream)
        stream.synchronize()
        dev.status()
        return td.cpu().numpy(), tl.cpu().numpy(), {"count": tc.cpu().numpy(), "n_dist": tnd.cpu().numpy(), "n_hops": tnh.cpu().numpy()}

    host = {True: dev.search_filtered_grouped(Q, K, 64, filters, qf, stats=True),
            False: dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)}
    bad = qf.copy()
    bad[[3, 50]] = len(filters)  # out of range on either side: the empty filter for those queries, the others untouched
    bad[[7, 99]] = -7
    is_bad = np.isin(np.arange(nq), [3, 50, 7, 99])
    for graph in (True, False):
        keys = GRAPH_KEYS if graph else SCAN_KEYS
        _rows_equal(run(qf, graph), np.arange(nq), host[graph], keys, ("device entry point", graph))
        got = run(bad, graph)
        _rows_equal(got, np.flatnonzero(~is_bad), tuple(x[~is_bad] if not isinstance(x, dict) else {k: v[~is_bad] for k, v in x.items()}
                                                      for x in host[graph]), keys, ("other rows", graph))
        assert np.isposinf(got[0][is_bad]).all() and (got[1][is_bad] == -1).all() and (got[2]["count"][is_bad] == 0).all()
        with pytest.raises(ValueError):
            (dev.search_filtered_grouped(Q, K, 64, filters, bad) if graph else dev.search_exhaustive_grouped(Q, K, filters, bad))
    # ... and the C ABI's host entry points themselves refuse them, naming the first offender
    L = hip.lib()
    d, l = np.empty((nq, K), np.float32), np.empty((nq, K), np.int32)
    rc = L.fnv_search_batch_exhaustive_grouped(dev._h, Q.ctypes.data, nq, K, table.ctypes.data, len(filters), table.shape[1], n_bits,
                                               bad.ctypes.data, d.ctypes.data, l.ctypes.data, None, None)
    assert rc == hip.FNV_ERR_INVALID and b"query_filter[3] = 3" in L.fnv_last_error()
    rc = L.fnv_search_batch_filtered_grouped(dev._h, Q.ctypes.data, nq, K, 64, 100, table.ctypes.data, len(filters), table.shape[1],
                                             n_bits, bad.ctypes.data, d.ctypes.data, l.ctypes.data, None, None, None)
    assert rc == hip.FNV_ERR_INVALID and b"query_filter[3] = 3" in L.fnv_last_error()


# ---- 7. concurrency -----------------------------------------------------------------------------------------------------------------
def test_grouped_and_plain_callers_on_one_handle(oracle_mod):
    rng = np.random.default_rng(71)
    n = 4000
    X, Q = _int_data(rng, n, 256, 32, "float32", "l2")
    _, dev = _pair(oracle_mod, "l2", "float32", X, efc=32)
    filters = [np.arange(0, n, 2), rng.choice(n, n // 20, replace=False), np.arange(100, 400)]
    qf = _mixed_query_filter(rng, len(Q), len(filters))
    calls = [lambda: dev.search_filtered_grouped(Q, 10, 64, filters, qf, stats=True),
             lambda: dev.search_exhaustive_grouped(Q, 10, filters, qf, stats=True),
             lambda: dev.search(Q, 10, 64, stats=True)]
    want = [c() for c in calls]
    errors = []

    def worker(i):
        try:
            for _ in range(6):
                got = calls[i]()
                _rows_equal(got, np.arange(len(Q)), want[i], tuple(want[i][2]), i)
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(calls))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []


def test_grouped_launches_take_no_sample_of_the_adaptive_choice(oracle_mod):
    # 2048 queries: the smallest batch the adaptive choice samples on.  A plain search starts the sampling (its launch is an
    # exploratory one, its time is pending); grouped launches in between are neither samples nor exploratory, and the next plain
    # search is still one -- nothing was settled on their account.
    rng = np.random.default_rng(72)
    n, nq = 8000, 2048
    X, Q = ds.sift_like(n, nq)
    _, dev = _pair(oracle_mod, "l2", "float32", X, efc=48)
    dev.set_option("sorted_beam", 2)
    filters = [rng.choice(n, n // 2, replace=False), rng.choice(n, n // 20, replace=False)]
    qf = _mixed_query_filter(rng, nq, len(filters))
    dev.search(Q, 10, 64)
    assert dev.launch_info()["exploratory"], dev.launch_info()
    explored = hip.lane_exploratory_launches(dev)[0]
    assert explored == 1
    dev.search_filtered_grouped(Q, 10, 64, filters, qf)
    assert not dev.launch_info()["exploratory"] and dev.launch_info()["variant"] == "two_heaps", dev.launch_info()
    dev.search_exhaustive_grouped(Q, 10, filters, qf)
    assert dev.launch_geometry()["kernel"] == "exhaustive_scan"
    assert hip.lane_exploratory_launches(dev)[0] == explored
    dev.search(Q, 10, 64)
    assert dev.launch_info()["exploratory"] and hip.lane_exploratory_launches(dev)[0] == explored + 1, dev.launch_info()


# ---- 8. the _core surface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_core_module_entry_points(flatnav, dtype):
    rng = np.random.default_rng(81)
    n, dim = 2000, 32
    X, Q = _int_data(rng, n, 30, dim, dtype, "l2")
    np_t = np.float32 if dtype == "float32" else np.uint8
    index = flatnav.index.create("l2", dim, n, 16, index_data_type=getattr(flatnav.data_type.DataType, dtype))
    index.set_num_threads(1)
    index.add(X.astype(np_t), 32)
    filters = [rng.choice(n, n // 4, replace=False), np.arange(10), np.zeros(0, np.int64)]
    mask = np.zeros((3, n), bool)
    for f, one in enumerate(filters):
        mask[f, one] = True
    qf = _mixed_query_filter(rng, len(Q), 3)
    dev = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)
    for table in (filters, mask):
        d, l = index.search_filtered_grouped(Q, 10, 64, table, qf)
        wd, wl = dev.search_filtered_grouped(Q, 10, 64, table, qf)
        assert np.array_equal(l, wl) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))
        d, l = index.search_exhaustive_grouped(Q, 10, table, qf)
        wd, wl = dev.search_exhaustive_grouped(Q, 10, table, qf)
        assert np.array_equal(l, wl) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))
    for bad_qf in (np.full(len(Q), 3), np.full(len(Q), -2), qf[:5]):
        with pytest.raises(ValueError):
            index.search_exhaustive_grouped(Q, 10, filters, bad_qf)
        with pytest.raises(ValueError):
            index.search_filtered_grouped(Q, 10, 64, filters, bad_qf)
    for bad_k in (0, 1025):
        with pytest.raises(ValueError):
            index.search_exhaustive_grouped(Q, bad_k, filters, qf)
    with pytest.raises(ValueError):
        index.search_filtered_grouped(Q[:, :5], 10, 64, filters, qf)
    with pytest.raises(ValueError):
        index.search_exhaustive_grouped(Q, 10, [np.array([1, -2])], qf)
