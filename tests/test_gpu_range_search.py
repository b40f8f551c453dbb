"""Range search on the GPU (option "scan_radius"; csrc/scan.hpp "Range search" and the three matrix engines) against numpy,
exactly.  600 rows of integer values below 60: every float32 distance is exact, so in range = float32(d) <= float32(r), the row =
lexsort((node id, d)) of the in-range candidates cut at K and padded, count = min(K, in range), n_dist = in range."""
import ctypes

import numpy as np
import pytest

from flatnav_amd import datasets as ds
from flatnav_amd import hip
from test_gpu_exhaustive import _build, _dist64, _same_results

pytestmark = pytest.mark.gpu
N, NQ = 600, 33
ENGINE = {"uint8": ("scan_matrix", "exhaustive_scan_matrix"), "int8": ("scan_matrix", "exhaustive_scan_matrix"),
          "float16": ("scan_matrix_float", "exhaustive_scan_matrix_float"), "float32": ("scan_matrix_float32", "exhaustive_scan_matrix_float32")}


def _bits(r):
    return int(np.array([r], np.float32).view(np.uint32)[0])


def _expected(D, cands, labels, K, r):
    """The contract from exact float64 distances D[nq][n], each query's ascending candidate node ids and the radius."""
    d, l = np.full((len(D), K), np.inf, np.float32), np.full((len(D), K), -1, np.int32)
    count, total = np.zeros(len(D), np.int32), np.zeros(len(D), np.uint64)
    for q, cand in enumerate(cands):
        dq = D[q, cand].astype(np.float32)
        ids, dq = cand[dq <= np.float32(r)], dq[dq <= np.float32(r)]
        order = np.lexsort((ids, dq))[:K]
        d[q, :len(order)], l[q, :len(order)], count[q], total[q] = dq[order], labels[ids[order]], len(order), len(ids)
    return d, l, count, total


def _check(got, want, what):
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(got[2]["count"], want[2]) and np.array_equal(got[2]["n_dist"].astype(np.uint64), want[3]), what


@pytest.mark.parametrize("metric", ["l2", "ip"])
# inside the matrix engines' register span and beyond it; a float32 split row
@pytest.mark.parametrize("dtype,dim", [("uint8", 128), ("uint8", 200), ("int8", 128), ("int8", 200), ("float16", 128), ("float16", 200),
                                       ("float32", 128), ("float32", 200), ("float32", 100)])
def test_against_numpy(oracle_mod, dtype, dim, metric):
    rng = np.random.default_rng(dim + len(dtype) + len(metric))
    X, Q = rng.integers(0, 60, (N, dim)).astype(dtype), rng.integers(0, 60, (NQ, dim)).astype(dtype)
    X[100:120] = X[99]  # twenty-one rows attain one distance
    X, labels, dev = _build(oracle_mod, metric, dtype, X, (rng.permutation(N) + 3).astype(np.int32), M=8, efc=16)
    D = _dist64(X, Q, metric)
    filters = [rng.choice(N, N // 2, replace=False) + 3, np.arange(3, 203), np.zeros(0, np.int64)]  # about half; a third; empty
    cand_of = [np.flatnonzero(np.isin(labels, f)) for f in filters] + [np.arange(N)]  # ([-1]: no filter)
    qf = rng.integers(-1, 3, NQ).astype(np.int32)
    qf[:4] = [-1, 0, 1, 2]
    calls = {"all": (lambda Q, K: dev.search_exhaustive(Q, K, stats=True), [cand_of[-1]] * NQ),
             "half": (lambda Q, K: dev.search_exhaustive(Q, K, allowed=filters[0], stats=True), [cand_of[0]] * NQ),
             "grouped": (lambda Q, K: dev.search_exhaustive_grouped(Q, K, filters, qf[:len(Q)], stats=True), [cand_of[f] for f in qf])}
    option, matrix_kernel = ENGINE[dtype]
    dev.set_option("scan_segment_rows", 64)
    before, geom_before = calls["all"][0](Q, 10), dev.launch_geometry()  # (the radius was never set)
    truncated = 0
    for name, (call, cands) in calls.items():
        Dc = D[:, cands[0]]
        values, counts = np.unique(Dc[0], return_counts=True)
        # below the smallest distance; one that many rows attain; the median (more than ten rows); above the largest; +inf
        radii = [Dc.min() - 1.0, float(values[counts.argmax()]), float(np.median(Dc)), D.max() + 1.0, np.inf]
        assert counts.max() >= 3
        for K, nq, seg in ((1, NQ, 64), (10, NQ, 64), (700, NQ, 64), (10, 1, 64), (10, NQ, 0)):  # (0: one segment on 600 rows)
            dev.set_option("scan_segment_rows", seg)
            dev.set_option("scan_radius", -1)
            off = call(Q[:nq], K)
            for r in radii:
                want = _expected(D[:nq], cands[:nq], labels, K, r)
                truncated += int((want[3] > want[2].astype(np.uint64)).sum())
                dev.set_option("scan_radius", _bits(r))
                for engine in (0, 1):
                    dev.set_option(option, engine)
                    dev.set_option("scan_matrix_grouped", engine)
                    got, geom, what = call(Q[:nq], K), dev.launch_geometry(), (dtype, dim, metric, name, K, nq, seg, r, engine)
                    assert geom["kernel"] == (matrix_kernel if engine and K <= 10 else "exhaustive_scan") and geom["range"] == 1, what
                    _check(got, want, what)
                    if r > D.max():  # every candidate is in range: the radius-off row, n_dist = the candidate count
                        _same_results(got, off, what)
                        assert np.array_equal(got[2]["n_dist"], [len(c) for c in cands[:nq]]), what
                dev.set_option(option, 0)
                dev.set_option("scan_matrix_grouped", 0)
    assert truncated > 0
    dev.set_option("scan_segment_rows", 64)
    dev.set_option("scan_radius", -1)
    _same_results(calls["all"][0](Q, 10), before, "radius off again")
    assert dev.launch_geometry() == geom_before and geom_before["range"] == 0
    if dtype == "float32" and dim == 128:  # a routed filtered graph search: its scan stage ignores the radius
        dev.set_option("filter_scan_max", 300)
        unset = dev.search_filtered(Q, 10, 64, filters[1], stats=True)
        dev.set_option("scan_radius", _bits(D.min() - 1.0))
        assert (unset[2]["count"] == 10).all() and (unset[2]["n_hops"] == 0).all()
        _same_results(dev.search_filtered(Q, 10, 64, filters[1], stats=True), unset, "routed")


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_real_values_with_a_nan_and_an_inf_row(oracle_mod, dtype, metric):
    """The engine writes the vector scan's bytes under the same radius, and both equal the radius-off call at K = n (the behaviour
    before there was a radius) cut at d <= r.  The NaN row is within no radius."""
    n, dim = N, 128
    X, Q = (a.astype(dtype) for a in ds.randn(n, NQ, dim, seed=7, normalize=metric == "ip"))
    o = oracle_mod.OracleIndex.create(metric, dim, n, 8, "float32")
    o.add(X.astype(np.float32), 16)  # (the graph is built on finite rows, in row order)
    X[80, 5], X[81, 7] = np.nan, np.inf
    nodes = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)
    blob = np.concatenate([X.view(np.uint8).reshape(n, X.itemsize * dim), nodes[:, o.data_size:]], axis=1)
    dev = hip.DeviceIndex.upload(blob.reshape(-1), blob.shape[1], X.itemsize * dim, o.M, n, dtype, metric, dim)
    dev.set_option("scan_segment_rows", 64)
    d0, l0, _ = dev.search_exhaustive(Q, n, stats=True)
    assert (l0[:, -1] == 80).all() and np.isnan(d0[:, -1]).all()
    for r in (float(np.median(d0[:, 1:n - 2])), float(d0[0, 20]), np.inf):
        with np.errstate(invalid="ignore"):
            keep = d0 <= np.float32(r)
        want = (np.where(keep, d0, np.float32(np.inf)), np.where(keep, l0, -1), keep.sum(1).astype(np.int32), keep.sum(1).astype(np.uint64))
        dev.set_option("scan_radius", _bits(r))
        for engine in (0, 1):
            dev.set_option(ENGINE[dtype][0], engine)
            got = dev.search_exhaustive(Q, n, stats=True)
            assert dev.launch_geometry()["kernel"] == ("exhaustive_scan", ENGINE[dtype][1])[engine]
            _check(got, want, (dtype, metric, r, engine))
            assert not (got[1] == 80).any() and (r != np.inf or (got[2]["count"] == n - 1).all())


def test_python_index_round_trip():  # set_exhaustive_radius reaches the mirror; None gives back the bytes from before it was set
    import flatnav_amd

    rng = np.random.default_rng(3)
    X, Q = rng.integers(0, 60, (N, 64)).astype(np.float32), rng.integers(0, 60, (NQ, 64)).astype(np.float32)
    index = flatnav_amd.index.create("l2", 64, N, 8)
    index.add(X, 16, labels=list(range(N)))
    ranges = []
    for r in (None, float(np.median(index.search_exhaustive(Q, 10)[0][:, 4])), None):
        index.set_exhaustive_radius(r)
        d, l = index.search_exhaustive(Q, 10)
        ranges.append(hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False).launch_geometry()["range"])
        if r is None:
            d0, l0 = (d, l) if len(ranges) == 1 else (d0, l0)
            assert np.array_equal(l, l0) and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
        else:
            keep = d0 <= np.float32(r)
            assert not keep.all() and np.array_equal(l, np.where(keep, l0, -1)) and np.array_equal(d, np.where(keep, d0, np.float32(np.inf)))
    assert ranges == [0, 1, 0]
