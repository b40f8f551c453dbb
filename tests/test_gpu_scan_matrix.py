"""The exhaustive search's matrix engine on the GPU (option "scan_matrix", csrc/scan_matrix.hpp): on uint8 / int8 indexes it writes
exactly what the contract says and exactly what the vector scan writes.  The reference is numpy: int64 dot products over the
rows in node order, the distance formed as the contract forms it -- float32(s) for L2, float32(1) - float32(s) for inner
product -- ordered by lexsort((node id, that float32)).  Data is full-range: at 3072-d sums pass 2^24, distinct integers round to
one float and the node id decides."""
import ctypes

import numpy as np
import pytest

import test_scan_matrix_plan as plan
from flatnav_amd import hip
from test_gpu_exhaustive import _build, _equal, _same_results

pytestmark = pytest.mark.gpu


def _data(rng, n, nq, dim, dtype):
    lo, hi = (0, 256) if dtype == "uint8" else (-128, 128)
    return rng.integers(lo, hi, (n, dim)).astype(dtype), rng.integers(lo, hi, (nq, dim)).astype(dtype)


def _dist(X, Q, metric):
    X, Q = X.astype(np.int64), Q.astype(np.int64)
    if metric == "l2":
        return ((Q * Q).sum(1)[:, None] + (X * X).sum(1)[None, :] - 2 * (Q @ X.T)).astype(np.float32)
    return np.float32(1) - (Q @ X.T).astype(np.float32)


def _topk(D, nodes, labels, K):
    nq, m, k = D.shape[0], len(nodes), min(K, len(nodes))
    d, l = np.full((nq, K), np.inf, np.float32), np.full((nq, K), -1, np.int32)
    order = np.lexsort((np.broadcast_to(nodes, (nq, m)), D[:, nodes]), axis=1)[:, :k]
    d[:, :k], l[:, :k] = np.take_along_axis(D[:, nodes], order, 1), labels[nodes[order]]
    return d, l, np.full(nq, k, np.int32), np.full(nq, m, np.uint64)


def _both_engines(dev, Q, K, want, what, allowed=None, matrix_mode=4):
    """The call with the engine on (against numpy, and launched as `matrix_mode`) and off (the same bytes, kernel 3)."""
    dev.set_option("scan_matrix", 1)
    on = dev.search_exhaustive(Q, K, allowed=allowed, stats=True)
    assert dev.launch_geometry()["kernel_mode"] == matrix_mode, (what, dev.launch_geometry())
    dev.set_option("scan_matrix", 0)
    off = dev.search_exhaustive(Q, K, allowed=allowed, stats=True)
    assert dev.launch_geometry()["kernel_mode"] == 3, what
    _equal(on, want, what)
    _same_results(on, off, what)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["uint8", "int8"])
@pytest.mark.parametrize("dim", [1, 16, 33, 100, 400, 3072])  # a sub-chunk row, one chunk, odd chunk count, padded, split, several spans
def test_geometry(oracle_mod, dtype, metric, dim):
    rng = np.random.default_rng(dim * 7 + len(dtype) + len(metric))
    n = 1500
    X, Q = _data(rng, n, 48, dim, dtype)
    labels = (rng.permutation(n) + 3).astype(np.int32)  # labels are not node ids
    X, labels, dev = _build(oracle_mod, metric, dtype, X, labels, M=8, efc=16)
    allowed = rng.choice(n, n // 10, replace=False) + 3
    nodes_f, D = np.flatnonzero(np.isin(labels, allowed)), _dist(X, Q, metric)
    for K in (1, 10, 100):
        want_all, want_f = _topk(D, np.arange(n), labels, K), _topk(D, nodes_f, labels, K)
        for seg in (0, 256):  # automatic, and many segments with a real merge
            dev.set_option("scan_segment_rows", seg)
            _both_engines(dev, Q, K, want_all, (dtype, metric, dim, K, seg, "all"))
            _both_engines(dev, Q, K, want_f, (dtype, metric, dim, K, seg, "10 %"), allowed=allowed)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_edges_of_tiles_and_of_k(oracle_mod, n):
    rng = np.random.default_rng(200 + n)
    X, Qall = _data(rng, n, 257, 32, "uint8")
    X, labels, dev = _build(oracle_mod, "l2", "uint8", X, (rng.permutation(n) + 3).astype(np.int32), M=8, efc=16)
    modes = set()
    for nq in (1, 31, 33, 257):
        D = _dist(X, Qall[:nq], "l2")
        for K in sorted({1, n, n + 5, 1024}):
            mode = 4 if plan.shape(plan.U8, 32, nq, K, n)["on"] else 3  # (K = 1024: 32 lists do not fit a block's LDS)
            _both_engines(dev, Qall[:nq], K, _topk(D, np.arange(n), labels, K), (n, nq, K), matrix_mode=mode)
            modes.add(mode)
    assert modes == {3, 4}


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_value_edges(oracle_mod, dtype, metric):
    rng = np.random.default_rng(len(dtype) * 3 + len(metric))
    lo, hi = (0, 255) if dtype == "uint8" else (-128, 127)
    X, Q = _data(rng, 300, 34, 3072, dtype)
    X[:40], X[40:80], Q[0], Q[1] = hi, lo, lo, hi  # constant rows and queries at both ends of the type: the largest sums
    X, labels, dev = _build(oracle_mod, metric, dtype, X, None, M=8, efc=16)
    _both_engines(dev, Q, 10, _topk(_dist(X, Q, metric), np.arange(300), labels, 10), (dtype, metric))


@pytest.mark.parametrize("dtype", ["float32", "float16", "uint8"])
def test_not_applicable_is_not_invalid(oracle_mod, dtype):
    """Float indexes, and the grouped call on a uint8 index, run the vector scan with the option on: the same bytes, kernel 3."""
    rng = np.random.default_rng(5)
    X, Q = rng.integers(0, 60, (500, 40)).astype(dtype), rng.integers(0, 60, (33, 40)).astype(dtype)
    _, _, dev = _build(oracle_mod, "l2", dtype, X, None, M=8, efc=16)
    filters, qf = [rng.choice(500, 50, replace=False), np.arange(100, 130)], rng.integers(-1, 2, 33).astype(np.int32)
    grouped = lambda: dev.search_exhaustive_grouped(Q, 10, filters, qf, stats=True)  # noqa: E731
    call = grouped if dtype == "uint8" else lambda: dev.search_exhaustive(Q, 10, stats=True)
    off = call()
    dev.set_option("scan_matrix", 1)
    on = call()
    assert dev.launch_geometry()["kernel_mode"] == 3
    _same_results(on, off, dtype)


def test_python_index_round_trip():  # set before the device mirror exists: reaches the mirror made later; toggled: the one there is
    import flatnav_amd

    classes = [c for c in vars(flatnav_amd._core.index).values() if isinstance(c, type) and hasattr(c, "search_exhaustive")]
    assert len(classes) == 8 and all(callable(getattr(c, "set_exhaustive_matrix", None)) for c in classes)
    X, Q = _data(np.random.default_rng(9), 600, 40, 64, "uint8")
    index = flatnav_amd.index.create("l2", 64, 600, 8, flatnav_amd.data_type.DataType.uint8)
    index.add(X, 16, labels=list(range(600)))
    got = []
    for on, mode in ((True, 4), (False, 3), (True, 4)):  # (the first: no mirror yet)
        index.set_exhaustive_matrix(on)
        got.append(index.search_exhaustive(Q, 10))
        geom = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False).launch_geometry()
        assert geom["kernel_mode"] == mode, (on, geom)
    for d, l in got[1:]:
        assert np.array_equal(l, got[0][1]) and np.array_equal(d.view(np.uint32), got[0][0].view(np.uint32))
