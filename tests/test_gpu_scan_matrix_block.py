"""The block form of the float matrix engines on the GPU (option "scan_matrix_block", csrc/scan_matrix_block.hpp): workgroups whose
wavefronts share every row tile write exactly what the vector scan writes -- labels, distance bits, padding, counts, n_dist -- and
both sit within the float bar of numpy float64.  A wavefront scoring another's queries, a ring buffer read too early or too late,
a norm from the wrong row or a span left out shows as a difference between the engines."""
import ctypes
import functools

import numpy as np
import pytest

import row_classes as rc
import test_gpu_scan_matrix_f16 as f16
import test_gpu_scan_matrix_f32 as f32
from distance_model import dist64
from flatnav_amd import datasets as ds
from flatnav_amd import hip

pytestmark = pytest.mark.gpu
ENGINE = {"float16": (f16._both_engines, 5), "float32": (f32._both_engines, 6)}  # (against the vector scan, the wave engine's mode)
# Rows the block form takes (at most 8 MFMA steps): a sub-chunk row, seven steps, exactly eight, a float32 split row with a
# side-table tail -- and one longer row per element type (13 and 17 steps), which the planner declines.
SHORT = [("float16", 1), ("float16", 100), ("float16", 128), ("float32", 1), ("float32", rc.dim_of("float32", "8x3-tail1")), ("float32", 128)]
LONG = [("float16", 200), ("float32", rc.dim_of("float32", "32x4-clamped"))]
N = 1500


def _check(dev, dtype, block, D, labels, Q, K, seg, what, allowed=None):
    """The call against the vector scan and float64; `block`: it must have run as the block form (kernel 7 / 8), else as the wave
    engine (5 / 6) -- the block form takes one filter, more than 32 queries, rows of at most 8 steps."""
    both, wave_mode = ENGINE[dtype]
    dev.set_option("scan_segment_rows", seg)
    return both(dev, D, labels, Q, K, what, allowed=allowed, mode=wave_mode + 2 if block else wave_mode)


def _upload(oracle_mod, metric, X, labels, rows=None):
    """A device index of `rows` (default X) in row order, with the option on.  The graph is built on X by ONE host thread, so node
    i is row i; the scan never reads it."""
    n, dim = X.shape
    rows = X if rows is None else rows
    o = oracle_mod.OracleIndex.create(metric, dim, n, 8, "float32")
    o.add(X.astype(np.float32), 16, labels=labels)
    nodes = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)
    blob = np.concatenate([rows.view(np.uint8).reshape(n, rows.itemsize * dim), nodes[:, o.data_size:]], axis=1)
    dev = hip.DeviceIndex.upload(blob.reshape(-1), blob.shape[1], rows.itemsize * dim, o.M, n, str(rows.dtype), metric, dim)
    dev.set_option("scan_matrix_block", 1)
    return dev


@functools.lru_cache(maxsize=2)
def _index(oracle_mod, dtype, metric, dim):
    rng = np.random.default_rng(dim * 7 + len(metric))
    X, Q = (a.astype(dtype) for a in ds.randn(N, 257, dim, seed=dim, normalize=metric == "ip"))
    labels = (rng.permutation(N) + 3).astype(np.int32)
    return _upload(oracle_mod, metric, X, labels), labels, Q, dist64(X, Q, metric), rng.choice(N, N // 10, replace=False) + 3


# two wavefronts, the second with one query; two full; four with the last nearly empty; more than one sub-tile per wavefront;
# several tiles with a ragged last one -- and one sub-tile or less: the planner declines
@pytest.mark.parametrize("nq", [33, 64, 97, 129, 257, 1, 32])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype,dim", SHORT + LONG)
def test_geometry(oracle_mod, dtype, dim, metric, nq):
    dev, labels, Q, D, allowed = _index(oracle_mod, dtype, metric, dim)
    for K in (1, 10, 100):
        for seg in (0, 256):  # automatic, and many segments with a real merge
            _check(dev, dtype, False, D[:nq], labels, Q[:nq], K, seg, (dtype, metric, dim, nq, K, seg, "all"))  # unfiltered: declined
            _check(dev, dtype, nq > 32 and (dtype, dim) in SHORT, D[:nq], labels, Q[:nq], K, seg, (dtype, metric, dim, nq, K, seg, "10 %"),
                   allowed=allowed)


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_adversarial_values(oracle_mod, dtype, metric):
    """Duplicates (the node id decides), rows one step of the element type from a query, bfloat16 / binary16 rounding ties, a NaN
    and a +inf row; n no multiple of 32, seven-step rows (float32: with a side-table tail), segments shorter than one row tile."""
    n, dim, nq = 403, 100, 70
    X, Q = (a.astype(dtype) for a in ds.randn(n, nq, dim, seed=3, normalize=metric == "ip"))
    X[10:50] = X[9]
    X[100], X[101], X[102], X[103] = Q[0], Q[0], Q[33], Q[33]
    X[101, 70], X[103, 99] = np.nextafter(X[101, 70], X.dtype.type(np.inf)), np.nextafter(X[103, 99], X.dtype.type(-np.inf))
    tie = lambda a: (a.astype(np.float32).view(np.uint32) & 0xFFFF0000 | 0x8000).view(np.float32)  # noqa: E731  halfway between two bfloat16
    X[106], X[107], Q[65] = tie(X[106]).astype(dtype), tie(Q[64]).astype(dtype), tie(Q[65]).astype(dtype)  # (float16: 2^-8 relative steps, exact)
    labels, finite = np.arange(n, dtype=np.int32), X.copy()  # (the graph is built on finite rows)
    X[80, 5], X[81, 7] = np.nan, np.inf
    dev = _upload(oracle_mod, metric, finite, labels, rows=X)
    with np.errstate(invalid="ignore", over="ignore"):
        D = dist64(X, Q, metric)
    most = np.flatnonzero(np.arange(n) % 7 != 0)  # (a filter that keeps every row named above)
    for seg in (0, 20):
        for K in (1, 10, 100):
            _check(dev, dtype, True, D, labels, Q, K, seg, (dtype, metric, K, seg, "6 / 7"), allowed=most)
        d, l, _ = _check(dev, dtype, True, D, labels, Q, 100, seg, (dtype, metric, 100, seg, "edge rows"), allowed=np.arange(60, 111))
        assert (l[:, 50] == 80).all() and np.isnan(d[:, 50]).all() and (l[:, 51:] == -1).all()
        if metric == "l2":
            assert (l[:, 49] == 81).all() and np.isposinf(d[:, 49]).all() and (d[[0, 33], 0] == 0).all() and l[0, 0] == 100 and l[33, 0] == 102


def test_python_index_round_trip():
    import flatnav_amd

    X, Q = (a.astype(np.float16) for a in ds.randn(600, 70, 64, seed=9))
    index = flatnav_amd.index.create("l2", 64, 600, 8, flatnav_amd.data_type.DataType.float16)
    index.add(X, 16, labels=list(range(600)))
    got = []
    for kw, mode, threads in (({"block": True}, 7, 192), ({}, 5, 64), ({"block": True}, 7, 192)):  # (the first: no mirror yet)
        index.set_exhaustive_matrix(True, float_rows=True, **kw)
        got.append(index.search_exhaustive(Q, 10, allowed=list(range(0, 600, 2))))
        geom = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False).launch_geometry()
        assert (geom["kernel_mode"], geom["block_threads"]) == (mode, threads), geom
    for d, l in got[1:]:
        assert np.array_equal(l, got[0][1]) and np.array_equal(d.view(np.uint32), got[0][0].view(np.uint32))
