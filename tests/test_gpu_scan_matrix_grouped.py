"""The matrix engines' grouped form on the GPU (option "scan_matrix_grouped", csrc/scan_matrix_feed.hpp): a grouped exhaustive
call whose rows come from each filter row's bitmap writes the numpy reference's results on integer-valued data (every sum exact,
ties decided by node id), the grouped vector scan's bytes, and per query the single-filter call's bytes under the same engine."""
import numpy as np
import pytest

from flatnav_amd import datasets as ds
from flatnav_amd import hip
from test_gpu_exhaustive import _build, _dist64, _equal, _same_results, _topk
from test_gpu_filtered import _int_data
from test_gpu_grouped_filters import SCAN_KEYS, _rows_equal

pytestmark = pytest.mark.gpu
ENGINE = {"uint8": ("scan_matrix", 4), "int8": ("scan_matrix", 4), "float16": ("scan_matrix_float", 5), "float32": ("scan_matrix_float32", 6)}
# one row length inside the engine's register span and one beyond it; float32 also a split row (24 chunks and a tail of one)
DIMS = [(t, d) for t in ("uint8", "int8") for d in (40, 200)] + [("float16", 40), ("float16", 136), ("float32", 40), ("float32", 136), ("float32", 97)]
N = 2203  # 69 bitmap words: a second, short 64-word step; the "all" filter's first step holds 2048 ids, eight times the queue
ALLOWED = (0, 1, 31, 32, 33, 65, N)  # nodes per filter; the last filter of a call (100 nodes) has no query
QUERIES = (1, 1, 1, 1, 31, 33, 129)  # queries per filter: 129 on the full row = two tiles of 128; 33 more with no filter (-1)


def _grouped(dev, dtype, on, *call):
    """The grouped call with the element type's engine on and "scan_matrix_grouped" = `on`; the kernel that ran is the expected one."""
    option, mode = ENGINE[dtype]
    dev.set_option(option, 1)
    dev.set_option("scan_matrix_grouped", int(on))
    got = dev.search_exhaustive_grouped(*call, stats=True)
    geom = dev.launch_geometry()
    assert geom["kernel_mode"] == (mode if on else 3) and geom["queue_ids"] == 256 and geom["tile_queries"] % (32 if on else 1) == 0, geom
    return got


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype, dim", DIMS)
def test_grouped_equals_reference_vector_scan_and_single_calls(oracle_mod, dtype, dim, metric):
    rng = np.random.default_rng(dim + len(dtype) + len(metric))
    X, Q = _int_data(rng, N, sum(QUERIES) + 33, dim, dtype, metric)
    X[N // 2:N // 2 + 1000] = X[:1000]  # exact duplicates: the node id decides
    labels = (rng.permutation(N) + 3).astype(np.int32)
    twins = lambda c: np.concatenate([h := rng.choice(1000, (c + 1) // 2, replace=False), h + N // 2])[:c]  # noqa: E731  (rows of every segment)
    filters = [labels[twins(c)] if c < N else labels.copy() for c in ALLOWED] + [labels[500:600]]
    qf = rng.permutation(np.repeat(np.arange(-1, len(ALLOWED)), (33,) + QUERIES)).astype(np.int32)
    X, labels, dev = _build(oracle_mod, metric, dtype, X, labels, M=8, efc=16)
    D = _dist64(X, Q, metric)
    nodes_of = {g: np.flatnonzero(np.isin(labels, filters[g])) if g >= 0 else np.arange(N) for g in range(-1, len(ALLOWED))}
    for seg in (4096, 250):  # one segment; nine, whose ends (words 7, 15, 23, ...) fall inside the 64-word steps
        dev.set_option("scan_segment_rows", seg)
        for K in (1, 10, 100):  # (100: more than six of the filters allow -- padding and count)
            on, off = _grouped(dev, dtype, True, Q, K, filters, qf), _grouped(dev, dtype, False, Q, K, filters, qf)
            _same_results(on, off, (dtype, metric, dim, K, seg, "vector scan"))
            for g, nodes in nodes_of.items():
                rows = np.flatnonzero(qf == g)
                sub = (on[0][rows], on[1][rows], {k: on[2][k][rows] for k in SCAN_KEYS})
                _equal(sub, _topk(D[rows][:, nodes], nodes, labels, K), (dtype, metric, dim, K, seg, g, "numpy"))
                single = dev.search_exhaustive(Q[rows], K, allowed=None if g < 0 else filters[g], stats=True)
                assert dev.launch_geometry()["kernel_mode"] == ENGINE[dtype][1]
                _rows_equal(on, rows, single, SCAN_KEYS, (dtype, metric, dim, K, seg, g, "single"))


def test_random_float_rows_with_a_nan_and_an_inf(oracle_mod):
    """Real-valued float32 rows: the prefilter passes a share of the pairs on, rescoring gives them the vector scan's bits."""
    n, dim = 1500, 136
    X, Q = ds.randn(n, 70, dim, seed=3)
    o = oracle_mod.OracleIndex.create("l2", dim, n, 8, "float32")
    o.add(X, 16)  # (the graph is built on finite rows, in row order; the scan never reads it)
    X[80, 5], X[81, 7] = np.nan, np.inf
    nodes = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)
    blob = np.concatenate([X.view(np.uint8).reshape(n, 4 * dim), nodes[:, o.data_size:]], axis=1)
    dev = hip.DeviceIndex.upload(blob.reshape(-1), blob.shape[1], 4 * dim, o.M, n, "float32", "l2", dim)
    filters, qf = [np.arange(60, 111), np.arange(0, n, 2)], np.repeat([0, 1, -1], (3, 34, 33)).astype(np.int32)
    for K in (10, 200):
        on, off = _grouped(dev, "float32", True, Q, K, filters, qf), _grouped(dev, "float32", False, Q, K, filters, qf)
        assert dev.scan_rescored() == {"scored": 0, "rescored": 0}  # (the vector scan ran last)
        _same_results(on, off, K)
    assert (on[1][:3, 50] == 80).all() and np.isnan(on[0][:3, 50]).all() and (on[1][:3, 49] == 81).all() and (on[1][:3, 51:] == -1).all()
    _grouped(dev, "float32", True, Q, 10, filters, qf)
    r = dev.scan_rescored()
    assert r["scored"] == 3 * 51 + 34 * (n // 2) + 33 * n and 0 < r["rescored"] < r["scored"], r


def test_a_k_beyond_the_lds_keeps_the_vector_scan(oracle_mod):
    rng = np.random.default_rng(7)
    X, Q = _int_data(rng, 300, 40, 40, "uint8", "l2")
    _, _, dev = _build(oracle_mod, "l2", "uint8", X, None, M=8, efc=16)
    filters, qf = [np.arange(100), np.arange(50, 300)], rng.integers(-1, 2, 40).astype(np.int32)
    for K in (100, 1024):  # 32 lists of 1024 keys: 256 KB
        dev.set_option("scan_matrix", 1)
        dev.set_option("scan_matrix_grouped", 1)
        on = dev.search_exhaustive_grouped(Q, K, filters, qf, stats=True)
        assert dev.launch_geometry()["kernel_mode"] == (4 if K == 100 else 3)
        _same_results(on, _grouped(dev, "uint8", False, Q, K, filters, qf), K)
