"""The exhaustive search's float16 matrix engine on the GPU (option "scan_matrix_float", csrc/scan_matrix_f16.hpp): on float16
indexes it writes exactly what the vector scan writes -- labels, distance bits, counts, n_dist -- and both sit within the float
bar (test_gpu_exhaustive.py's RTOL / ATOL) of numpy float64 distances.  A margin too narrow, a wrong accumulator mapping or a
rescoring in another lane order shows as a difference between the engines."""
import ctypes

import numpy as np
import pytest

import test_scan_matrix_f16_plan as plan
from distance_model import dist64
from flatnav_amd import datasets as ds
from flatnav_amd import hip
from test_gpu_exhaustive import ATOL, RTOL, _build, _same_results

pytestmark = pytest.mark.gpu


def _both_engines(dev, D, labels, Q, K, what, allowed=None, mode=5):
    """The call with the engine on (launched as kernel `mode`) and off (kernel 3): the same bytes; every finite reported
    distance within the float bar of D = the float64 distance of its own label (D[query][node]), every returned row among the
    float64 top-K up to that bar."""
    dev.set_option("scan_matrix_float", 1)
    on = dev.search_exhaustive(Q, K, allowed=allowed, stats=True)
    assert dev.launch_geometry()["kernel_mode"] == mode, (what, dev.launch_geometry())
    dev.set_option("scan_matrix_float", 0)
    off = dev.search_exhaustive(Q, K, allowed=allowed, stats=True)
    assert dev.launch_geometry()["kernel_mode"] == 3, what
    _same_results(on, off, what)
    node_of = np.empty(int(labels.max()) + 1, np.int64)
    node_of[labels] = np.arange(len(labels))
    cand = np.arange(len(labels)) if allowed is None else np.flatnonzero(np.isin(labels, allowed))
    k = min(K, len(cand))
    assert (on[2]["count"] == k).all() and (on[2]["n_dist"] == len(cand)).all(), what
    own = np.take_along_axis(D, node_of[on[1][:, :k]], 1)
    kth = np.sort(D[:, cand], axis=1)[:, k - 1:k]  # (NaN sorts last)
    with np.errstate(invalid="ignore"):
        ok = np.abs(on[0][:, :k] - own) <= ATOL + RTOL * np.abs(own)
        among = own <= kth + ATOL + RTOL * np.abs(kth)
    assert ok[np.isfinite(own)].all() and among[np.isfinite(own) & np.isfinite(kth)].all(), what
    return on


@pytest.mark.parametrize("metric", ["l2", "ip"])
# a sub-chunk row, one chunk, two, padded, split rows, several register spans (G = 64); G = 16 and G = 32 (tests/row_classes.py)
@pytest.mark.parametrize("dim", [1, 8, 9, 50, 200, 1536, 300, 600])
def test_geometry(oracle_mod, metric, dim):
    rng = np.random.default_rng(dim * 7 + len(metric))
    n = 1500
    X, Q = (a.astype(np.float16) for a in ds.randn(n, 48, dim, seed=dim, normalize=metric == "ip"))
    X, labels, dev = _build(oracle_mod, metric, "float16", X, (rng.permutation(n) + 3).astype(np.int32), M=8, efc=16)
    allowed, D = rng.choice(n, n // 10, replace=False) + 3, dist64(X, Q, metric)
    for K in (1, 10, 100):
        for seg in (0, 256):  # automatic, and many segments with a real merge
            dev.set_option("scan_segment_rows", seg)
            _both_engines(dev, D, labels, Q, K, (metric, dim, K, seg, "all"))
            _both_engines(dev, D, labels, Q, K, (metric, dim, K, seg, "10 %"), allowed=allowed)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_adversarial_values(oracle_mod, metric):
    """Duplicates (the node id decides), rows one binary16 step from a query, subnormals only, +-65504, queries equal to rows
    (L2 = 0 by cancellation of large norms), and a NaN and a +inf row, which the engine must let through to rank as ever."""
    n, dim = 400, 1536
    X, Q = (a.astype(np.float16) for a in ds.randn(n, 34, dim, seed=3, normalize=metric == "ip"))
    rng = np.random.default_rng(4)
    if metric == "ip":  # non-negative queries: no dot product with a +-65504 row cancels (the bar is relative to |distance|,
        Q = np.abs(Q)   # which no float32 sum meets under cancellation -- the vector scan's neither)
    X[10:50] = X[9]
    X[100], X[101], X[102], X[103] = Q[0], Q[0], Q[1], Q[1]
    X[101, 700], X[103, 1535] = np.nextafter(X[101, 700], np.float16(np.inf)), np.nextafter(X[103, 1535], np.float16(-np.inf))
    X[60:64] = (rng.integers(-1023, 1024, (4, dim)) * 2.0 ** -24).astype(np.float16)
    X[70], X[71] = 65504, -65504
    if metric == "l2":
        X[72] = (65504 * rng.choice([-1.0, 1.0], dim)).astype(np.float16)
        Q[2], Q[3], Q[4] = X[70], X[72], X[61]
    o = oracle_mod.OracleIndex.create(metric, dim, n, 8, "float32")
    o.add(X.astype(np.float32), 16)  # (the graph is built on finite rows, in row order; the node store is narrowed to float16)
    X[80, 5], X[81, 7] = np.nan, np.inf
    nodes = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)
    blob = np.concatenate([X.view(np.uint8).reshape(n, 2 * dim), nodes[:, o.data_size:]], axis=1)
    dev = hip.DeviceIndex.upload(blob.reshape(-1), blob.shape[1], 2 * dim, o.M, n, "float16", metric, dim)
    labels = np.arange(n, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        D = dist64(X, Q, metric)
    for K in (10, 200):
        _both_engines(dev, D, labels, Q, K, (metric, K))
    d, l, st = _both_engines(dev, D, labels, Q, 200, (metric, "edge rows"), allowed=np.arange(60, 111))
    assert (l[:, 50] == 80).all() and np.isnan(d[:, 50]).all() and (l[:, 51:] == -1).all()
    if metric == "l2":
        assert (l[:, 49] == 81).all() and np.isposinf(d[:, 49]).all() and (d[[0, 2], 0] == 0).all() and l[0, 0] == 100 and l[2, 0] == 70


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_edges_of_tiles_and_of_k(oracle_mod, n):
    X, Qall = (a.astype(np.float16) for a in ds.randn(n, 257, 32, seed=n))
    X, labels, dev = _build(oracle_mod, "l2", "float16", X, (np.random.default_rng(n).permutation(n) + 3).astype(np.int32), M=8, efc=16)
    modes = set()
    for nq in (1, 31, 33, 257):
        D = dist64(X, Qall[:nq], "l2")
        for K in sorted({1, n, n + 5, 1024}):
            mode = 5 if plan.shape(plan.F16, 32, nq, K, n)["on"] else 3  # (K = 1024: 32 lists do not fit a block's LDS)
            _both_engines(dev, D, labels, Qall[:nq], K, (n, nq, K), mode=mode)
            modes.add(mode)
    assert modes == {3, 5}


def test_the_prefilter_filters(oracle_mod):
    """Every pair is scored on the matrix cores and few are scored again.  The cap is no performance figure: it fails an engine
    that passes by rescoring everything.  The margin simulated with numpy on this input, 32 rows a step in the launch's three
    segments with the K-th distance taken at the start of a step, lets 14 110 of the 256 000 pairs through: 5.5 % against the
    cap's 25 %."""
    n, nq = 4000, 64
    X, Q = (a.astype(np.float16) for a in ds.randn(n, nq, 128, seed=11))
    X, labels, dev = _build(oracle_mod, "l2", "float16", X, None, M=8, efc=16)
    dev.set_option("scan_segment_rows", 0)
    _both_engines(dev, dist64(X, Q, "l2"), labels, Q, 10, "prefilter")
    assert dev.scan_rescored() == {"scored": 0, "rescored": 0}  # (the vector scan ran last)
    dev.set_option("scan_matrix_float", 1)
    dev.search_exhaustive(Q, 10)
    r = dev.scan_rescored()
    print("float16 matrix engine: %d of %d pairs rescored (%.2f %%)" % (r["rescored"], r["scored"], 100.0 * r["rescored"] / r["scored"]))
    assert r["scored"] == nq * n and 0 < r["rescored"] <= r["scored"] // 4


@pytest.mark.parametrize("dtype", ["float32", "uint8", "float16"])
def test_not_applicable_is_not_invalid(oracle_mod, dtype):
    """Float32 and uint8 indexes, and the grouped call on a float16 index, keep the vector scan with the option on: kernel 3."""
    rng = np.random.default_rng(5)
    X, Q = rng.integers(0, 60, (500, 40)).astype(dtype), rng.integers(0, 60, (33, 40)).astype(dtype)
    _, _, dev = _build(oracle_mod, "l2", dtype, X, None, M=8, efc=16)
    filters, qf = [rng.choice(500, 50, replace=False), np.arange(100, 130)], rng.integers(-1, 2, 33).astype(np.int32)
    grouped = lambda: dev.search_exhaustive_grouped(Q, 10, filters, qf, stats=True)  # noqa: E731
    call = grouped if dtype == "float16" else lambda: dev.search_exhaustive(Q, 10, stats=True)
    off = call()
    dev.set_option("scan_matrix_float", 1)
    on = call()
    assert dev.launch_geometry()["kernel_mode"] == 3 and dev.scan_rescored() == {"scored": 0, "rescored": 0}
    _same_results(on, off, dtype)


def test_python_index_round_trip():  # set before the device mirror exists: reaches the mirror made later; toggled: the one there is
    import flatnav_amd

    classes = [c for c in vars(flatnav_amd._core.index).values() if isinstance(c, type) and hasattr(c, "search_exhaustive")]
    assert len(classes) == 8 and all(callable(getattr(c, "set_exhaustive_matrix", None)) for c in classes)
    X, Q = (a.astype(np.float16) for a in ds.randn(600, 40, 64, seed=9))
    index = flatnav_amd.index.create("l2", 64, 600, 8, flatnav_amd.data_type.DataType.float16)
    index.add(X, 16, labels=list(range(600)))
    got = []
    for on, mode in ((True, 5), (False, 3), (True, 5)):  # (the first: no mirror yet)
        index.set_exhaustive_matrix(on, float_rows=True)
        got.append(index.search_exhaustive(Q, 10))
        geom = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False).launch_geometry()
        assert geom["kernel_mode"] == mode and geom["kernel"] == ("exhaustive_scan_matrix_float" if on else "exhaustive_scan"), (on, geom)
    for d, l in got[1:]:
        assert np.array_equal(l, got[0][1]) and np.array_equal(d.view(np.uint32), got[0][0].view(np.uint32))
