"""The exhaustive search's float32 matrix engine on the GPU (option "scan_matrix_float32", csrc/scan_matrix_f32.hpp): on float32
indexes it writes exactly what the vector scan writes -- labels, distance bits, counts, n_dist -- and both sit within the float
bar of numpy float64 distances.  A margin too narrow, a wrong operand or accumulator mapping, a chunk from the wrong table or a
rescoring in another lane order shows as a difference between the engines."""
import ctypes

import numpy as np
import pytest

import row_classes as rc
import test_gpu_scan_matrix_f16 as f16
import test_scan_matrix_f32_plan as plan
from distance_model import dist64
from flatnav_amd import datasets as ds
from flatnav_amd import hip
from test_gpu_exhaustive import _build, _same_results

pytestmark = pytest.mark.gpu


class _Float32Option:  # the float16 file's _both_engines toggles "scan_matrix_float": here it toggles this engine's option
    def __init__(self, dev):
        self.dev = dev

    def set_option(self, name, value):
        self.dev.set_option("scan_matrix_float32" if name == "scan_matrix_float" else name, value)

    def __getattr__(self, name):
        return getattr(self.dev, name)


def _both_engines(dev, D, labels, Q, K, what, allowed=None, mode=6):
    """Engine on (kernel `mode`) and off (kernel 3): the same bytes, finite distances within the float bar of D, rows among its top-K."""
    return f16._both_engines(_Float32Option(dev), D, labels, Q, K, what, allowed=allowed, mode=mode)


def _dist64(X, Q, metric):  # (a float64 distance beyond float32's range is reported as an infinity: not held to the bar)
    with np.errstate(invalid="ignore", over="ignore"):
        D = dist64(X, Q, metric)
        return np.where(np.abs(D) > np.finfo(np.float32).max, np.sign(D) * np.inf, D)


# tests/row_classes.py, float32: a sub-chunk row (one chunk of a step's four), one whole chunk, split rows (24 main chunks and a
# tail of one and of two), a row of exactly one register span, rows of several spans with G = 16, 32 and 64 (the others: G = 8);
# dims 8 and 9: two and three chunks of a step's four
DIMS = [rc.dim_of("float32", c) for c in ("8x1-clamped", "8x1-clamped-dense", "8x3-tail1", "8x3-tail2", "8x4-full", "16x4-clamped",
                                          "32x4-clamped", "64x4-clamped")] + [8, 9]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", DIMS)
def test_geometry(oracle_mod, metric, dim):
    rng = np.random.default_rng(dim * 7 + len(metric))
    n = 1500
    X, Q = ds.randn(n, 48, dim, seed=dim, normalize=metric == "ip")
    X, labels, dev = _build(oracle_mod, metric, "float32", X, (rng.permutation(n) + 3).astype(np.int32), M=8, efc=16)
    allowed, D = rng.choice(n, n // 10, replace=False) + 3, dist64(X, Q, metric)
    for K in (1, 10, 100):
        for seg in (0, 256):  # automatic, and many segments with a real merge
            dev.set_option("scan_segment_rows", seg)
            _both_engines(dev, D, labels, Q, K, (metric, dim, K, seg, "all"))
            _both_engines(dev, D, labels, Q, K, (metric, dim, K, seg, "10 %"), allowed=allowed)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_adversarial_values(oracle_mod, metric):
    """Duplicates (the node id decides), rows one float32 step from a query, rows that differ from a query below bfloat16's
    precision, bfloat16 rounding ties, subnormals only, magnitudes that narrow to bfloat16 infinity, queries equal to rows (L2 = 0
    by cancellation of large norms), and a NaN and a +inf row, which the engine must let through to rank as ever."""
    n, dim = 400, 200
    X, Q = ds.randn(n, 34, dim, seed=3, normalize=metric == "ip")
    rng = np.random.default_rng(4)
    if metric == "ip":  # non-negative queries: no dot product with a huge row cancels (no float32 sum meets a relative bar then)
        Q = np.abs(Q)
    X[10:50] = X[9]
    X[100], X[101], X[102], X[103] = Q[0], Q[0], Q[1], Q[1]
    X[101, 70], X[103, 199] = np.nextafter(X[101, 70], np.float32(np.inf)), np.nextafter(X[103, 199], np.float32(-np.inf))
    X[104], X[105] = Q[5] * np.float32(1 + 2.0 ** -12), Q[5] * np.float32(1 - 2.0 ** -13)
    X[106], X[107], Q[6] = plan.bf16(X[106], True), plan.bf16(Q[7], True), plan.bf16(Q[6], True)
    X[60:64] = (rng.integers(-(2 ** 23) + 1, 2 ** 23, (4, dim)) * 2.0 ** -149).astype(np.float32)
    X[120], X[121] = 3.4e38, -3.4e38
    if metric == "l2":
        X[122], X[123] = X[122] * np.float32(1e15), (3.4e38 * rng.choice([-1.0, 1.0], dim)).astype(np.float32)
        Q[2], Q[3], Q[4], Q[8] = X[120], X[123], X[61], X[122]
    o = oracle_mod.OracleIndex.create(metric, dim, n, 8, "float32")
    o.add(np.clip(X, -1e3, 1e3), 16)  # (the graph is built on tame rows, in row order; the scan never reads it)
    X[80, 5], X[81, 7] = np.nan, np.inf
    nodes = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)
    blob = np.concatenate([X.view(np.uint8).reshape(n, 4 * dim), nodes[:, o.data_size:]], axis=1)
    dev = hip.DeviceIndex.upload(blob.reshape(-1), blob.shape[1], 4 * dim, o.M, n, "float32", metric, dim)
    labels, D = np.arange(n, dtype=np.int32), _dist64(X, Q, metric)
    for K in (1, 10, 200):
        full = _both_engines(dev, D, labels, Q, K, (metric, K))
    d, l, st = _both_engines(dev, D, labels, Q, 200, (metric, "edge rows"), allowed=np.arange(60, 111))
    assert (l[:, 50] == 80).all() and np.isnan(d[:, 50]).all() and (l[:, 51:] == -1).all()
    if metric == "l2":  # (queries 2 and 3 are infinitely far from every row but their own; rows 60 .. 63 differ by subnormals: squares of 0)
        assert (l[9:, 49] == 81).all() and np.isposinf(d[9:, 49]).all() and (d[[0, 4], 0] == 0).all() and l[0, 0] == 100 and l[4, 0] == 60
        assert (full[0][[2, 3, 8], 0] == 0).all() and (full[1][[2, 3, 8], 0] == [120, 123, 122]).all()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_edges_of_tiles_and_of_k(oracle_mod, n):
    X, Qall = ds.randn(n, 257, 32, seed=n)
    X, labels, dev = _build(oracle_mod, "l2", "float32", X, (np.random.default_rng(n).permutation(n) + 3).astype(np.int32), M=8, efc=16)
    modes = set()
    for nq in (1, 31, 33, 257):
        D = dist64(X, Qall[:nq], "l2")
        for K in sorted({1, n, n + 5, 1024}):
            mode = 6 if plan.shape(plan.F32, 32, nq, K, n)["on"] else 3  # (K = 1024: 32 lists do not fit a block's LDS)
            _both_engines(dev, D, labels, Qall[:nq], K, (n, nq, K), mode=mode)
            modes.add(mode)
    assert modes == {3, 6}


def test_the_prefilter_filters(oracle_mod):
    """Every pair is scored on the matrix cores and few are scored again.  The cap is no performance figure: it fails an engine
    that passes by rescoring everything.  The margin simulated with numpy on this input, 32 rows a step in the launch's three
    segments with the K-th distance taken at the start of a step, lets 15 307 of the 256 000 pairs through: 6.0 % against 25 %."""
    n, nq = 4000, 64
    X, Q = ds.randn(n, nq, 128, seed=11)
    X, labels, dev = _build(oracle_mod, "l2", "float32", X, None, M=8, efc=16)
    dev.set_option("scan_segment_rows", 0)
    _both_engines(dev, dist64(X, Q, "l2"), labels, Q, 10, "prefilter")
    assert dev.scan_rescored() == {"scored": 0, "rescored": 0}  # (the vector scan ran last)
    dev.set_option("scan_matrix_float32", 1)
    dev.search_exhaustive(Q, 10)
    r = dev.scan_rescored()
    print("float32 matrix engine: %d of %d pairs rescored (%.2f %%)" % (r["rescored"], r["scored"], 100.0 * r["rescored"] / r["scored"]))
    assert dev.launch_geometry()["segments"] == 3 and r["scored"] == nq * n and 0 < r["rescored"] <= r["scored"] // 4


@pytest.mark.parametrize("dtype", ["float32", "uint8", "float16"])
def test_not_applicable_is_not_invalid(oracle_mod, dtype):
    """uint8 and float16 indexes, and the grouped call on a float32 index, keep the vector scan with the option on: kernel 3."""
    rng = np.random.default_rng(5)
    X, Q = rng.integers(0, 60, (500, 40)).astype(dtype), rng.integers(0, 60, (33, 40)).astype(dtype)
    _, _, dev = _build(oracle_mod, "l2", dtype, X, None, M=8, efc=16)
    filters, qf = [rng.choice(500, 50, replace=False), np.arange(100, 130)], rng.integers(-1, 2, 33).astype(np.int32)
    grouped = lambda: dev.search_exhaustive_grouped(Q, 10, filters, qf, stats=True)  # noqa: E731
    call = grouped if dtype == "float32" else lambda: dev.search_exhaustive(Q, 10, stats=True)
    off = call()
    dev.set_option("scan_matrix_float32", 1)
    on = call()
    assert dev.launch_geometry()["kernel_mode"] == 3 and dev.scan_rescored() == {"scored": 0, "rescored": 0}
    _same_results(on, off, dtype)


def test_python_index_round_trip():  # set before the device mirror exists: reaches the mirror made later; toggled: the one there is
    import flatnav_amd

    X, Q = ds.randn(600, 40, 64, seed=9)
    index = flatnav_amd.index.create("l2", 64, 600, 8)
    index.add(X, 16, labels=list(range(600)))
    got = []
    for on, mode in ((True, 6), (False, 3), (True, 6)):  # (the first: no mirror yet)
        index.set_exhaustive_matrix(on, float32_rows=True)
        got.append(index.search_exhaustive(Q, 10))
        geom = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False).launch_geometry()
        assert geom["kernel_mode"] == mode and geom["kernel"] == ("exhaustive_scan_matrix_float32" if on else "exhaustive_scan"), (on, geom)
    for d, l in got[1:]:
        assert np.array_equal(l, got[0][1]) and np.array_equal(d.view(np.uint32), got[0][0].view(np.uint32))
