"""The float16 matrix engine of the exhaustive search on the CPU (option "scan_matrix_float"): when scan_matrix_shape
(flatnav_amd/csrc/launch_plan.hpp) gives it a call and the launch it then gets, and that scan_margin (csrc/scan_select.hpp) covers
the distance between a re-associated float32 score and the vector scan's lane-by-lane distance (tests/distance_model.py).
tests/scan_matrix_f16_harness.cpp is compiled with g++ and loaded with ctypes."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import distance_model as dm
import row_classes as rc

TESTS = os.path.dirname(os.path.abspath(__file__))
U8, F16, F32 = 0, 8, 9  # FNV_DTYPE_* (include/flatnav_hip.h)
FIELDS = ("on", "float_rows", "group_lanes", "tile", "tiles", "segments", "lds", "block")
_LIB = []


def lib():
    if not _LIB:
        tmp = tempfile.mkdtemp(prefix="flatnav_scan_matrix_f16_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libscan_matrix_f16_harness.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", os.path.join(TESTS, "scan_matrix_f16_harness.cpp"), "-o", out])
        _LIB.append(C.CDLL(out))
        _LIB[0].smf_margin.argtypes = [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return _LIB[0]


def shape(dtype, dim, nq, K, live, segment_rows=0, matrix=0, matrix_float=1, num_cus=256) -> dict:
    res = (C.c_int64 * len(FIELDS))()
    lib().smf_shape((C.c_int64 * 10)(dtype, dim, max(live, 1), num_cus, segment_rows, matrix, matrix_float, nq, K, live), res)
    return dict(zip(FIELDS, (int(v) for v in res)))


def test_shapes():
    # a short row, whole in registers (16 chunks = 8 steps): 344 bytes per query, two sub-tiles in the 32 KB budget, seven blocks per CU
    assert shape(F16, 128, 10_000, 10, 1_000_000) == dict(on=1, float_rows=1, group_lanes=8, tile=64, tiles=157, segments=11, lds=64 * 344, block=64)
    # a long row (192 chunks = 96 steps, twelve register spans): one sub-tile, one block per CU, the most segments a launch takes
    assert shape(F16, 1536, 33, 10, 100_000) == dict(on=1, float_rows=1, group_lanes=64, tile=32, tiles=2, segments=64, lds=32 * 3160, block=64)
    assert shape(F16, 200, 48, 10, 1500, segment_rows=256)["segments"] == 6 and shape(F16, 200, 48, 10, 1500)["group_lanes"] == 8
    assert [shape(F16, 300, 48, 10, 1500)["group_lanes"], shape(F16, 600, 48, 10, 1500)["group_lanes"]] == [16, 32]
    # refused: 32 lists of K keys beside 32 rows' steps beyond a block's 160 KB
    assert [shape(F16, 1536, 100, K, 5000)["on"] for K in (100, 255, 256, 1024)] == [1, 1, 0, 0]
    assert shape(F16, 32, 100, 1024, 5000)["on"] == 0
    # each option governs its own element types, and neither the other's
    assert [shape(t, 128, 100, 10, 5000)["on"] for t in (F32, F16, U8)] == [0, 1, 0]
    assert [shape(t, 128, 100, 10, 5000, matrix=1, matrix_float=0)["on"] for t in (F32, F16, U8)] == [0, 0, 1]
    assert shape(U8, 128, 100, 10, 5000, matrix=1, matrix_float=1)["float_rows"] == 0


def _edge_rows(rng, n, nq, dim, normalize):
    """Random normal rows and queries as float16, and the values that strain a margin: copies of queries, one last-place step
    away from a query, subnormals only, the largest finite magnitude."""
    X, Q = rng.standard_normal((n, dim)), rng.standard_normal((nq, dim))
    if normalize:
        X, Q = X / np.linalg.norm(X, axis=1, keepdims=True), Q / np.linalg.norm(Q, axis=1, keepdims=True)
    X, Q = X.astype(np.float16), Q.astype(np.float16)
    X[0], X[1] = Q[0], Q[1]
    X[1, dim // 2] = np.nextafter(X[1, dim // 2], np.float16(np.inf))
    X[2:5] = (rng.integers(-1023, 1024, (3, dim)) * 2.0 ** -24).astype(np.float16)
    Q[2] = (rng.integers(-1023, 1024, dim) * 2.0 ** -24).astype(np.float16)
    if not normalize:
        X[5], X[6], Q[3] = 65504, -65504, 65504
        X[7], Q[4] = X[7] * np.float16(1000), Q[0] * np.float16(1000)
        X[8] = Q[4]  # L2 = 0 by cancellation of large norms
    return X, Q


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", [50, 128, 200, 1536])
def test_margin_covers_a_reassociated_sum(dim, metric, flush):
    """scan_margin >= |float32 score from numpy's pairwise sums - the lane-by-lane model's distance| on every pair, also when the
    re-associated dot product loses its binary16 subnormals (assumption (d) of scan_select.hpp)."""
    rng = np.random.default_rng(dim + len(metric))
    for normalize in (False, True):
        X, Q = _edge_rows(rng, 40, 30, dim, normalize)
        geo = rc.walk_of_row("float16", dim)
        P = 16 * ((geo["nchunks"] + geo["tail_chunks"] + 1) // 2)
        exact = dm.distances("float16", metric, X, Q).view(np.float32).astype(np.float64)
        x, q = X.astype(np.float32), Q.astype(np.float32)
        rn, qn = (x * x).sum(1, dtype=np.float32), (q * q).sum(1, dtype=np.float32)
        xd, qd = (np.where(np.abs(a) < 2.0 ** -14, np.float32(0), a) if flush else a for a in (x, q))
        dot = np.stack([(xd * v).sum(1, dtype=np.float32) for v in qd])
        score = (rn[None, :] + qn[:, None]) - np.float32(2) * dot if metric == "l2" else np.float32(1) - dot
        assert score.dtype == np.float32
        RN, QN = (np.ascontiguousarray(np.broadcast_to(a, score.shape), np.float32) for a in (rn[None, :], qn[:, None]))
        margin = np.empty(score.shape, np.float32)
        lib().smf_margin(P, int(metric == "ip"), RN.ctypes.data, QN.ctypes.data, score.size, margin.ctypes.data)
        err = np.abs(score.astype(np.float64) - exact)
        assert np.isfinite(err).all() and np.isfinite(margin).all()
        print("margin, dim %d %s%s%s: worst error / margin = %.4f" % (dim, metric, " normalised" if normalize else "", " flushed" if flush else "",
                                                                      float((err / margin).max())))
        assert (err <= margin).all()
