"""The float32 matrix engine of the exhaustive search on the CPU (option "scan_matrix_float32"): the launch scan_matrix_shape
(csrc/launch_plan.hpp) gives it, and that scan_margin_f32 (csrc/scan_select.hpp) covers the distance between a float32 score of
bfloat16-narrowed operands and the vector scan's lane-by-lane distance.  tests/scan_matrix_f32_harness.cpp: g++ and ctypes."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import distance_model as dm
import row_classes as rc

U8, F16, F32 = 0, 8, 9  # FNV_DTYPE_* (include/flatnav_hip.h)
FIELDS = ("on", "float_rows", "float32_rows", "group_lanes", "tile", "tiles", "segments", "lds", "block")
_LIB = []


def lib():
    if not _LIB:
        out = os.path.join(tempfile.mkdtemp(prefix="flatnav_scan_matrix_f32_"), "harness.so")
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_matrix_f32_harness.cpp")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", src, "-o", out])
        _LIB.append(C.CDLL(out))
        _LIB[0].smf32_margin.argtypes = [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return _LIB[0]


def shape(dtype, dim, nq, K, live, segment_rows=0, options=(0, 0, 1), num_cus=256) -> dict:
    """options = ("scan_matrix", "scan_matrix_float", "scan_matrix_float32")"""
    res = (C.c_int64 * len(FIELDS))()
    lib().smf32_shape((C.c_int64 * 11)(dtype, dim, max(live, 1), num_cus, segment_rows, *options, nq, K, live), res)
    return dict(zip(FIELDS, (int(v) for v in res)))


def test_shapes():
    # 128-d: 32 chunks = 8 steps, whole in registers; 344 bytes per query as float16's, two sub-tiles in the 32 KB budget
    assert shape(F32, 128, 10_000, 10, 1_000_000) == dict(on=1, float_rows=0, float32_rows=1, group_lanes=8, tile=64, tiles=157, segments=11,
                                                          lds=64 * 344, block=64)
    # a long row (384 chunks = 96 steps, twelve register spans): one sub-tile, one block per CU, the most segments a launch takes
    assert shape(F32, 1536, 33, 10, 100_000) == dict(on=1, float_rows=0, float32_rows=1, group_lanes=64, tile=32, tiles=2, segments=64,
                                                     lds=32 * 3160, block=64)
    assert shape(F32, 100, 48, 10, 1500, segment_rows=256)["segments"] == 6
    assert [shape(F32, d, 48, 10, 1500)["group_lanes"] for d in (100, 150, 300, 768)] == [8, 16, 32, 64]
    # refused: 32 lists of K keys beside 32 rows' steps beyond a block's 160 KB
    assert [shape(F32, 1536, 100, K, 5000)["on"] for K in (100, 255, 256, 1024)] == [1, 1, 0, 0]
    assert shape(F32, 32, 100, 1024, 5000)["on"] == 0
    # each option governs its own element types, and neither of the others'
    for options, on in (((0, 0, 1), [1, 0, 0]), ((0, 1, 0), [0, 1, 0]), ((1, 0, 0), [0, 0, 1]), ((1, 1, 0), [0, 1, 1]), ((0, 0, 0), [0, 0, 0])):
        assert [shape(t, 128, 100, 10, 5000, options=options)["on"] for t in (F32, F16, U8)] == on, options
    assert [shape(F16, 128, 100, 10, 5000, options=(1, 1, 1))[k] for k in ("float_rows", "float32_rows")] == [1, 0]


def bf16(a, tie=False):
    """float32 -> the nearest bfloat16 (ties to even) as float32, by bit arithmetic; `tie`: the midpoint above it instead."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000) | (0x8000 if tie else 0)).astype(np.uint32).view(np.float32)


def _edge_rows(rng, n, nq, dim, normalize):
    """Normal rows and queries, and what strains a margin: copies of queries, one last-place step from a query, a difference below
    bfloat16's precision, bfloat16 rounding ties, subnormals only, large magnitudes, L2 = 0 by cancellation of large norms."""
    X, Q = rng.standard_normal((n, dim)), rng.standard_normal((nq, dim))
    if normalize:
        X, Q = X / np.linalg.norm(X, axis=1, keepdims=True), Q / np.linalg.norm(Q, axis=1, keepdims=True)
    X, Q = X.astype(np.float32), Q.astype(np.float32)
    X[0], X[1], X[9] = Q[0], Q[1], Q[5] * np.float32(1 + 2.0 ** -12)
    X[1, dim // 2] = np.nextafter(X[1, dim // 2], np.float32(np.inf))
    X[10], X[11], Q[6] = bf16(X[10], True), bf16(Q[6], True), bf16(Q[6], True)
    X[2:5] = (rng.integers(-(2 ** 23) + 1, 2 ** 23, (3, dim)) * 2.0 ** -149).astype(np.float32)
    Q[2] = (rng.integers(-(2 ** 23) + 1, 2 ** 23, dim) * 2.0 ** -149).astype(np.float32)
    if not normalize:
        X[5], X[6], Q[3] = 1e17, -1e17, 1e17
        X[7], Q[4] = X[7] * np.float32(1e15), Q[0] * np.float32(1e15)
        X[8] = Q[4]
    return X, Q


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", [50, 128, 200, 1536])
def test_margin_covers_a_narrowed_reassociated_sum(dim, metric, flush):
    """scan_margin_f32 >= |float32 score from bfloat16-narrowed operands - the lane-by-lane model's distance| on every pair, also
    when subnormal operands are flushed (assumption (d') of scan_select.hpp)."""
    rng = np.random.default_rng(dim + len(metric))
    for normalize in (False, True):
        X, Q = _edge_rows(rng, 40, 30, dim, normalize)
        geo = rc.walk_of_row("float32", dim)
        P = 16 * ((geo["nchunks"] + geo["tail_chunks"] + 3) // 4)
        exact = dm.distances("float32", metric, X, Q).view(np.float32).astype(np.float64)
        rn, qn = (X * X).sum(1, dtype=np.float32), (Q * Q).sum(1, dtype=np.float32)
        xd, qd = (bf16(np.where(np.abs(a) < 2.0 ** -126, np.float32(0), a) if flush else a) for a in (X, Q))
        dot = np.stack([(xd * v).sum(1, dtype=np.float32) for v in qd])
        score = (rn[None, :] + qn[:, None]) - np.float32(2) * dot if metric == "l2" else np.float32(1) - dot
        RN, QN = (np.ascontiguousarray(np.broadcast_to(a, score.shape), np.float32) for a in (rn[None, :], qn[:, None]))
        margin = np.empty(score.shape, np.float32)
        lib().smf32_margin(P, int(metric == "ip"), RN.ctypes.data, QN.ctypes.data, score.size, margin.ctypes.data)
        err = np.abs(score.astype(np.float64) - exact)
        print("margin, dim %d %s normalised %d flushed %d: worst error / margin = %.4f" % (dim, metric, normalize, flush, float((err / margin).max())))
        assert score.dtype == np.float32 and np.isfinite(err).all() and np.isfinite(margin).all() and (err <= margin).all()
