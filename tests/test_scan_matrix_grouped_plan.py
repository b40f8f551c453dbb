"""The matrix engines' launch for a GROUPED exhaustive call on the CPU (option "scan_matrix_grouped"): scan_matrix_shape
(csrc/launch_plan.hpp) with its filter_rows argument.  tests/scan_matrix_grouped_harness.cpp: g++ and ctypes."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

U8, I8, F16, F32 = 0, 4, 8, 9  # FNV_DTYPE_* (include/flatnav_hip.h)
OWN = {U8: (1, 0, 0), I8: (1, 0, 0), F16: (0, 1, 0), F32: (0, 0, 1)}  # the element type's own option of the three
FIELDS = ("on", "tile", "tiles", "segments", "lds", "tile_bound", "queue_bytes", "max_lds")
_LIB = []


def shape(dtype, dim, nq, K, live, rows=-1, grouped=1, own=None, segment_rows=0) -> dict:
    if not _LIB:
        out = os.path.join(tempfile.mkdtemp(prefix="flatnav_scan_matrix_grouped_"), "harness.so")
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_matrix_grouped_harness.cpp")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", src, "-o", out])
        _LIB.append(C.CDLL(out))
    res = (C.c_int64 * len(FIELDS))()
    own = OWN[dtype] if own is None else own
    _LIB[0].smg_shape((C.c_int64 * 13)(dtype, dim, max(live, 1), 256, segment_rows, *own, grouped, nq, K, live, rows), res)
    return dict(zip(FIELDS, (int(v) for v in res)))


# what the three engines' own plan tests hold for ungrouped calls (tests/test_scan_matrix*_plan.py), whatever the new option says
UNGROUPED = [((F32, 128, 10_000, 10, 1_000_000), (64, 157, 11, 64 * 344)), ((F16, 128, 10_000, 10, 1_000_000), (64, 157, 11, 64 * 344)),
             ((F32, 1536, 33, 10, 100_000), (32, 2, 64, 32 * 3160)), ((F16, 1536, 33, 10, 100_000), (32, 2, 64, 32 * 3160))]


@pytest.mark.parametrize("args, want", UNGROUPED)
def test_ungrouped_calls_are_shaped_as_before(args, want):
    for grouped in (0, 1):
        for rows in (-1, 0):  # the argument left out, and given as 0
            s = shape(*args, rows=rows, grouped=grouped)
            assert (s["on"], s["tile"], s["tiles"], s["segments"], s["lds"]) == (1,) + want, (grouped, rows)
    assert shape(U8, 128, 10_000, 10, 1_000_000, rows=0)["tile"] == 128 and shape(I8, 3072, 100, 255, 5000, rows=0)["on"] == 1


@pytest.mark.parametrize("dtype", [U8, I8, F16, F32])
@pytest.mark.parametrize("dim, nq, K, live, rows", [(128, 10_000, 10, 1_000_000, 18), (128, 10_000, 10, 1_000_000, 2050), (40, 230, 100, 2203, 10),
                                                    (200, 33, 1, 2203, 3), (1536, 500, 10, 100_000, 40), (97, 5, 10, 50, 7)])
def test_grouped_calls(dtype, dim, nq, K, live, rows):
    assert shape(dtype, dim, nq, K, live, rows=rows, grouped=0)["on"] == 0  # the new option off: the grouped vector scan
    assert shape(dtype, dim, nq, K, live, rows=rows, own=(0, 0, 0))["on"] == 0  # ... or the element type's own
    s, plain = shape(dtype, dim, nq, K, live, rows=rows), shape(dtype, dim, nq, K, live)
    assert s["on"] == 1 and s["tile"] % 32 == 0 and 32 <= s["tile"] <= plain["tile"]
    per_query = plain["lds"] // plain["tile"]
    assert s["lds"] == s["tile"] * per_query + s["queue_bytes"] <= s["max_lds"] and s["queue_bytes"] == 1024
    assert s["tiles"] == s["tile_bound"] > 0 and 1 <= s["segments"] <= 64
    assert shape(dtype, dim, nq, K, live, rows=rows, segment_rows=250)["segments"] == min(1024, -(-live // 250))


def test_a_k_that_overflows_the_lds_keeps_the_vector_scan():
    # 3072 one-byte elements, K = 255: 32 queries and their lists take 163 712 of a block's 163 840 bytes -- the queue no longer fits
    assert [shape(I8, 3072, 100, K, 5000, rows=4)["on"] for K in (100, 254, 255, 1024)] == [1, 0, 0, 0]
    assert [shape(t, 32, 100, 1024, 5000, rows=4)["on"] for t in (U8, F16, F32)] == [0, 0, 0]
