"""scan_matrix_shape (flatnav_amd/csrc/launch_plan.hpp) on the CPU: when the exhaustive search's matrix engine takes a call, and
the launch it then gets.  tests/scan_matrix_harness.cpp is compiled with g++ and loaded with ctypes."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
U8, I8, F16, F32 = 0, 4, 8, 9  # FNV_DTYPE_* (include/flatnav_hip.h)
FIELDS = ("on", "tile", "tiles", "segments", "lds", "block", "partial_bytes")
_LIB = []


def shape(dtype, dim, nq, K, live, segment_rows=0, matrix=1, num_cus=256) -> dict:
    if not _LIB:
        tmp = tempfile.mkdtemp(prefix="flatnav_scan_matrix_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libscan_matrix_harness.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", os.path.join(TESTS, "scan_matrix_harness.cpp"), "-o", out])
        _LIB.append(C.CDLL(out))
    res = (C.c_int64 * len(FIELDS))()
    _LIB[0].smh_shape((C.c_int64 * 9)(dtype, dim, max(live, 1), num_cus, segment_rows, matrix, nq, K, live), res)
    return dict(zip(FIELDS, (int(v) for v in res)))


@pytest.mark.parametrize("dtype,dim,nq,K,live,segment_rows", [
    (U8, 128, 10_000, 10, 1_000_000, 0),   # c2-uint8: the widest tile
    (I8, 128, 10_000, 100, 1_000_000, 0),  # lists that leave room for one sub-tile
    (U8, 128, 60_000, 256, 1_000_000, 0),  # partial lists near their 256 MB bound
    (U8, 400, 48, 10, 1500, 256),          # split rows, forced segments
    (I8, 3072, 33, 1, 1500, 0),            # rows of several spans: one sub-tile
    (U8, 1, 1, 1, 1, 0),
])
def test_shapes_the_engine_takes(dtype, dim, nq, K, live, segment_rows):
    s = shape(dtype, dim, nq, K, live, segment_rows)
    assert s["on"] == 1 and s["block"] == 64, s
    assert s["tile"] % 32 == 0 and 32 <= s["tile"] <= 128 and s["tile"] < nq + 32 and (dim <= 128 or s["tile"] == 32), s
    assert s["tiles"] == -(-nq // s["tile"]) and s["lds"] <= 160 * 1024, s
    if segment_rows:
        assert s["segments"] == min(1024, -(-live // segment_rows)), s
    else:
        assert s["segments"] == 1 or (s["partial_bytes"] <= 256 << 20 and s["tiles"] * s["segments"] <= 256 * 8), s


def test_shapes_the_engine_declines():
    assert shape(U8, 128, 10_000, 10, 1_000_000)["tile"] == 128
    assert [shape(t, 128, 100, 10, 5000)["on"] for t in (F32, F16, U8, I8)] == [0, 0, 1, 1]
    assert shape(U8, 128, 100, 10, 5000, matrix=0)["on"] == 0
    assert shape(U8, 32, 100, 1024, 5000)["on"] == 0  # 32 lists of 1024 keys: 256 KB
    assert [shape(I8, 3072, 100, K, 5000)["on"] for K in (100, 255, 256, 512)] == [1, 1, 0, 0]
