"""The block form of the float matrix engines in the launch planner (option "scan_matrix_block"; csrc/launch_plan.hpp,
scan_block_shape), on the CPU: when it takes a call and the shape it gives it.  tests/scan_matrix_block_harness.cpp: g++ and ctypes."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

U8, F16, F32 = 0, 8, 9  # FNV_DTYPE_* (include/flatnav_hip.h)
FIELDS = ("on", "tile", "tiles", "segments", "lds", "block", "waves", "wave_subtiles")
MAX_LDS = 160 << 10  # kScanMaxLds
_LIB = []


def lib():
    """The harness, compiled once per process (tests/exhaustive_sequences.py calls it with inputs of its own)."""
    if not _LIB:
        out = os.path.join(tempfile.mkdtemp(prefix="flatnav_scan_matrix_block_"), "harness.so")
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_matrix_block_harness.cpp")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", src, "-o", out])
        _LIB.append(C.CDLL(out))
        _LIB[0].smb_vector_lds.restype = C.c_int64
    return _LIB[0]


def shape(dtype, dim, nq, K, live=1_000_000, own=1, block=1, grouped=0, filter_rows=0, radius=0, segment_rows=0, listed=1) -> dict:
    """`listed`: the call has one filter -- the class the block form takes (unfiltered calls are declined by measurement)."""
    res = (C.c_int64 * len(FIELDS))()
    options = (1 if dtype == U8 else 0, own if dtype == F16 else 0, own if dtype == F32 else 0, grouped, block)
    lib().smb_shape((C.c_int64 * 16)(dtype, dim, live, 256, segment_rows, *options, nq, K, live, filter_rows, radius, listed and not filter_rows), res)
    return dict(zip(FIELDS, (int(v) for v in res)))


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("dim", [128, 768])
def test_off_and_declined_calls_keep_the_wave_shape(dtype, dim):
    for nq, K, seg in [(1, 10, 0), (33, 1, 0), (128, 100, 256), (10_000, 10, 0)]:
        wave = shape(dtype, dim, nq, K, block=0, segment_rows=seg)
        assert wave["on"] and wave["block"] == 64 and wave["waves"] == 0, wave
        # a range search and a grouped call (with and without "scan_matrix_grouped") are declined: the shape with the option off
        # ... and, by measurement (profiles/scan_matrix_block.md), the unfiltered call
        for kw in ({"radius": 1}, {"filter_rows": 3, "grouped": 1}, {"filter_rows": 3}, {"listed": 0}):
            assert shape(dtype, dim, nq, K, segment_rows=seg, **kw) == shape(dtype, dim, nq, K, block=0, segment_rows=seg, **kw), kw
    assert shape(dtype, dim, 128, 10, own=0) == shape(dtype, dim, 128, 10, own=0, block=0) and not shape(dtype, dim, 128, 10, own=0)["on"]
    assert shape(U8, dim, 128, 10) == shape(U8, dim, 128, 10, block=0) and shape(U8, dim, 128, 10)["block"] == 64  # 1-byte: its own engine


# (nq, dim) -> (W, sub-tiles per wavefront) of a single-filter call at K = 10: LDS per query 344 bytes at 128-d (ring 16.75 KB;
# 80 KB hold five sub-tiles); 768-d: rows beyond the register span, declined by measurement (profiles/scan_matrix_block.md)
@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("dim,nq,want", [(128, 32, None), (128, 33, (2, 1)), (128, 128, (4, 1)), (128, 10_000, (4, 1)),
                                         (768, 32, None), (768, 33, None), (768, 128, None), (768, 10_000, None)])
def test_waves_and_tile(dtype, dim, nq, want):
    s = shape(dtype, dim, nq, 10)
    if want is None:  # one sub-tile, or long rows: the wave form
        assert s == shape(dtype, dim, nq, 10, block=0) and s["waves"] == 0
        return
    steps = dim // 16
    assert (s["waves"], s["wave_subtiles"]) == want and s["block"] == 64 * s["waves"] and s["tile"] == 32 * want[0] * want[1]
    assert s["tiles"] == -(-nq // s["tile"]) and 1 <= s["segments"] <= 64
    assert s["lds"] == s["tile"] * (steps * 32 + 8 * 10 + 8) + 2 * (min(steps, 8) * 1024 + 384) <= MAX_LDS


def test_lds_bound_and_wide_wavefronts():
    assert shape(F16, 16, 129, 1)["wave_subtiles"] == 2 and shape(F16, 16, 129, 1)["tile"] == 256  # five sub-tiles on four wavefronts
    assert shape(F16, 16, 10_000, 1)["wave_subtiles"] == 4  # (the accumulators' bound)
    for dtype in (F16, F32):
        for dim in (1, 50, 128, 200, 768, 1536, 4000):
            for K in (1, 10, 100, 1024):
                for nq in (33, 257, 10_000):
                    s = shape(dtype, dim, nq, K)
                    assert s["lds"] <= MAX_LDS and (not s["on"] or s["block"] == 64 * max(1, s["waves"])), (dtype, dim, K, nq, s)
                    assert s["waves"] == 0 or dim * (2 if dtype == F16 else 4) <= (256 if dtype == F16 else 512), (dtype, dim, s)  # never beyond 8 steps
