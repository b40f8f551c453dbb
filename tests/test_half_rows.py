"""The half-width mirror of float32 rows (flatnav_amd/csrc/half_rows.hpp) on the CPU: tests/half_rows_harness.cpp is compiled
with g++ and loaded with ctypes.  Checked here, without a GPU: the chunk -> (unit, half) map is a bijection onto the mirror row
for every eligible row configuration; a lane-by-lane emulation of the float32 kernel and of the mirror kernel gives bit-equal
distances on binary16-representable rows against arbitrary float32 queries (and tells a wrong order apart); the bitwise
round-trip predicate agrees with numpy; which geometries are eligible."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from flatnav_amd.hip import DTYPE_ORD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "half_rows_harness.cpp")
FLAGS = ["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"]
F32 = DTYPE_ORD["float32"]
L2, IP = 0, 1
_lib = None
_tmp = None


def tmpdir() -> str:
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="flatnav_half_rows_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        out = os.path.join(tmpdir(), "libhalf_rows_harness.so")
        subprocess.check_call(FLAGS + ["-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.hrh_eligible.argtypes = [C.c_int, C.c_uint32, C.c_uint64]
        L.hrh_eligible_cfg.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32]
        L.hrh_cfg.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.hrh_unit_map.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.hrh_first_chunk_of_unit.argtypes = [C.c_uint32] * 3
        L.hrh_first_chunk_of_unit.restype = C.c_uint32
        L.hrh_round_trip.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.hrh_convert_row.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hrh_dist_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int]
        L.hrh_dist_f32.restype = C.c_float
        L.hrh_dist_half.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        L.hrh_dist_half.restype = C.c_float
        _lib = L
    return _lib


def eligible_cfgs():
    """(G, CU) of the row configurations a mirror exists for."""
    L = lib()
    out = []
    for cfg in range(L.hrh_num_cfgs()):
        g, cu = C.c_int(0), C.c_int(0)
        L.hrh_cfg(cfg, C.byref(g), C.byref(cu))
        if L.hrh_eligible_cfg(F32, cfg, 1, 0):
            out.append((g.value, cu.value))
    return out


def shapes():
    """(G, CU, nchunks): every eligible configuration at one span, the widest at one and two spans."""
    return [(g, cu, g * cu) for g, cu in eligible_cfgs()] + [(64, 4, 512)]


def test_eligible_configurations_are_the_even_cu_ones():
    assert eligible_cfgs() == [(8, 2), (8, 4), (16, 4), (32, 4), (64, 4)]
    L = lib()
    for cfg in range(L.hrh_num_cfgs()):
        assert not L.hrh_eligible_cfg(F32, cfg, 0, 0)  # rows that are not whole spans
        assert not L.hrh_eligible_cfg(F32, cfg, 1, 1)  # split rows
        for other in ("uint8", "int8", "float16"):
            assert not L.hrh_eligible_cfg(DTYPE_ORD[other], cfg, 1, 0)


@pytest.mark.parametrize("G,CU,nchunks", shapes())
def test_chunk_to_unit_map_is_a_bijection_onto_the_mirror_row(G, CU, nchunks):
    L = lib()
    unit = np.zeros(nchunks, dtype=np.uint32)
    half = np.zeros(nchunks, dtype=np.uint32)
    L.hrh_unit_map(nchunks, G, CU, unit.ctypes.data, half.ctypes.data)
    # byte offsets of the chunks' 8-byte halves: every 8-byte slot of the row_bytes / 2 = nchunks * 8 bytes exactly once
    offsets = np.sort(unit.astype(np.int64) * 16 + half.astype(np.int64) * 8)
    assert np.array_equal(offsets, np.arange(nchunks, dtype=np.int64) * 8)
    for c in range(nchunks):  # the inverse map of the conversion kernel, and the neighbour inside a unit
        assert L.hrh_first_chunk_of_unit(int(unit[c]), G, CU) + int(half[c]) * G == c
    # lane g's j-th load of a span covers G contiguous units: unit = c0 / 2 + j * G + g
    for c in range(nchunks):
        c0, r = c // (G * CU) * (G * CU), c % (G * CU)
        assert unit[c] == c0 // 2 + (r // G // 2) * G + r % G and half[c] == (r // G) % 2


def _rows_and_queries(nchunks, n_rows, seed):
    rng = np.random.default_rng(seed)
    rows = rng.normal(size=(n_rows, nchunks * 4)).astype(np.float16).astype(np.float32)
    rows[0, :4] = [65504.0, -65504.0, 2.0 ** -24, -0.0]
    queries = rng.normal(size=(n_rows, nchunks * 4)).astype(np.float32)  # not representable in binary16
    assert not np.array_equal(queries, queries.astype(np.float16).astype(np.float32))
    return rows, queries


def _mirror(rows, nchunks, G, CU):
    L = lib()
    out = np.zeros((rows.shape[0], nchunks * 4), dtype=np.uint16)
    for i in range(rows.shape[0]):
        assert L.hrh_convert_row(rows[i].ctypes.data, out[i].ctypes.data, nchunks, G, CU) == 1
    return out


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("G,CU,nchunks", shapes())
def test_emulated_lanes_agree_bit_for_bit_and_tell_orders_apart(G, CU, nchunks, metric):
    L = lib()
    rows, queries = _rows_and_queries(nchunks, 24, seed=G * 100 + nchunks + metric)
    mirror = _mirror(rows, nchunks, G, CU)
    want = np.array([L.hrh_dist_f32(queries[i].ctypes.data, rows[i].ctypes.data, nchunks, G, CU, metric) for i in range(len(rows))],
                    dtype=np.float32)
    got = np.array([L.hrh_dist_half(queries[i].ctypes.data, mirror[i].ctypes.data, nchunks, G, CU, metric, 0) for i in range(len(rows))],
                   dtype=np.float32)
    assert not np.isnan(want).any()
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    # the plain numpy value is close (the emulation computes a distance at all)
    ref = ((queries.astype(np.float64) - rows) ** 2).sum(1) if metric == L2 else 1.0 - (queries.astype(np.float64) * rows).sum(1)
    assert np.allclose(want, ref, rtol=1e-4, atol=1e-2 * np.abs(ref).max())
    # the two chunks of every unit swapped: these inputs can tell the orders apart
    swapped = np.array([L.hrh_dist_half(queries[i].ctypes.data, mirror[i].ctypes.data, nchunks, G, CU, metric, 1) for i in range(len(rows))],
                       dtype=np.float32)
    assert not np.array_equal(want.view(np.uint32), swapped.view(np.uint32))


def _round_trip(values: np.ndarray):
    L = lib()
    bits = np.ascontiguousarray(values).view(np.uint32).reshape(-1)
    back = np.zeros_like(bits)
    ok = np.zeros(bits.size, dtype=np.uint8)
    L.hrh_round_trip(bits.ctypes.data, bits.size, back.ctypes.data, ok.ctypes.data)
    return bits, back, ok.astype(bool)


def _numpy_lossless(values: np.ndarray):
    with np.errstate(over="ignore", invalid="ignore"):
        return values.astype(np.float16).astype(np.float32).view(np.uint32) == values.view(np.uint32)


def test_round_trip_predicate_matches_numpy():
    named = np.array([0.0, -0.0, 1.0, 255.0, 2048.0, 2049.0, 65504.0, 65520.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1.0 / 3.0,
                      np.inf, np.nan], dtype=np.float32)
    expect = [True, True, True, True, True, False, True, False, True, True, False, False, True, True]
    bits, back, ok = _round_trip(named)
    assert ok.tolist() == expect
    assert _numpy_lossless(named).tolist() == expect
    assert np.array_equal(back[ok], bits[ok])
    # every binary16 value, widened by numpy, is lossless; its neighbours one float32 ulp away are not
    every = np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(np.float32)
    bits, back, ok = _round_trip(every)
    assert ok.all() and np.array_equal(back, bits)
    finite = np.isfinite(every) & (every != 0)
    off = (every.view(np.uint32)[finite] + 1).view(np.float32)
    assert not _round_trip(off)[2].any()
    # random bit patterns (NaNs, infinities, subnormals included)
    rnd = np.random.default_rng(7).integers(0, 1 << 32, size=200_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert np.array_equal(_round_trip(rnd)[2], _numpy_lossless(rnd))


def test_convert_row_places_values_by_the_map_and_flags_lossy_rows():
    L = lib()
    G, CU, nchunks = 8, 4, 32
    rows, _ = _rows_and_queries(nchunks, 2, seed=3)
    mirror = _mirror(rows, nchunks, G, CU)
    unit = np.zeros(nchunks, dtype=np.uint32)
    half = np.zeros(nchunks, dtype=np.uint32)
    L.hrh_unit_map(nchunks, G, CU, unit.ctypes.data, half.ctypes.data)
    h = rows.astype(np.float16).view(np.uint16)
    for c in range(nchunks):
        at = int(unit[c]) * 8 + int(half[c]) * 4
        assert np.array_equal(mirror[:, at:at + 4], h[:, 4 * c:4 * c + 4])
    bad = rows[0].copy()
    bad[77] = 1.0 / 3.0
    out = np.zeros(nchunks * 4, dtype=np.uint16)
    assert L.hrh_convert_row(bad.ctypes.data, out.ctypes.data, nchunks, G, CU) == 0


@pytest.mark.parametrize("dtype,dim,want", [("float32", 128, True), ("float32", 120, True), ("float32", 64, True), ("float32", 256, True),
                                            ("float32", 512, True), ("float32", 1024, True), ("float32", 2048, True),
                                            ("float32", 100, False), ("float32", 768, False), ("float32", 32, False),
                                            ("uint8", 128, False), ("int8", 128, False), ("float16", 128, False), ("float16", 256, False),
                                            ("uint8", 512, False)])
def test_which_geometries_have_a_mirror(dtype, dim, want):
    assert bool(lib().hrh_eligible(DTYPE_ORD[dtype], dim, 100_000)) == want


def test_harness_runs_clean_under_the_host_sanitizers():
    """The same harness as a stand-alone program with AddressSanitizer and UBSan: maps, conversion and both emulations stay
    inside their arrays."""
    exe = os.path.join(tmpdir(), "half_rows_harness_asan")
    subprocess.check_call(FLAGS + ["-g", "-DHRH_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "half_rows_harness OK" in run.stdout
