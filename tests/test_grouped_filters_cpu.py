"""Grouped filters (fnv_search_batch_*_grouped: one allowed set per query) without a GPU.  tests/group_tiles_harness.cpp is
compiled with g++ over flatnav_amd/csrc/scan_select.hpp and loaded with ctypes: the row a query_filter value selects, the bound
on the data-dependent tile count that the host launches, and the tile descriptors -- stated sequentially and as the device
computes them, one binary search per descriptor.  Then pack_filters against numpy.packbits, the new names in the header, the
binding and the classes, and the argument checks that need no device."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "group_tiles_harness.cpp")
HEADER = os.path.join(ROOT, "include", "flatnav_hip.h")
NAMES = ("fnv_search_batch_filtered_grouped", "fnv_search_batch_filtered_grouped_device",
         "fnv_search_batch_exhaustive_grouped", "fnv_search_batch_exhaustive_grouped_device")
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="flatnav_group_tiles_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libgroup_tiles_harness.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.gth_filter_row.argtypes = [C.c_int32, C.c_uint32]
        L.gth_filter_row.restype = C.c_uint32
        L.gth_tile_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.gth_tile_bound.restype = C.c_uint64
        L.gth_queue_ids.restype = C.c_uint32
        L.gth_layout.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
        L.gth_layout.restype = C.c_uint32
        L.gth_by_search.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
        _lib = L
    return _lib


def test_row_of_a_query_filter_value():
    L = lib()
    for F in (0, 1, 5, 1000):
        assert L.gth_filter_row(-1, F) == F  # no filter: the row of every live node
        for v in range(F if F < 10 else 10):
            assert L.gth_filter_row(v, F) == v
        if F:
            assert L.gth_filter_row(F - 1, F) == F - 1
        for v in (F, F + 1, -2, -7, 2**31 - 1, -2**31):  # everything else: the empty row, never outside the table
            assert L.gth_filter_row(v, F) == F + 1, (v, F)


def _layouts(counts, tile):
    L = lib()
    counts = np.ascontiguousarray(counts, np.uint32)
    nq, rows = int(counts.sum()), counts.size
    bound = int(L.gth_tile_bound(nq, rows, tile))
    seq = np.zeros((bound, 3), np.uint32)
    real = L.gth_layout(counts.ctypes.data, rows, tile, seq.ctypes.data, bound)
    dev = np.full((bound, 3), 0xFFFFFFFF, np.uint32)
    L.gth_by_search(counts.ctypes.data, rows, tile, dev.ctypes.data, bound)
    return nq, bound, real, seq, dev


def _check(counts, tile):
    counts = np.asarray(counts)
    nq, bound, real, seq, dev = _layouts(counts, tile)
    want_tiles = int(((counts + tile - 1) // tile).sum())
    assert real == want_tiles and want_tiles <= bound <= max(nq, 1), (counts, tile, real, bound)
    assert bound <= -(-nq // tile) + min(counts.size, nq)
    assert np.array_equal(seq, dev), (counts, tile)  # the device's rule is the sequential statement
    assert (seq[real:, 1] == 0).all() and (seq[:real, 1] >= 1).all() and (seq[:, 1] <= tile).all()
    # every slot of the permutation exactly once, and a tile never leaves its row's slots
    start = np.concatenate([[0], np.cumsum(counts)])
    seen = np.zeros(nq, np.int64)
    for first, count, row in seq[:real]:
        seen[first:first + count] += 1
        assert start[row] <= first and first + count <= start[row + 1], (counts, tile, first, count, row)
    assert (seen == 1).all()


@pytest.mark.parametrize("tile", [1, 2, 31, 32])
def test_tile_bound_and_descriptors(tile):
    rng = np.random.default_rng(tile)
    for case in range(300):
        rows = int(rng.integers(2, 60))
        counts = rng.integers(0, 100, rows) * (rng.random(rows) < 0.6)
        if counts.sum() == 0:
            counts[int(rng.integers(rows))] = 1
        _check(counts, tile)
    for nq in (1, 3, 64, 257):
        _check(np.concatenate([np.ones(nq, np.int64), [0, 0]]), tile)  # every query in its own group
        _check(np.array([0, nq, 0]), tile)                             # all queries in one
        _check(np.array([0] * 7 + [nq]), tile)                         # ... in the last row (the empty filter's)
    _check(np.array([1, 31, 32, 33, 64, 96]), tile)


def test_queue_holds_a_batch_and_a_word():
    # the widest batch of the scan is 24 rows (8-lane groups, three passes): leftovers + one 32-node word must fit, and the
    # queue plus a 19 KB tile is sixteen 1280-byte LDS granules -- eight blocks per CU
    q = lib().gth_queue_ids()
    assert q >= 23 + 32 and q * 4 + 19 * 1024 <= 16 * 1280


def test_pack_filters_against_packbits():
    from flatnav_amd import hip

    rng = np.random.default_rng(5)
    filters = [rng.random(77) < 0.5, np.array([3, 200, 3, 9]), np.zeros(0, np.int64), np.array([0]), np.ones(13, bool), []]
    table, n_bits = hip.pack_filters(filters)
    assert n_bits == 201 and table.shape == (6, 26) and table.dtype == np.uint8 and table.flags.c_contiguous
    for f, one in enumerate(filters):
        mask = np.zeros(n_bits, bool)
        one = np.asarray(one)
        if one.dtype == np.bool_:
            mask[: one.size] = one
        elif one.size:
            mask[one] = True
        assert np.array_equal(table[f], np.packbits(mask, bitorder="little")), f
        bits, own = hip.pack_allowed(one)  # the row is the filter's own bitmap, zero beyond it
        assert np.array_equal(table[f, : bits.size], bits) and not table[f, bits.size:].any()
    mask2d = rng.random((4, 50)) < 0.3
    table, n_bits = hip.pack_filters(mask2d)
    assert n_bits == 50 and np.array_equal(table, np.packbits(mask2d, axis=1, bitorder="little"))
    table, n_bits = hip.pack_filters([])
    assert table.shape == (0, 0) and n_bits == 0
    with pytest.raises(ValueError):
        hip.pack_filters([np.array([1, -2])])
    with pytest.raises(ValueError):
        hip.pack_filters(np.zeros((2, 3), np.int32))


def test_header_binding_and_classes_agree_on_the_new_surface():
    import flatnav_amd
    from flatnav_amd import hip

    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fnv_\w+)\s*\(", text, re.M))
    for name in NAMES:
        assert name in declared and name in hip.C_ABI_SYMBOLS, name
    assert declared == set(hip.C_ABI_SYMBOLS) and len(hip.C_ABI_SYMBOLS) == 41
    assert "filter_stride_bytes" in text and "query_filter" in text
    for method in ("search_filtered_grouped", "search_exhaustive_grouped", "search_device_filtered_grouped",
                   "search_device_exhaustive_grouped"):
        assert callable(getattr(hip.DeviceIndex, method, None)), method
    classes = [c for c in vars(flatnav_amd._core.index).values() if isinstance(c, type) and hasattr(c, "search_exhaustive")]
    assert len(classes) == 8
    for c in classes:
        assert hasattr(c, "search_filtered_grouped") and hasattr(c, "search_exhaustive_grouped"), c


def test_query_filter_of_the_python_surface():
    from flatnav_amd import hip

    assert hip._query_filter([0, -1, 2], 3, 3).dtype == np.int32
    for bad, nq in (([0, 3], 2), ([-2, 0], 2), ([0], 2), ([[0, 1]], 2), ([0.5, 1.0], 2)):
        with pytest.raises(ValueError):
            hip._query_filter(bad, nq, 3)


def test_argument_validation_needs_no_device():
    from flatnav_amd import hip

    L = hip.lib()
    q = (C.c_float * 4)()
    d, l = (C.c_float * 4)(), (C.c_int32 * 4)()
    qf = (C.c_int32 * 1)(0)
    table = (C.c_uint8 * 8)()
    host_f = lambda ix, filters, F, stride, n_bits, qfp: L.fnv_search_batch_filtered_grouped(
        ix, q, 1, 1, 16, 1, filters, F, stride, n_bits, qfp, d, l, None, None, None)
    host_e = lambda ix, K, filters, F, stride, n_bits, qfp: L.fnv_search_batch_exhaustive_grouped(
        ix, q, 1, K, filters, F, stride, n_bits, qfp, d, l, None, None)
    dev_f = lambda ix, filters, F, stride, n_bits, qfp: L.fnv_search_batch_filtered_grouped_device(
        ix, q, 1, 1, 16, 1, filters, F, stride, n_bits, qfp, d, l, None, None, None, None)
    dev_e = lambda ix, K, filters, F, stride, n_bits, qfp: L.fnv_search_batch_exhaustive_grouped_device(
        ix, q, 1, K, filters, F, stride, n_bits, qfp, d, l, None, None, None)
    for call in (lambda *a: host_f(None, *a), lambda *a: dev_f(None, *a), lambda *a: host_e(None, 1, *a),
                 lambda *a: dev_e(None, 1, *a)):
        assert call(table, 1, 8, 64, qf) == hip.FNV_ERR_INVALID  # a null handle
        assert b"index is null" in L.fnv_last_error()
    fake = C.c_void_p(1)  # never dereferenced: these are refused before the handle is looked at
    for call in (lambda *a: host_f(fake, *a), lambda *a: dev_f(fake, *a), lambda *a: host_e(fake, 1, *a),
                 lambda *a: dev_e(fake, 1, *a)):
        assert call(table, 1, 8, 2**31 + 1, qf) == hip.FNV_ERR_INVALID
        assert b"n_bits" in L.fnv_last_error()
        assert call(table, 1, 7, 64, qf) == hip.FNV_ERR_INVALID
        assert b"filter_stride_bytes" in L.fnv_last_error()
        assert call(None, 1, 8, 64, qf) == hip.FNV_ERR_INVALID
        assert b"filters is null" in L.fnv_last_error()
        assert call(table, 1, 8, 64, None) == hip.FNV_ERR_INVALID
        assert b"query_filter is null" in L.fnv_last_error()
        assert call(table, 2**31, 8, 64, qf) == hip.FNV_ERR_INVALID
        assert b"n_filters" in L.fnv_last_error()
    for K in (0, 1025):
        assert host_e(fake, K, table, 1, 8, 64, qf) == hip.FNV_ERR_INVALID
        assert dev_e(fake, K, table, 1, 8, 64, qf) == hip.FNV_ERR_INVALID
    # the host entry points read query_filter before anything is launched and name the first offender
    for bad in (1, -2, -7):
        for call in (lambda p: host_f(fake, table, 1, 8, 64, p), lambda p: host_e(fake, 1, table, 1, 8, 64, p)):
            assert call((C.c_int32 * 1)(bad)) == hip.FNV_ERR_INVALID
            assert b"query_filter[0] = %d" % bad in L.fnv_last_error()
