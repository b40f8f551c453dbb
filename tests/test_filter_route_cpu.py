"""Filter routing ("filter_scan_max" / "filter_scan_on_overflow": graph search or exhaustive scan, per query, inside one
filtered call) without a GPU.  tests/filter_route_harness.cpp is compiled with g++ over flatnav_amd/csrc/scan_select.hpp and
loaded with ctypes: the route word of a query from its filter row's popcount, and the grouping of the routed queries alone
into the scan stage's tiles.  Then the header, the symbol count and the classes."""
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
SRC = os.path.join(ROOT, "tests", "filter_route_harness.cpp")
HEADER = os.path.join(ROOT, "include", "flatnav_hip.h")
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="flatnav_filter_route_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libfilter_route_harness.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.frh_route_by_count.argtypes = [C.c_uint32, C.c_uint64]
        L.frh_route_by_count.restype = C.c_uint32
        for name in ("frh_route_graph", "frh_route_scan", "frh_route_overflow", "frh_no_row"):
            getattr(L, name).restype = C.c_uint32
        L.frh_tile_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.frh_tile_bound.restype = C.c_uint64
        L.frh_route_at_launch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
        L.frh_route_at_launch.restype = None
        L.frh_group_routed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint32]
        L.frh_group_routed.restype = C.c_uint32
        _lib = L
    return _lib


def test_route_words_are_distinct_and_graph_is_zero():
    L = lib()
    assert L.frh_route_graph() == 0  # (a route buffer that was never written must not read as "routed": the kernel tests != 0)
    assert len({L.frh_route_graph(), L.frh_route_scan(), L.frh_route_overflow()}) == 3
    assert L.frh_no_row() == 0xFFFFFFFF


@pytest.mark.parametrize("threshold", [1, 2, 60, 600, 2**31, 2**40])
def test_route_decision_around_the_threshold(threshold):
    L = lib()
    scan, graph = L.frh_route_scan(), L.frh_route_graph()
    for count, want in ((threshold - 1, scan), (threshold, scan), (threshold + 1, graph)):
        if 0 <= count < 2**32:
            assert L.frh_route_by_count(count, threshold) == want, (count, threshold)
    assert L.frh_route_by_count(0, threshold) == scan  # the empty row always scans once the rule is on


def test_threshold_zero_is_off():
    L = lib()
    for count in (0, 1, 60, 2**32 - 1):
        assert L.frh_route_by_count(count, 0) == L.frh_route_graph(), count


def _route_at_launch(qf, n_filters, row_count, scan_max):
    L = lib()
    nq = len(qf) if qf is not None else 5
    qf_arr = None if qf is None else np.ascontiguousarray(qf, np.int32)
    rc = np.ascontiguousarray(row_count, np.uint32)
    assert rc.size == n_filters + 2
    route = np.full(nq, 77, np.uint32)
    L.frh_route_at_launch(None if qf_arr is None else qf_arr.ctypes.data, nq, n_filters, rc.ctypes.data, scan_max, route.ctypes.data)
    return route


def test_the_unfiltered_row_and_the_empty_row():
    # six filters allowing 0, 1, 5, 60, 300, 600 of 600 live nodes; row 6 = every live node (-1), row 7 = none (anything else)
    row_count = [0, 1, 5, 60, 300, 600, 600, 0]
    qf = np.array([0, 1, 2, 3, 4, 5, -1, 6, 7, -2, -2**31, 2**31 - 1], np.int32)
    counts = np.array([0, 1, 5, 60, 300, 600, 600, 0, 0, 0, 0, 0])
    for scan_max in (0, 1, 59, 60, 61, 599, 600, 10**6):
        want = ((counts <= scan_max) & (scan_max > 0)).astype(np.uint32)
        assert np.array_equal(_route_at_launch(qf, 6, row_count, scan_max), want), scan_max
    # a -1 row counts n_live: it scans only at a threshold of n_live or more; out-of-range values count 0
    assert _route_at_launch([-1], 6, row_count, 599)[0] == 0 and _route_at_launch([-1], 6, row_count, 600)[0] == 1
    assert _route_at_launch([99], 6, row_count, 1)[0] == 1 and _route_at_launch([99], 6, row_count, 0)[0] == 0
    # the single-filter call: no query_filter at all, a table of one -- every query reads row 0
    for count, scan_max, want in ((6, 5, 0), (6, 6, 1), (0, 1, 1), (6, 0, 0)):
        assert (_route_at_launch(None, 1, [count, 600, 0], scan_max) == want).all()


def _group(qf, route, n_filters, tile):
    """-> (query_row, perm, tiles[real], bound, real) of the routed subset."""
    L = lib()
    nq = len(route)
    rows = n_filters + 2
    bound = int(L.frh_tile_bound(nq, rows, tile))
    qf_arr = None if qf is None else np.ascontiguousarray(qf, np.int32)
    route = np.ascontiguousarray(route, np.uint32)
    query_row = np.zeros(nq, np.uint32)
    perm = np.zeros(nq, np.uint32)
    tiles = np.full((bound, 3), 0xFFFFFFFF, np.uint32)
    real = L.frh_group_routed(None if qf_arr is None else qf_arr.ctypes.data, route.ctypes.data, nq, n_filters, tile,
                              query_row.ctypes.data, perm.ctypes.data, tiles.ctypes.data, bound)
    return query_row, perm, tiles, bound, real


def _check_group(qf, route, n_filters, tile):
    route = np.asarray(route, np.uint32)
    nq = len(route)
    query_row, perm, tiles, bound, real = _group(qf, route, n_filters, tile)
    routed = np.flatnonzero(route != 0)
    values = np.zeros(nq, np.int64) if qf is None else np.asarray(qf, np.int64)
    want_row = np.where(values == -1, n_filters, np.where((values >= 0) & (values < n_filters), values, n_filters + 1))
    assert np.array_equal(query_row[routed], want_row[routed])
    assert (query_row[route == 0] == 0xFFFFFFFF).all()
    # the tile count stays within the bound the host launches, and the descriptors past the real ones are empty
    assert real <= bound <= max(nq, 1), (real, bound, nq)
    assert real == sum(-(-int(c) // tile) for c in np.bincount(want_row[routed], minlength=n_filters + 2))
    assert (tiles[real:, 1] == 0).all()
    seen = np.zeros(nq, np.int64)
    for first, count, row in tiles[:real]:
        assert 1 <= count <= tile
        members = perm[first:first + count]
        assert (members < nq).all()
        seen[members] += 1
        assert (query_row[members] == row).all(), (first, count, row)  # one filter row per tile
    assert (seen[routed] == 1).all()       # every routed query in exactly one tile
    assert (seen[route == 0] == 0).all()   # no unrouted query in any
    assert (perm[len(routed):] == 0xFFFFFFFF).all()  # the permutation holds the routed queries and nothing else


@pytest.mark.parametrize("tile", [1, 2, 7, 32])
def test_subset_grouping_over_random_route_vectors(tile):
    rng = np.random.default_rng(100 + tile)
    for case in range(300):
        n_filters = int(rng.integers(0, 12))
        nq = int(rng.integers(1, 200))
        qf = rng.integers(-2, n_filters + 2, nq).astype(np.int32)  # out-of-range values on both sides included
        route = rng.choice([0, 1, 2], nq, p=[0.5, 0.3, 0.2])
        _check_group(qf, route, n_filters, tile)
    for nq in (1, tile, tile + 1, 97):
        qf = rng.integers(-1, 4, nq).astype(np.int32)
        _check_group(qf, np.zeros(nq), 4, tile)            # none routed: no tile at all
        _check_group(qf, np.ones(nq), 4, tile)             # all routed
        _check_group(qf, np.full(nq, 2), 4, tile)          # ... all by overflow
        one = np.zeros(nq)
        one[nq // 2] = 1
        _check_group(qf, one, 4, tile)                     # exactly one
        _check_group(None, rng.integers(0, 3, nq), 1, tile)  # the single-filter call: row 0 for every query
        _check_group(None, np.ones(nq), 1, tile)
    _check_group(np.array([3], np.int32), [1], 6, tile)    # nq = 1
    _check_group(np.array([3], np.int32), [0], 6, tile)


def test_header_documents_the_options_and_keeps_its_symbols():
    from flatnav_amd import hip

    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fnv_\w+)\s*\(", text, re.M))
    assert declared == set(hip.C_ABI_SYMBOLS) and len(declared) == 41  # two options, no new entry point
    for option in ('"filter_scan_max"', '"filter_scan_on_overflow"'):
        assert text.count(option) >= 2, option  # in the option list and in the section on routing
    options = text[text.index("Tuning / test knobs"):text.index("int fnv_set_option")]
    assert '"filter_scan_max"' in options and '"filter_scan_on_overflow"' in options
    not_covered = [line for line in text.splitlines() if "Not covered:" in line]
    assert not_covered and not any("routing" in line for line in not_covered)
    assert "out_nhops[q] = 0" in text


def test_the_eight_classes_expose_set_filter_routing():
    import flatnav_amd

    classes = [c for c in vars(flatnav_amd._core.index).values() if isinstance(c, type) and hasattr(c, "search_exhaustive")]
    assert len(classes) == 8
    for c in classes:
        assert callable(getattr(c, "set_filter_routing", None)), c
    index = flatnav_amd.index.create("l2", 8, 16, 4)
    index.set_filter_routing()  # the defaults: off; no device mirror exists yet, so nothing is uploaded
    index.set_filter_routing(scan_max_allowed=10, scan_on_overflow=True)
    with pytest.raises(ValueError):
        index.set_filter_routing(scan_max_allowed=-1)
