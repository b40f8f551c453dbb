"""The exhaustive search's selection rules (flatnav_amd/csrc/scan_select.hpp) on the CPU: tests/scan_select_harness.cpp is
compiled with g++ and loaded with ctypes.  Checked here, without a GPU: the 64-bit key orders (distance, node id) pairs as
np.lexsort does -- NaN after +inf, NaNs among themselves by id, -0 = +0 -- and round-trips; the rank merge of two sorted,
padded lists writes every position exactly once and equals the top K of their union; folding S lists does too; the public
header, the ctypes binding and DeviceIndex agree on the new surface."""
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
SRC = os.path.join(ROOT, "tests", "scan_select_harness.cpp")
HEADER = os.path.join(ROOT, "include", "flatnav_hip.h")
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="flatnav_scan_select_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libscan_select_harness.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.ssh_pad.restype = C.c_uint64
        L.ssh_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ssh_unkeys.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.ssh_less.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ssh_lower_bound.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        L.ssh_lower_bound.restype = C.c_uint32
        L.ssh_upper_bound.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        L.ssh_upper_bound.restype = C.c_uint32
        L.ssh_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.ssh_merge_many.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib = L
    return _lib


def keys_of(dist, nodes) -> np.ndarray:
    dist = np.ascontiguousarray(dist, np.float32)
    nodes = np.ascontiguousarray(nodes, np.uint32)
    out = np.empty(dist.size, np.uint64)
    lib().ssh_keys(dist.ctypes.data, nodes.ctypes.data, dist.size, out.ctypes.data)
    return out


SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 2.0, 3.0, np.inf, -np.inf, np.nan, 3e38, 1e-45, -1e-45, 16777216.0], np.float32)


def random_pairs(rng, n, id_range):
    """n (distance, node id) pairs with distinct ids: few distinct distances (heavy ties), NaNs (several payloads), infs."""
    d = rng.choice(SPECIALS, n).astype(np.float32)
    some = rng.random(n) < 0.3
    d[some] = rng.integers(-3, 4, int(some.sum())).astype(np.float32)
    weird = rng.random(n) < 0.05  # NaNs with other payloads and signs: all rank the same
    bits = d.view(np.uint32).copy()
    bits[weird] = rng.choice(np.array([0x7FC00001, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32), int(weird.sum()))
    d = bits.view(np.float32)
    ids = rng.choice(id_range, n, replace=False).astype(np.uint32)
    return d, ids


def lexsorted(d, ids):
    """Indices in the contract's order: distance ascending, NaN last, ties (and NaNs) by id."""
    return np.lexsort((ids, d))


def padded_sorted_keys(d, ids, K):
    order = lexsorted(d, ids)[:K]
    out = np.full(K, lib().ssh_pad(), np.uint64)
    out[: order.size] = keys_of(d[order], ids[order])
    return out


def test_key_orders_pairs_like_lexsort():
    rng = np.random.default_rng(1)
    L = lib()
    for case in range(10_000):
        n = int(rng.integers(1, 40))
        d, ids = random_pairs(rng, n, 64 if case % 2 else (1 << 32) - 1)
        k = keys_of(d, ids)
        want = lexsorted(d, ids)
        got = np.argsort(k, kind="stable")
        assert np.array_equal(got, want), (case, d, ids)
        assert (k != L.ssh_pad()).all()
        # the compare itself, on every neighbouring pair of the sorted order and its reverse
        a, b = k[want[:-1]], k[want[1:]]
        less = np.empty(a.size, np.uint8)
        L.ssh_less(a.ctypes.data, b.ctypes.data, a.size, less.ctypes.data)
        assert less.all()
        L.ssh_less(b.ctypes.data, a.ctypes.data, a.size, less.ctypes.data)
        assert not less.any()
        # and back: the id as it was, the distance's bits (every NaN as the quiet NaN, a zero as +0)
        bits, nodes = np.empty(n, np.uint32), np.empty(n, np.uint32)
        L.ssh_unkeys(k.ctypes.data, n, bits.ctypes.data, nodes.ctypes.data)
        assert np.array_equal(nodes, ids)
        back = bits.view(np.float32)
        nan = np.isnan(d)
        assert np.array_equal(np.isnan(back), nan) and (bits[nan] == 0x7FC00000).all()
        assert np.array_equal(back[~nan], d[~nan]) and not np.signbit(back[~nan & (d == 0)]).any()
        assert np.array_equal(bits[~nan & (d != 0)], d.view(np.uint32)[~nan & (d != 0)])


def test_merge_of_two_padded_lists_is_the_top_k_of_their_union():
    rng = np.random.default_rng(2)
    L = lib()
    for case in range(10_000):
        K = int(rng.choice([1, 2, 3, 7, 16, 33]))
        na, nb = int(rng.integers(0, 2 * K + 1)), int(rng.integers(0, 2 * K + 1))  # shorter than K: padding; longer: truncated
        d, ids = random_pairs(rng, na + nb, 4 * K + 8)
        a = padded_sorted_keys(d[:na], ids[:na], K)
        b = padded_sorted_keys(d[na:], ids[na:], K)
        out = np.zeros(K, np.uint64)
        written = np.zeros(K, np.uint32)
        L.ssh_merge(a.ctypes.data, b.ctypes.data, K, out.ctypes.data, written.ctypes.data)
        assert (written == 1).all(), (case, written)
        real = np.concatenate([a[a != L.ssh_pad()], b[b != L.ssh_pad()]])
        di, ni = np.empty(real.size, np.uint32), np.empty(real.size, np.uint32)
        L.ssh_unkeys(real.ctypes.data, real.size, di.ctypes.data, ni.ctypes.data)
        want = padded_sorted_keys(di.view(np.float32), ni, K)
        assert np.array_equal(out, want), case
        for key in (a[0], b[K - 1], out[K // 2]):  # the binary searches against numpy's
            assert L.ssh_lower_bound(out.ctypes.data, K, int(key)) == np.searchsorted(out, key, "left")
            assert L.ssh_upper_bound(out.ctypes.data, K, int(key)) == np.searchsorted(out, key, "right")


@pytest.mark.parametrize("S", [1, 2, 7, 64])
def test_merge_of_s_lists_is_the_top_k_of_their_union(S):
    rng = np.random.default_rng(3 + S)
    L = lib()
    for case in range(300):
        K = int(rng.choice([1, 5, 10, 64, 100]))
        n = int(rng.integers(0, 3 * K * max(1, S // 4) + 2))
        d, ids = random_pairs(rng, n, max(n, 1) * 2)
        owner = rng.integers(0, S, n)  # which segment saw each row
        lists = np.stack([padded_sorted_keys(d[owner == s], ids[owner == s], K) for s in range(S)])
        out = np.zeros(K, np.uint64)
        L.ssh_merge_many(np.ascontiguousarray(lists).ctypes.data, S, K, out.ctypes.data)
        assert np.array_equal(out, padded_sorted_keys(d, ids, K)), (S, case)


def test_header_and_binding_agree_on_the_new_symbols():
    from flatnav_amd import hip

    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fnv_\w+)\s*\(", text, re.M))
    for name in ("fnv_search_batch_exhaustive", "fnv_search_batch_exhaustive_device"):
        assert name in declared, name
        assert name in hip.C_ABI_SYMBOLS, name
    assert '"scan_segment_rows"' in text
    assert "node id" in text.lower()  # the tie order is stated
    assert lib().ssh_max_k() == 1024 and "K <= 1024" in text


def test_device_index_has_search_exhaustive():
    from flatnav_amd import hip

    assert callable(getattr(hip.DeviceIndex, "search_exhaustive", None))
    assert callable(getattr(hip.DeviceIndex, "search_device_exhaustive", None))
