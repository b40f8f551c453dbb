"""Filtered search without a GPU: the CPU restatement (tests/filtered_search_ref.cpp) against the oracle, the label-bitmap
packing of the Python surface, argument validation of the C ABI, and the new entry points' declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filtered_ref
from flatnav_amd import datasets as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNV_ERR_INVALID = 1  # include/flatnav_hip.h


def _index(oracle_mod, metric, dtype, X, M=16, efc=100, labels=None):
    o = oracle_mod.OracleIndex.create(metric, X.shape[1], X.shape[0], M, dtype)
    o.add(X, efc, labels=labels)
    return o


def _data(kind, n, nq, dim, metric):
    if kind == "sift_f32":
        X, Q = ds.sift_like(n, nq, dim)
        return "float32", X, Q
    if kind == "u8":
        X, Q = ds.sift_like(n, nq, dim)
        return "uint8", X.astype(np.uint8), Q.astype(np.uint8)
    if kind == "i8":
        X, Q = ds.sift_like(n, nq, dim)
        return "int8", (X - 64).clip(-128, 127).astype(np.int8), (Q - 64).clip(-128, 127).astype(np.int8)
    if kind == "ties":  # a handful of values per coordinate: equal distances everywhere
        rng = np.random.default_rng(5)
        lo, hi = (-2, 3) if metric == "ip" else (0, 3)
        return "int8", rng.integers(lo, hi, (n, dim)).astype(np.int8), rng.integers(lo, hi, (nq, dim)).astype(np.int8)
    if kind == "float":
        X, Q = ds.randn(n, nq, dim, seed=11, normalize=metric == "ip")
        return "float32", X, Q
    raise AssertionError(kind)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("kind", ["sift_f32", "u8", "i8", "ties", "float"])
def test_restatement_all_allowed_equals_oracle(oracle_mod, kind, metric):
    dtype, X, Q = _data(kind, 3000, 60, 40, metric)
    o = _index(oracle_mod, metric, dtype, X)
    for K, ef in ((1, 16), (10, 50), (100, 100)):
        od, ol, ost = o.search(Q, K, ef, stats=True)
        rd, rl, rst = filtered_ref.search_oracle_index(o, Q, K, ef, np.ones(X.shape[0], bool))
        assert np.array_equal(rl, ol), (kind, metric, K)
        assert np.array_equal(rd.view(np.uint32), od.view(np.uint32)), (kind, metric, K)
        for key in ("count", "n_dist", "n_hops"):
            assert np.array_equal(rst[key], ost[key].astype(rst[key].dtype)), (kind, metric, K, key)


def test_restatement_filter_follows_labels_not_node_ids(oracle_mod):
    # labels given in reverse order: allowing label L must allow node n - 1 - L
    dtype, X, Q = _data("u8", 2000, 30, 32, "l2")
    n = X.shape[0]
    o = _index(oracle_mod, "l2", dtype, X, labels=np.arange(n)[::-1].astype(np.int32))
    rng = np.random.default_rng(3)
    allowed = rng.choice(n, n // 10, replace=False)
    rd, rl, rst = filtered_ref.search_oracle_index(o, Q, 10, 64, allowed)
    assert np.isin(rl[rl >= 0], allowed).all()
    assert (rst["count"] == 10).all()
    # a filter that is a superset by labels beyond n_bits changes nothing
    rd2, rl2, _ = filtered_ref.search_oracle_index(o, Q, 10, 64, np.concatenate([allowed, [n + 5, n + 100]]))
    assert np.array_equal(rl, rl2) and np.array_equal(rd.view(np.uint32), rd2.view(np.uint32))


def test_restatement_invariants(oracle_mod):
    dtype, X, Q = _data("sift_f32", 3000, 40, 32, "l2")
    o = _index(oracle_mod, "l2", dtype, X)
    n = X.shape[0]
    rng = np.random.default_rng(9)
    for frac in (0.5, 0.1, 0.01):
        allowed = rng.choice(n, max(1, int(frac * n)), replace=False)
        rd, rl, rst = filtered_ref.search_oracle_index(o, Q, 10, 100, allowed)
        for q in range(Q.shape[0]):
            c = int(rst["count"][q])
            assert np.isin(rl[q, :c], allowed).all() and len(set(rl[q, :c])) == c
            assert (np.diff(rd[q, :c]) >= 0).all()
            assert (rl[q, c:] == -1).all() and np.isinf(rd[q, c:]).all()
    three = [5, 1700, 2999]
    rd, rl, rst = filtered_ref.search_oracle_index(o, Q, 10, 3000, three)  # a beam over the whole graph finds all three
    assert (rst["count"] == 3).all() and (np.sort(rl[:, :3], axis=1) == sorted(three)).all() and (rl[:, 3:] == -1).all()
    rd, rl, rst = filtered_ref.search_oracle_index(o, Q, 10, 100, np.zeros(0, np.int64))
    assert (rst["count"] == 0).all() and (rl == -1).all() and np.isinf(rd).all()


# ---- packing of `allowed` (flatnav_amd.hip.pack_allowed, pure numpy) -------------------------------------------------
def test_pack_allowed_mask_and_labels_agree():
    from flatnav_amd.hip import pack_allowed

    mask = np.zeros(21, bool)
    mask[[0, 3, 8, 20]] = True
    bits, n_bits = pack_allowed(mask)
    assert n_bits == 21 and bits.tolist() == [0b00001001, 0b00000001, 0b00010000]
    bits2, n2 = pack_allowed([20, 8, 3, 0, 3, 20])  # order and duplicates ignored
    assert n2 == 21 and np.array_equal(bits, bits2)
    bits3, n3 = pack_allowed(np.array([20, 8, 3, 0], np.uint32))
    assert n3 == 21 and np.array_equal(bits, bits3)
    assert np.array_equal(np.packbits(mask, bitorder="little"), bits)


def test_pack_allowed_edge_cases():
    from flatnav_amd.hip import pack_allowed

    assert pack_allowed(np.zeros(0, np.int64))[1] == 0
    assert pack_allowed([])[1] == 0
    assert pack_allowed(np.zeros(0, bool))[1] == 0
    with pytest.raises(ValueError):
        pack_allowed([3, -1])
    with pytest.raises(ValueError):
        pack_allowed(np.ones((2, 2), bool))
    with pytest.raises(ValueError):
        pack_allowed([0.5, 1.0])
    with pytest.raises(ValueError):
        pack_allowed([1 << 31])


# ---- the C ABI: declarations and argument validation (no GPU: every call below fails before touching the device) ------
def test_filtered_symbols_declared_and_bound():
    from flatnav_amd import hip

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flatnav_hip.h")).read(), flags=re.S)
    for name in ("fnv_search_batch_filtered", "fnv_search_batch_filtered_device"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hip.C_ABI_SYMBOLS, name


@pytest.fixture(scope="module")
def cabi():
    from flatnav_amd import build

    L = C.CDLL(build.build())
    L.fnv_last_error.restype = C.c_char_p
    L.fnv_search_batch_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_uint64] + [C.c_void_p] * 5
    L.fnv_search_batch_filtered_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_uint64] + [C.c_void_p] * 6
    return L


def test_filtered_argument_validation(cabi):
    q = np.zeros(8, np.float32)
    out = np.zeros(8, np.float32)
    bits = np.zeros(4, np.uint8)
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    host = cabi.fnv_search_batch_filtered
    dev = cabi.fnv_search_batch_filtered_device
    assert host(fake, q.ctypes.data, 1, 1, 1, 1, None, 5, out.ctypes.data, out.ctypes.data, None, None, None) == FNV_ERR_INVALID
    assert b"allowed_bits" in cabi.fnv_last_error()
    assert host(fake, q.ctypes.data, 1, 1, 1, 1, bits.ctypes.data, (1 << 31) + 1, out.ctypes.data, out.ctypes.data, None, None,
                None) == FNV_ERR_INVALID
    assert b"n_bits" in cabi.fnv_last_error()
    assert host(None, q.ctypes.data, 1, 1, 1, 1, bits.ctypes.data, 8, out.ctypes.data, out.ctypes.data, None, None,
                None) == FNV_ERR_INVALID
    assert dev(None, q.ctypes.data, 1, 1, 1, 1, bits.ctypes.data, 8, out.ctypes.data, out.ctypes.data, None, None, None,
               None) == FNV_ERR_INVALID
    assert dev(fake, q.ctypes.data, 1, 1, 1, 1, None, 3, out.ctypes.data, out.ctypes.data, None, None, None, None) == FNV_ERR_INVALID
    assert dev(fake, q.ctypes.data, 1, 1, 1, 1, bits.ctypes.data, 1 << 40, out.ctypes.data, out.ctypes.data, None, None, None,
               None) == FNV_ERR_INVALID
