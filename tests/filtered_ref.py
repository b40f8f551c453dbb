"""ctypes front-end of tests/filtered_search_ref.cpp, the CPU restatement of the filtered search (test infrastructure).

`search(blob, meta, queries, K, ef, allowed)` runs it over an index blob in the oracle's AoS layout and returns
(dist float32[Q,K], labels int32[Q,K], {"count", "n_dist", "n_hops"}).  `allowed` is anything
flatnav_amd.hip.pack_allowed takes (bool mask by label, or integer labels)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "filtered_search_ref.cpp")
DTYPE_ORD = {"float32": 9, "uint8": 0, "int8": 4}
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="flatnav_filtered_ref_"), "libfiltered_ref.so")
        # no FP contraction, no fast-math: the float32 summation order is the written one (as in the oracle)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.fsr_search.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_uint32,
                                 C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5
        _lib = L
    return _lib


def pack(allowed):
    """(uint8 bitmap, n_bits) exactly as the product packs it (flatnav_amd.hip.pack_allowed, pure numpy)."""
    from flatnav_amd.hip import pack_allowed

    return pack_allowed(allowed)


def search(blob, node_size: int, data_size: int, M: int, n_nodes: int, dtype: str, metric: str, dim: int, queries, K: int,
           ef: int, allowed, num_initializations: int = 100):
    blob = np.ascontiguousarray(np.asarray(blob).view(np.uint8).reshape(-1))
    assert blob.size >= node_size * n_nodes
    q = np.ascontiguousarray(queries, dtype={"float32": np.float32, "uint8": np.uint8, "int8": np.int8}[dtype])
    assert q.ndim == 2 and q.shape[1] == dim
    bits, n_bits = pack(allowed)
    bits = np.ascontiguousarray(bits if bits.size else np.zeros(1, np.uint8))
    nq = q.shape[0]
    d = np.empty((nq, K), np.float32)
    l = np.empty((nq, K), np.int32)
    cnt = np.empty(nq, np.int32)
    nd = np.empty(nq, np.uint64)
    nh = np.empty(nq, np.uint64)
    rc = lib().fsr_search(blob.ctypes.data, node_size, data_size, M, n_nodes, DTYPE_ORD[dtype], 0 if metric == "l2" else 1, dim,
                          q.ctypes.data, nq, K, ef, num_initializations, bits.ctypes.data, n_bits, d.ctypes.data, l.ctypes.data,
                          cnt.ctypes.data, nd.ctypes.data, nh.ctypes.data)
    assert rc == 0, "filtered_search_ref: bad arguments"
    return d, l, {"count": cnt, "n_dist": nd, "n_hops": nh}


def search_oracle_index(ix, queries, K: int, ef: int, allowed, num_initializations: int = 100):
    """search() over an oracle.OracleIndex's own blob."""
    return search(ix.blob(), ix.node_size, ix.data_size, ix.M, ix.cur_nodes, ix.dtype, ix.metric, ix.dim, queries, K, ef,
                  allowed, num_initializations)
