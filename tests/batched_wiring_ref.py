"""ctypes front-end of tests/batched_wiring_ref.cpp, the CPU model of the batched device builder's wiring rule (test
infrastructure; the product never loads it).

`insert_batch(blob, node_size, data_size, M, dtype, metric, dim, first, count, efc, beams)` returns the link table of nodes
[0, first + count) after the batch (uint32 [first + count, M]) and a dict of path counters.  `beams` = (distances float32
[count, efc], node ids int32 [count, efc], counts int32 [count]), closest first, what a search with K = ef = efc returns.
float16 blobs are widened to float32 first (exact): the oracle and the model work on the float32 values the float16 ones
widen to, as tests/test_float16.py does it.

`oracle_beams` / `Batch` build a batch's inputs from the oracle, for both test files that use the model."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "batched_wiring_ref.cpp")
DTYPE_ORD = {"float32": 9, "uint8": 0, "int8": 4}
ESIZE = {"float32": 4, "float16": 2, "uint8": 1, "int8": 1}
COUNTERS = ["max_requesters", "chunked_targets", "pruned_then_extended", "shared_free_slots", "block_crossing_runs",
            "wide_prunes", "equal_key_pops", "short_beam_nodes", "targets", "pruned_targets", "wide_prunes_connect", "requests"]
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="flatnav_batched_wiring_ref_"), "libbatched_wiring_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.bwr_insert_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                       C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        assert L.bwr_n_counters() == len(COUNTERS)
        _lib = L
    return _lib


def widen_f16_blob(blob, n: int, dim: int, M: int) -> np.ndarray:
    """A float16 AoS blob with its data section widened to float32 (exact); links and labels as they are."""
    nodes = np.asarray(blob).view(np.uint8).reshape(-1)[: n * (2 * dim + 4 * M + 4)].reshape(n, 2 * dim + 4 * M + 4)
    out = np.empty((n, 4 * dim + 4 * M + 4), np.uint8)
    out[:, : 4 * dim] = nodes[:, : 2 * dim].copy().view(np.float16).astype(np.float32).view(np.uint8)
    out[:, 4 * dim:] = nodes[:, 2 * dim:]
    return out.reshape(-1)


def insert_batch(blob, node_size: int, data_size: int, M: int, dtype: str, metric: str, dim: int, first: int, count: int,
                 efc: int, beams, dump_node: int = -1):
    n = first + count
    if dtype == "float16":
        blob, dtype = widen_f16_blob(blob, n, dim, M), "float32"
        node_size, data_size = 4 * dim + 4 * M + 4, 4 * dim
    blob = np.ascontiguousarray(np.asarray(blob).view(np.uint8).reshape(-1))
    assert blob.size >= node_size * n
    bd = np.ascontiguousarray(beams[0], dtype=np.float32)
    bi = np.ascontiguousarray(beams[1], dtype=np.int32)
    bc = np.ascontiguousarray(beams[2], dtype=np.int32)
    assert bd.shape == (count, efc) and bi.shape == (count, efc) and bc.shape == (count,)
    links = np.empty((n, M), np.uint32)
    ctr = np.zeros(len(COUNTERS), np.uint64)
    rc = lib().bwr_insert_batch(blob.ctypes.data, node_size, data_size, M, DTYPE_ORD[dtype], 0 if metric == "l2" else 1, dim, first,
                                count, efc, bd.ctypes.data, bi.ctypes.data, bc.ctypes.data, links.ctypes.data, ctr.ctypes.data,
                                dump_node)
    assert rc == 0, "batched_wiring_ref: %s" % {2: "a beam shorter than M/2 but longer than 16 has equal distances"}.get(rc, "bad arguments")
    return links, {k: int(v) for k, v in zip(COUNTERS, ctr)}


def oracle_dtype(dtype: str) -> str:
    return "float32" if dtype == "float16" else dtype  # the oracle works on the float32 values float16 widens to


def oracle_beams(oracle_mod, metric: str, dtype: str, dim: int, M: int, blob, first: int, queries, efc: int):
    """The beams of an insertion batch: the oracle's search with K = ef = efc over the first `first` nodes of `blob` (an
    oracle-layout blob whose labels are the node ids).  -> ((dist, ids, count), sum of n_dist)"""
    dt = oracle_dtype(dtype)
    node_size = dim * ESIZE[dt] + 4 * M + 4
    live = oracle_mod.OracleIndex.from_blob(metric, dt, dim, first, first, M, np.asarray(blob).reshape(-1)[: first * node_size])
    d, l, st = live.search(queries, efc, efc, stats=True)
    return (d, l, st["count"]), int(st["n_dist"].sum())


class Batch:
    """A whole table in the oracle's layout, live nodes [0, n_live) wired, every record present, labels = node ids.  `insert`
    runs the model for the next `count` nodes and adopts its links."""

    def __init__(self, oracle_mod, metric: str, dtype: str, dim: int, M: int, X, first: int, efc: int):
        self.orc, self.metric, self.dtype, self.dim, self.M, self.efc = oracle_mod, metric, dtype, dim, M, efc
        self.odt = oracle_dtype(dtype)
        self.X = np.ascontiguousarray(X, dtype={"float32": np.float32, "uint8": np.uint8, "int8": np.int8}[self.odt])
        n = len(self.X)
        self.data_size = dim * ESIZE[self.odt]
        self.node_size = self.data_size + 4 * M + 4
        seed = oracle_mod.OracleIndex.create(metric, dim, first, M, self.odt)
        seed.add(self.X[:first], efc)
        nodes = np.empty((n, self.node_size), np.uint8)
        nodes[:, : self.data_size] = self.X.view(np.uint8).reshape(n, self.data_size)
        ids = np.arange(n, dtype=np.uint32)
        nodes[:, self.data_size: self.data_size + 4 * M] = np.repeat(ids[:, None], M, axis=1).view(np.uint8)
        nodes[:, self.data_size + 4 * M:] = ids.astype(np.int32)[:, None].view(np.uint8)
        want_labels = nodes[:first, self.data_size + 4 * M:].copy()
        nodes[:first] = np.asarray(seed.blob())[: first * self.node_size].reshape(first, self.node_size)
        assert np.array_equal(nodes[:first, self.data_size + 4 * M:], want_labels)  # default labels = node ids
        self.nodes, self.first, self.n_live = nodes, first, first
        self.initial = nodes.copy()  # the table before any batch: what a device index is loaded with

    def links(self, n=None):
        n = self.n_live if n is None else n
        return self.nodes[:n, self.data_size: self.data_size + 4 * self.M].copy().view(np.uint32)

    def device_blob(self):
        """(blob, node_size, data_size) of the initial table in the index's own element type (float16: the data section
        narrowed, exact)."""
        if self.dtype != "float16":
            return self.initial.reshape(-1), self.node_size, self.data_size
        n, dim = len(self.initial), self.dim
        out = np.empty((n, 2 * dim + 4 * self.M + 4), np.uint8)
        out[:, : 2 * dim] = self.initial[:, : 4 * dim].copy().view(np.float32).astype(np.float16).view(np.uint8)
        out[:, 2 * dim:] = self.initial[:, 4 * dim:]
        return out.reshape(-1), 2 * dim + 4 * self.M + 4, 2 * dim

    def insert(self, count: int, dump_node: int = -1):
        """-> (links of [0, n_live + count) after the batch, counters, the beam searches' distance evaluations)"""
        first = self.n_live
        beams, evals = oracle_beams(self.orc, self.metric, self.odt, self.dim, self.M, self.nodes, first,
                                    self.X[first: first + count], self.efc)
        links, ctr = insert_batch(self.nodes.reshape(-1), self.node_size, self.data_size, self.M, self.odt, self.metric, self.dim,
                                  first, count, self.efc, beams, dump_node)
        self.nodes[: first + count, self.data_size: self.data_size + 4 * self.M] = links.view(np.uint8)
        self.n_live = first + count
        return links, ctr, evals

    def search(self, Q, K: int, ef: int):
        o = self.orc.OracleIndex.from_blob(self.metric, self.odt, self.dim, self.n_live, self.n_live, self.M,
                                           self.nodes[: self.n_live].reshape(-1))
        return o.search(np.asarray(Q).astype(self.X.dtype), K, ef)


def integer_data(rng, n: int, dim: int, dtype: str, hi: int):
    """Integer values 0 .. hi-1 (int8: centred on zero) in the element type the oracle stores for `dtype`."""
    lo = -(hi // 2) if dtype == "int8" else 0
    return rng.integers(lo, lo + hi, (n, dim)).astype({"float16": np.float32}.get(dtype, dtype))
