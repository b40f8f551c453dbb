"""The row geometry classes the launch planner can produce, derived from the planner itself (test infrastructure; not a conftest).

A kernel's distance loop is chosen by (row configuration, FULL or not, side-table chunks of a split row, one span or several).
`walk(dtype)` runs tests/launch_plan_harness.cpp -- through the loader of tests/test_launch_plan.py -- over every dim of
1 .. MAX_DIM and groups the dims by that key.  A class is represented by its SMALLEST dim, the one with the most zero padding
in the last chunk and in the row: the most lanes are clamped or masked there.  A clamped class has a second representative, its
DENSE dim: the smallest dim whose row is all data (row_bytes = dim x element size).  Rows padded to whole 128-byte lines end in
zero chunks at the smallest dim, so a clamped lane re-reads zeros there and a broken select would not show; at the dense dim it
re-reads data.  (Found by dropping the select of batch_dists' clamped branch: at the smallest dims only the three classes whose
rows are not padded to lines turned red.)
CLASSES pins the names of the classes the walk finds
today: tests/test_row_classes.py fails when the planner starts to produce another one, and tests/test_gpu_row_classes.py runs
every representative of every pinned class (CASES) through every search kernel family.

The walk is taken at the default layout: FLATNAV_ROW_PAD_PCT, FLATNAV_SPLIT_ROWS and FLATNAV_SPLIT_TAIL_MAX_MB are removed from
the environment while it runs.  The capacity is that of the GPU file's indexes (split rows depend on it only beyond 2 M rows)."""
from __future__ import annotations

import collections
import ctypes as C
import functools

import numpy as np
import pytest

import test_launch_plan as tlp
from flatnav_amd import datasets as ds

TYPES = {"float32": 9, "float16": 8, "uint8": 0, "int8": 4}  # FNV_DTYPE_* (include/flatnav_hip.h)
MAX_DIM = 9000
N_ROWS = 600  # rows of one index of tests/test_gpu_row_classes.py
LAYOUT_ENV = ("FLATNAV_ROW_PAD_PCT", "FLATNAV_SPLIT_ROWS", "FLATNAV_SPLIT_TAIL_MAX_MB")
# What the walk finds today, for every element type: <lanes per row>x<chunks per lane and span>-<form>[-spans].
CLASSES = ["8x1-clamped", "8x1-full", "8x2-clamped", "8x2-full", "8x3-full", "8x3-tail1", "8x3-tail2", "8x4-clamped", "8x4-full",
           "16x4-clamped", "16x4-full", "32x4-clamped", "32x4-full", "64x3-full", "64x4-clamped", "64x4-full", "64x4-clamped-spans",
           "64x4-full-spans"]

ELEM_BYTES = {"float32": 4, "float16": 2, "uint8": 1, "int8": 1}
RowClass = collections.namedtuple("RowClass", "name cfg G CU full tail_chunks multi_span dim n_dims last_dim dense_dim")


def cfgs():
    """kCfgs as the harness exports it: [(G, CU)] by configuration index."""
    L = tlp.lib()
    g, cu = C.c_int(0), C.c_int(0)
    out = []
    for c in range(L.lph_row_cfg(-1, C.byref(g), C.byref(cu))):
        L.lph_row_cfg(c, C.byref(g), C.byref(cu))
        out.append((g.value, cu.value))
    return out


def name_of(G, CU, full, tail_chunks, multi_span):
    form = "full" if full else "tail%d" % tail_chunks if tail_chunks else "clamped"
    return "%dx%d-%s%s" % (G, CU, form, "-spans" if multi_span else "")


def _plans(dtype: str, dims, capacity: int):
    """The planner harness's plan table over `dims`, at the default layout."""
    _, plan_cols, shape_cols = tlp.columns()
    dims = np.asarray(dims, np.int64).reshape(-1)
    opts = tlp.option_row({})
    cases = np.array([[TYPES[dtype], d, 8, capacity, 0, tlp.NUM_CUS, 64, 10, 16] + opts for d in dims.tolist()], np.int64)
    plans = np.empty((len(cases), len(plan_cols)), np.int64)
    none = np.empty(1, np.int64)
    with pytest.MonkeyPatch.context() as mp:
        for name in LAYOUT_ENV:
            mp.delenv(name, raising=False)
        tlp.lib().lph_sweep(cases.ctypes.data, len(cases), cases.shape[1], none.ctypes.data, 0, tlp.N_INIT, plans.ctypes.data, plans.shape[1],
                            none.ctypes.data, len(shape_cols))
    t = tlp.Table(plans, plan_cols)
    assert (t["rc"] == 0).all(), "the planner refuses a row width"
    return t


def geometry(dtype: str, dims, capacity: int = N_ROWS):
    """Per dim: (cfg, full, row_bytes, tail_bytes) as the planner's harness returns them, at the default layout."""
    t = _plans(dtype, dims, capacity)
    return t["cfg"], t["full"], t["row_bytes"], t["tail_bytes"]


def walk_of_row(dtype: str, dim: int, capacity: int = N_ROWS):
    """How the kernels walk a row of this dim, in the planner's words (row_geometry, csrc/launch_plan.hpp): a dict of cfg, G, CU,
    full, tail_chunks, nchunks (of the main table's row) and q_chunks (of the staged query).  tests/distance_model.py takes its
    geometry from here and restates no layout rule."""
    t = _plans(dtype, [dim], capacity)
    cfg = int(t["cfg"][0])
    G, CU = cfgs()[cfg]
    out = dict(cfg=cfg, G=G, CU=CU, full=bool(t["full"][0]), tail_chunks=int(t["heaps.tail_chunks"][0]), nchunks=int(t["heaps.nchunks"][0]),
               q_chunks=int(t["heaps.q_chunks"][0]))
    assert out["nchunks"] * 16 == t["row_bytes"][0] and out["tail_chunks"] * 16 == t["tail_bytes"][0], (dtype, dim)
    return out


def keys_of(dtype: str, dims, capacity: int = N_ROWS):
    """Per dim: the class key (cfg, full, tail_chunks, spans > 1); spans = ceil(main-table chunks / (G * CU))."""
    cfg, full, row_bytes, tail_bytes = geometry(dtype, dims, capacity)
    table = np.array(cfgs(), np.int64)
    per_span = table[cfg, 0] * table[cfg, 1]
    nchunks = row_bytes // 16
    assert (row_bytes % 16 == 0).all() and (tail_bytes % 16 == 0).all()
    spans = -(-nchunks // per_span)
    return list(zip(cfg.tolist(), full.tolist(), (tail_bytes // 16).tolist(), (spans > 1).tolist()))


@functools.lru_cache(maxsize=None)
def walk(dtype: str):
    """{class name: RowClass} over dims 1 .. MAX_DIM, in order of the classes' smallest dims."""
    table = cfgs()
    dims = np.arange(1, MAX_DIM + 1)
    dense = geometry(dtype, dims)[2] == dims * ELEM_BYTES[dtype]  # the row is all data: no zero padding behind it
    found = {}
    for dim, key, all_data in zip(dims.tolist(), keys_of(dtype, dims), dense.tolist()):
        first, n, _, first_dense = found.get(key, (dim, 0, dim, None))
        found[key] = (first, n + 1, dim, dim if all_data and first_dense is None else first_dense)
    out = {}
    for (cfg, full, tail, multi), (first, n, last, first_dense) in sorted(found.items(), key=lambda kv: kv[1][0]):
        G, CU = table[cfg]
        name = name_of(G, CU, full, tail, multi)
        assert name not in out
        out[name] = RowClass(name, cfg, G, CU, bool(full), tail, bool(multi), first, n, last, first_dense)
    return out


def representatives(dtype: str, name: str):
    """[(case name, dim)] of a class: its smallest dim, and for a clamped class its dense dim."""
    c = walk(dtype)[name]
    clamped = not c.full and not c.tail_chunks
    return [(name, c.dim)] + ([(name + "-dense", c.dense_dim)] if clamped else [])


CASES = [case for name in CLASSES for case in ([name] + ([name + "-dense"] if "clamped" in name else []))]


def dim_of(dtype: str, case: str) -> int:
    return dict(representatives(dtype, case[: -len("-dense")] if case.endswith("-dense") else case))[case]


def class_of(dtype: str, dim: int, capacity: int = N_ROWS) -> str:
    (cfg, full, tail, multi), = keys_of(dtype, [dim], capacity)
    G, CU = cfgs()[cfg]
    return name_of(G, CU, full, tail, multi)


def format_table() -> str:
    lines = ["%-20s %s" % ("class", "  ".join("%-30s" % t for t in TYPES)), ""]
    for name in CLASSES:
        cells = []
        for t in TYPES:
            c = walk(t).get(name)
            dense = "" if c is None or c.full or c.tail_chunks else ", dense %d" % c.dense_dim
            cells.append("%-30s" % ("-" if c is None else "%d (%d dims, to %d%s)" % (c.dim, c.n_dims, c.last_dim, dense)))
        lines.append("%-20s %s" % (name, "  ".join(cells)))
    return "\n".join(lines)


def float_case(dtype: str, metric: str, dim: int):
    """The float data of one class: (rows, queries) as an index of that type holds them."""
    X, Q = ds.randn(N_ROWS, 40, dim, seed=dim, normalize=metric == "ip")
    if dtype == "float16":
        X, Q = X.astype(np.float16), Q.astype(np.float16)
    return X, Q
