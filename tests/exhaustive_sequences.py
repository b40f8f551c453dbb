"""Seeded call sequences of the exhaustive search (test infrastructure; not a conftest): what one handle is asked, step by step,
as a serving process asks it -- unfiltered, single-filter and grouped calls of changing nq, K, segment length, filter, radius and
engine options -- with the planner's answer for every step and the numpy contract of its results.
tests/test_exhaustive_sequences_plan.py replays the sequences through the planner alone and holds them to the code they are
meant to reach; tests/test_gpu_exhaustive_sequences.py runs them on one device index each.

The data: _int_data's small integers (every distance an exact integer in any summation order, in float16 and in
bfloat16-narrowed float32 as well), a quarter of the rows copied onto a second block and an eighth onto a third (the node id
decides; a distance is attained three times), every eighth row all zeros and one all-zero query, and on l2 three queries copied
into rows (distance 0: the radii -0.0 and 0.0).  The zeros: on ip a zero row is at distance 1 from every query, and the zero query
from every row.  On l2 the float16 engines' prefilter margin (scan_margin, csrc/scan_select.hpp) is ZERO for a zero row and the
zero query and nowhere else, and on integer data a row's bound can EQUAL the K-th distance only there: every other pair's bound is
its exact integer distance less a margin that is no integer.  The compacted candidate list is in no particular order, so among
more than K zero rows one with a smaller id arrives after the list is full of zeros -- the one place where these sequences tell
`bound > kd` from `bound >= kd`.

Everything here is in ROW order with labels: a filter is a set of labels.  The GPU file builds the index with several threads, so
its node order differs -- candidate SETS, counts and in-range counts do not depend on it, the planner sees none of it."""
from __future__ import annotations

import collections
import ctypes as C
import functools

import numpy as np

import row_classes as rc
import test_scan_matrix_block_plan as block_plan
from test_gpu_exhaustive import _dist64, _topk
from test_gpu_filtered import _int_data
from test_gpu_range_search import _expected

SEED = 122  # (the first seed at which tests/test_exhaustive_sequences_plan.py holds)
STEPS = 40  # per index
NQ = 130  # queries of an index; a step takes the first nq
ZERO_QUERY = 40  # Q[ZERO_QUERY] is all zeros: in every call of more than 40 queries
ZERO_STRIDE = 8  # rows 5, 13, 21, ... are all zeros (and the copies of such rows)
QUERY_ROWS = (0, 1, 33)  # l2: these queries are copied into rows
MAX_K = 1024  # SCAN_MAX_K
MAX_LDS = 160 << 10  # kScanMaxLds
OWN = {"uint8": "scan_matrix", "int8": "scan_matrix", "float16": "scan_matrix_float", "float32": "scan_matrix_float32"}
WAVE_MODE = {"uint8": 4, "int8": 4, "float16": 5, "float32": 6}  # fnv_last_launch_geometry's kernel mode of the type's engine
NQ_SET = (1, 31, 32, 33, 64, 65, 129, 130)
SEG_SET = (0, 20, 31, 64, 250, 4096)
RADII = ("below", "tie", "median", "above", "inf", "zero")

Index = collections.namedtuple("Index", "dtype metric dim n")
# kind: "all" (unfiltered), "one" (allowed=filters[0]) or "grouped" (filters, qf); radius: None or a float32; own / grouped /
# block: the element type's engine option, "scan_matrix_grouped", "scan_matrix_block"; foreign: the other two engine options
Step = collections.namedtuple("Step", "kind nq K seg filters qf radius radius_kind own grouped block foreign")
# what the planner makes of a step: refused (the call raises), kernel_mode, waves (0: not the block form), row segments
Plan = collections.namedtuple("Plan", "refused kernel_mode waves segments")


@functools.lru_cache(maxsize=None)
def indexes() -> tuple:
    """Per (element type, metric): a row inside the matrix engines' register span (float types: at most 8 MFMA steps, the block
    form's reach) and one beyond it; float16 a second, three-step row (the block form on l2 float16 rows is where a bound can equal the K-th distance), float32 a split row with a side-table tail.
    n % 64 is never 0 or 1; 1003 keeps n - 1, n and n + 5 below the largest K."""
    dims = {"uint8": (120, 200), "int8": (72, 200), "float16": (40, 128, 200), "float32": (128, 200, rc.dim_of("float32", "8x3-tail1"))}
    sizes = (1237, 2203, 1003, 1500, 1789, 2467)
    out = [Index(t, m, d, 0) for t in dims for m in ("l2", "ip") for d in dims[t]]
    return tuple(ix._replace(n=sizes[i % len(sizes)]) for i, ix in enumerate(out))


def name_of(ix: Index) -> str:
    return "%s-%s-%d-%d" % ix


def _rng(ix: Index, what: int):
    return np.random.default_rng([SEED, what, rc.TYPES[ix.dtype], len(ix.metric), ix.dim, ix.n])


@functools.lru_cache(maxsize=4)
def data(ix: Index):
    """(X, Q, labels) in row order; labels are not row numbers."""
    rng, n = _rng(ix, 0), ix.n
    X, Q = _int_data(rng, n, NQ, ix.dim, ix.dtype, ix.metric)
    X[5::ZERO_STRIDE] = 0
    X[n // 2:n // 2 + n // 4] = X[:n // 4]
    X[n - 7 - n // 8:n - 7] = X[:n // 8]
    Q[ZERO_QUERY] = 0
    if ix.metric == "l2":
        for i, q in enumerate(QUERY_ROWS):
            X[n // 4 + 5 + i] = Q[q]
    return X, Q, (rng.permutation(n) + 3).astype(np.int32)


def _rows(rng, n, c):
    """c rows: at random, or -- half of the time, where the copied block holds them -- as pairs of a row and its copy, the last
    pair cut in two by an odd c: exact duplicates on both sides of the filter."""
    if rng.random() < 0.5 and (c + 1) // 2 <= n // 4:
        h = rng.choice(n // 4, (c + 1) // 2, replace=False)
        return np.concatenate([h, h + n // 2])[:c]
    return rng.choice(n, c, replace=False)


def _pick(rng, values, share=0.5, lo=1, hi=1):
    """One of `values`, or (the other share of the draws) uniform in lo .. hi."""
    return int(values[rng.integers(len(values))] if rng.random() < share or hi <= lo else rng.integers(lo, hi + 1))


def row_candidates(step: Step, labels) -> list:
    """Per query of the step: the ascending ids, in the order of `labels`, of its candidates."""
    everything = np.arange(len(labels))
    if step.kind == "all":
        return [everything] * step.nq
    of_filter = [np.flatnonzero(np.isin(labels, f)) for f in step.filters]
    return [of_filter[0] if step.kind == "one" else everything if f < 0 else of_filter[f] for f in (step.qf if step.kind == "grouped" else [0] * step.nq)]


def expected(step: Step, D, labels, cands=None):
    """The contract of the step's results from exact distances D[>= nq][n] in the order of `labels`: (dist float32 [nq, K],
    labels int32 [nq, K], count, n_dist) -- _expected of tests/test_gpu_range_search.py under a radius, else _topk of
    tests/test_gpu_exhaustive.py over each group of queries that shares its candidates."""
    cands = row_candidates(step, labels) if cands is None else cands
    if step.radius is not None:
        return _expected(D[:step.nq], cands, labels, step.K, step.radius)
    d, l = np.empty((step.nq, step.K), np.float32), np.empty((step.nq, step.K), np.int32)
    count, total = np.empty(step.nq, np.int32), np.empty(step.nq, np.uint64)
    group = np.zeros(step.nq, np.int64) if step.kind != "grouped" else step.qf.astype(np.int64)
    for g in np.unique(group):
        rows = np.flatnonzero(group == g)
        nodes = cands[rows[0]]
        d[rows], l[rows], count[rows], total[rows] = _topk(D[rows][:, nodes], nodes, labels, step.K)
    return d, l, count, total


def _radius(rng, ix: Index, step: Step, D, labels):
    """(radius, its kind), drawn among the kinds this call's candidates allow: below the smallest candidate distance; a distance at
    least three candidates of query 0 attain; the median; above the largest; +inf; on l2, where a copy of a query exists, +-0."""
    cands = row_candidates(step, labels)
    mine = np.concatenate([D[q, c] for q, c in enumerate(cands)])
    values, counts = np.unique(D[0, cands[0]], return_counts=True)
    kinds = [k for k in RADII if (k != "tie" or counts.max(initial=0) >= 3) and (k != "median" or mine.size) and (k != "zero" or ix.metric == "l2")]
    kind = kinds[rng.integers(len(kinds))]
    tied = values[counts >= 3]
    r = {"below": mine.min(initial=D.min()) - 1.0, "tie": tied[rng.integers(len(tied))] if len(tied) else 0.0, "median": np.median(mine) if mine.size else 0.0,
         "above": D.max() + 1.0, "inf": np.inf, "zero": (-0.0, 0.0)[int(rng.integers(2))]}[kind]
    return np.float32(r), kind


@functools.lru_cache(maxsize=None)
def sequence(ix: Index) -> tuple:
    """The STEPS steps of an index.  Every input is drawn on its own; the weights lean towards the calls the planner treats
    apart -- one filter, the engines on, more than one sub-tile of queries -- and step 0 has no radius (the sequence ends by
    repeating it with every option set back)."""
    X, Q, labels = data(ix)
    D = _dist64(X, Q, ix.metric)
    rng, n = _rng(ix, 1), ix.n
    k_set = [k for k in (1, 2, 9, 10, 11, 32, 33, 100, 101, 255, 256, n - 1, n, n + 5, 1024) if k <= MAX_K]
    sizes = [0, 1, 31, 32, 33, 65, n // 100, n // 10, n // 2, n - 1, n]
    steps = []
    for i in range(STEPS):
        kind = ("all", "one", "grouped")[int(rng.choice(3, p=(0.15, 0.5, 0.35)))]
        nq, K, seg = _pick(rng, NQ_SET, 0.6, 1, NQ), _pick(rng, k_set, 0.5, 1, 300), _pick(rng, SEG_SET, 1.0)
        filters, qf = None, None
        if kind == "one":
            filters = [labels[_rows(rng, n, _pick(rng, sizes, 1.0))]]
        if kind == "grouped":
            filters = [labels[_rows(rng, n, _pick(rng, sizes, 1.0))] for _ in range(int(rng.integers(1, 7)))]
            idle = int(rng.integers(len(filters)))  # this filter row has no query
            used = np.array([f for f in range(-1, len(filters)) if f != idle])
            qf = used[rng.integers(len(used), size=nq)].astype(np.int32)
        own, grouped, block = (int(rng.random() < p) for p in (0.75, 0.7, 0.75))
        step = Step(kind, nq, K, seg, filters, qf, None, None, own, grouped, block, tuple(int(b) for b in rng.integers(0, 2, 2)))
        if i and rng.random() < 0.45:
            step = step._replace(**dict(zip(("radius", "radius_kind"), _radius(rng, ix, step, D, labels))))
        steps.append(step)
    return tuple(steps)


def option_values(ix: Index, step: Step) -> dict:
    """The options a step sets before its call ("scan_radius": the radius's float32 bits, -1 = off)."""
    others = [name for name in ("scan_matrix", "scan_matrix_float", "scan_matrix_float32") if name != OWN[ix.dtype]]
    bits = -1 if step.radius is None else int(np.array([step.radius], np.float32).view(np.uint32)[0])
    return {OWN[ix.dtype]: step.own, **dict(zip(others, step.foreign)), "scan_matrix_grouped": step.grouped, "scan_matrix_block": step.block,
            "scan_segment_rows": step.seg, "scan_radius": bits}


def plan(ix: Index, step: Step) -> Plan:
    """What scan_device_impl (csrc/launch.hip) does with the step, from the planner alone (tests/scan_matrix_block_harness.cpp):
    it refuses a call whose vector scan exceeds a block's LDS (with a radius: the in-range counter included); else it records
    kernel mode 7 / 8 where the block form took the call, 6 / 5 / 4 by element type where a matrix engine did, else 3."""
    o = option_values(ix, step)
    c = (C.c_int64 * 16)(rc.TYPES[ix.dtype], ix.dim, ix.n, 256, step.seg, o["scan_matrix"], o["scan_matrix_float"], o["scan_matrix_float32"],
                         step.grouped, step.block, step.nq, step.K, ix.n, len(step.filters) + 2 if step.kind == "grouped" else 0,
                         step.radius is not None, step.kind == "one")
    out = (C.c_int64 * len(block_plan.FIELDS))()
    block_plan.lib().smb_shape(c, out)
    s = dict(zip(block_plan.FIELDS, (int(v) for v in out)))
    mode = WAVE_MODE[ix.dtype] + 2 if s["waves"] else WAVE_MODE[ix.dtype] if s["on"] else 3
    return Plan(block_plan.lib().smb_vector_lds(c) > MAX_LDS, mode, s["waves"], s["segments"])
