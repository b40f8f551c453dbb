"""The launch planner (flatnav_amd/csrc/launch_plan.hpp) on the CPU: tests/launch_plan_harness.cpp is compiled with g++, loaded
with ctypes and swept over element types, row widths, capacities, beam widths, occupancy caps and options -- far more
shapes than the GPU suite launches.  The HIP runtime is replaced by the byte-wise occupancy count the planner's comments
describe (lds > 163840 ? 0 : min(wave_cap, 163840 / max(lds, 1))).

What is asserted are the invariants the kernels rely on -- the LDS areas of a query slot are aligned, ordered and do not
overlap; the visited-table geometry satisfies the preconditions of the device side's model (tests/test_visited_model.py);
residency respects the LDS granules; the plan's mode follows its rules; a launch's shape is consistent -- plus the worked
examples the planner's comments state in full.  No other expected number is invented here."""
from __future__ import annotations

import atexit
import ctypes as C
import itertools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_visited_model import ModelVisited

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_plan_harness.cpp")
F32, U8, F16 = 9, 0, 8  # FNV_DTYPE_* (include/flatnav_hip.h)
FNV_ERR_INVALID = 1
WAVE, OVF_LIST, STASH = 64, 30, 64
SCAN_WAVES, SCAN_QPB, SCAN_QUEUE_IDS = 4, 32, 256  # (csrc/search_types.h, csrc/scan_select.hpp)
MODE_HEAPS, MODE_MERGED_REGS, MODE_MERGED_LDS = 0, 1, 2
LDS_PER_CU, GRANULE = 163840, 1280
NUM_CUS, M, K, N_INIT = 256, 16, 10, 100

ROWS = [(F32, d) for d in (40, 100, 104, 105, 128, 200, 768, 1000)] + [(U8, 128), (U8, 400), (F16, 128), (F16, 768)]
CAPACITIES = [1, 2, 4096, 2**16 - 1, 2**16 + 1, 2**24 - 1, 2**24 + 1, 2**30, 2**31 - 1, 2**31, 2**32 - 2]
BEAMS = [1, 10, 52, 64, 65, 128, 129, 256, 257, 800, 1200, 30000]  # (the last: too large for LDS)
WAVE_CAPS = [5, 12, 16, 20]
NQS = [1, 63, 64, 2048, 20000]
OPTION_SETS = {
    "default": {}, "visited_slots=256": {"visited_slots": 256}, "visited_slots=384": {"visited_slots": 384},
    "visited_slots=3072": {"visited_slots": 3072}, "visited_wide": {"visited_wide": 1}, "visited_tag_bits=21": {"visited_tag_bits": 21},
    "cand_slots=300": {"cand_slots": 300}, "sorted_cand_lds=0": {"sorted_cand_lds": 0}, "sorted_cand_lds=1": {"sorted_cand_lds": 1},
    "beam_registers=0": {"beam_registers": 0}, "blocks_per_cu=3": {"blocks_per_cu": 3}, "sorted_beam=0": {"sorted_beam": 0},
    "sorted_beam_min=100": {"sorted_beam_min": 100},
}
DEFAULTS = dict(visited_factor=27, visited_slots=0, visited_floor=2048, occupancy_target=13, occupancy_roomy=9, cand_factor=2, cand_slots=0,
                spill_entries=16384, blocks_per_cu=0, visited_wide=0, visited_tag_bits=0, sorted_beam=2, sorted_beam_min=1,
                sorted_cand_lds=2, sorted_tail_exact_pct=-1, beam_registers=1, shadow_exact=1, tie_replay=1, tie_log_entries=0,
                visited_direct=1, overflow_list=-1)  # IndexOptions' initial values
_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="flatnav_launch_plan_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "liblaunch_plan_harness.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        for f in (L.lph_option_columns, L.lph_param_columns, L.lph_plan_columns, L.lph_shape_columns):
            f.restype = C.c_char_p
        L.lph_plan.restype = C.c_void_p
        L.lph_plan.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.lph_free.argtypes = [C.c_void_p]
        L.lph_launch.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
        L.lph_sweep.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        L.lph_variant.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.lph_slots_per_cu.argtypes = [C.c_uint32]
        L.lph_tune_candidates.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_int]
        L.lph_scan_columns.restype = C.c_char_p
        L.lph_scan_sweep.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.lph_group_arrays.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        L.lph_entry_scan_tile.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]
        _lib = L
    return _lib


def _names(raw: bytes):
    return [n for n in raw.decode().split(",") if n]


def columns():
    """-> (option names, plan columns, shape columns); the parameter blocks are prefixed heaps. / sorted. / p."""
    L = lib()
    params = _names(L.lph_param_columns())
    plan = _names(L.lph_plan_columns()) + ["heaps." + p for p in params] + ["sorted." + p for p in params]
    shape = _names(L.lph_shape_columns()) + ["p." + p for p in params]
    return _names(L.lph_option_columns()), plan, shape


class Table:
    """Rows of int64 with named columns; `sub(prefix)` views one parameter block under its bare field names."""

    def __init__(self, rows, names, extra=None):
        self.rows, self.names, self.extra = rows, {n: i for i, n in enumerate(names)}, dict(extra or {})

    def __getitem__(self, name):
        return self.extra[name] if name in self.extra else self.rows[:, self.names[name]]

    def sub(self, prefix, **extra):
        names = {n[len(prefix):]: i for n, i in self.names.items() if n.startswith(prefix)}
        t = Table(self.rows, [], {**self.extra, **extra})
        t.names = names
        return t

    def where(self, mask):
        t = Table(self.rows[mask], [], {k: v[mask] for k, v in self.extra.items()})
        t.names = self.names
        return t

    def __len__(self):
        return len(self.rows)


def option_row(overrides):
    names = columns()[0]
    assert set(names) == set(DEFAULTS), "the harness and this file list the same options"
    return [dict(DEFAULTS, **overrides)[n] for n in names]


@pytest.fixture(scope="module", params=list(OPTION_SETS))
def sweep(request):
    """One option set over every (row, capacity, beam width, occupancy cap): the options, the cases, the plans and, per plan
    and batch size of NQS, the launches (rows of -1 where there is no plan)."""
    opts = dict(DEFAULTS, **OPTION_SETS[request.param])
    _, plan_cols, shape_cols = columns()
    grid = list(itertools.product(ROWS, CAPACITIES, BEAMS, WAVE_CAPS))
    cases = np.array([[dt, dim, M, cap, 0, NUM_CUS, B, K, wc] + option_row(OPTION_SETS[request.param]) for (dt, dim), cap, B, wc in grid], np.int64)
    plans = np.empty((len(cases), len(plan_cols)), np.int64)
    shapes = np.empty((len(cases), len(NQS), len(shape_cols)), np.int64)
    nqs = np.array(NQS, np.int64)
    lib().lph_sweep(cases.ctypes.data, len(cases), cases.shape[1], nqs.ctypes.data, len(NQS), N_INIT, plans.ctypes.data, plans.shape[1],
                    shapes.ctypes.data, shapes.shape[2])
    extra = {"capacity": cases[:, 3], "wave_cap": cases[:, 8], "dtype": cases[:, 0], "dim_in": cases[:, 1], "B_in": cases[:, 6]}
    plan = Table(plans, plan_cols, extra)
    assert set(np.unique(plan["rc"])) <= {0, FNV_ERR_INVALID}
    # (an ordinary beam may be refused as well: 1000-d float32 rows at B = 1200 on a 4096-row index -- the roomy table is untagged
    #  there, every smaller one is tagged, and the ladder never steps across a change of format)
    assert (plan["rc"][plan["B_in"] == 30000] == FNV_ERR_INVALID).all() and (plan["rc"][plan["B_in"] <= 800] == 0).all()
    ok = plan["rc"] == 0
    rep = lambda a: np.repeat(a[ok], len(NQS))
    launch = Table(shapes[ok].reshape(-1, shapes.shape[2]), shape_cols,
                   {"capacity": rep(cases[:, 3]), "nq": np.tile(nqs, int(ok.sum())), "plan_bpc": rep(plans[:, plan_cols.index("bpc")]),
                    "plan_sbpc": rep(plans[:, plan_cols.index("sbpc")])})
    return opts, plan.where(ok), launch


def align16(v):
    return (v + 15) // 16 * 16


def log2_exact(v):
    v = np.asarray(v, np.int64)
    assert ((v > 0) & ((v & (v - 1)) == 0)).all(), "a power of two"
    return np.round(np.log2(v.astype(np.float64))).astype(np.int64)


def occupancy(lds, wave_cap):
    return np.where(lds > LDS_PER_CU, 0, np.minimum(wave_cap, LDS_PER_CU // np.maximum(lds, 1)))


def blocks(plan, launch):
    """Every parameter block the sweep produced, with the mode it was laid out for and its LDS bytes: the two-heap layouts,
    the merged-beam layouts of the plans that run them, and what each launch hands its kernel (DIRECT forms included)."""
    merged = plan.where(plan["mode"] != MODE_HEAPS)
    return [("heaps", plan.sub("heaps.", mode=np.zeros(len(plan), np.int64), lds=plan["lds"])),
            ("sorted", merged.sub("sorted.", mode=merged["mode"], lds=merged["slds"])),
            ("launch", launch.sub("p.", mode=launch["mode"], lds=launch["lds"]))]


def test_lds_areas_are_aligned_ordered_and_disjoint(sweep):
    _, plan, launch = sweep
    for name, p in blocks(plan, launch):
        assert len(p) or name == "sorted", name  # (option sets that rule the merged-beam kernel out plan no such layout)
        B, mode, cand = p["B"], p["mode"], p["cand_slots"]
        for off in ("off_q", "off_vis", "off_stage_ids", "off_ovf"):
            assert (p[off] % 16 == 0).all(), (name, off)
        assert (p["off_nbr"] % 16 == 8).all() and (p["off_cand"] % 16 == 8).all(), name
        own_stage = mode == MODE_MERGED_LDS
        assert (p["off_stage_d"][own_stage] % 16 == 0).all() and (p["off_stage_d"][~own_stage] == p["off_nbr"][~own_stage]).all(), name
        # (start, size) of each area, in order; an absent area is empty and starts where the next one does
        nbr_size = np.maximum((B + 2) * 8, np.where(mode == MODE_MERGED_REGS, (WAVE + 1) * 4, 0))
        cand_start = np.where(cand > 0, p["off_cand"], p["off_vis"])
        areas = [(p["off_q"], p["q_lds_bytes"]), (p["off_nbr"], nbr_size),
                 (np.where(own_stage, p["off_stage_d"], cand_start), np.where(own_stage, (WAVE + 1) * 4, 0)),
                 (cand_start, np.where(cand > 0, (cand + 1) * 8, 0)),
                 (p["off_vis"], p["vis_bytes"]), (p["off_stage_ids"], np.full(len(p), (WAVE + 1) * 4)),
                 (p["off_ovf"], np.full(len(p), (OVF_LIST + 2 + STASH) * 4)), (p["lds"], 0)]
        assert (p["off_q"] == 0).all()
        for (start, size), (nxt, _) in zip(areas, areas[1:]):
            assert (start + size <= nxt).all(), name
        assert (p["lds"] == align16(p["off_ovf"] + (OVF_LIST + 2 + STASH) * 4)).all(), name
        assert (p["lds"] <= LDS_PER_CU).all(), name


def test_visited_geometry_meets_the_device_side_preconditions(sweep):
    _, plan, launch = sweep
    modelled = set()
    for name, p in blocks(plan, launch):
        cap = p["capacity"]
        nbits = np.maximum(1, np.ceil(np.log2(cap.astype(np.float64))).astype(np.int64))  # smallest n >= 1 with 2^n >= capacity
        assert ((1 << nbits) >= cap).all() and ((nbits == 1) | ((1 << (nbits - 1)) < cap)).all() and (nbits <= 32).all()
        direct = p["vis_w"] == 1  # small launches on small indexes: a bitmap of all node ids, no table
        assert name == "launch" or not direct.any()
        d = p.where(direct)
        assert (d["vis_bytes"] % 16 == 0).all() and (d["vis_bytes"] * 8 >= d["capacity"]).all() and (d["vis_slots"] == d["vis_bytes"] * 8).all()
        t = p.where((p["vis_tag16"] == 1) & ~direct)
        tb = nbits[(p["vis_tag16"] == 1) & ~direct]
        w, slots, mult = t["vis_w"], t["vis_slots"], t["vis_mult"]
        assert np.isin(w, (16, 21, 32)).all(), name
        fields = np.where(w == 16, 4, np.where(w == 21, 3, 2))
        buckets = slots // fields
        assert (fields * buckets == slots).all() and np.isin(mult, (1, 3)).all() and (buckets % mult == 0).all(), name
        assert (t["vis_rshift"] + log2_exact(buckets // mult) == tb).all(), name
        assert (t["vis_nmask"] == (1 << tb) - 1).all() and (t["vis_nmask"] >= t["capacity"] - 1).all(), name
        assert (t["vis_rmask"] == (1 << t["vis_rshift"]) - 1).all(), name
        assert (t["vis_rshift"] <= np.where(w == 16, np.where(mult == 3, 15, 14), w - 2)).all(), name  # the remainder fits the tag
        assert ((mult == 1) | (w == 16)).all(), name
        assert (t["vis_bytes"] == np.where(w == 16, slots * 2, buckets * 8)).all(), name
        model = (w == 16) & (mult == 1)
        modelled |= set(zip(slots[model].tolist(), tb[model].tolist()))
        u = p.where((p["vis_tag16"] == 0) & ~direct)
        assert (u["vis_shift"] == 32 - log2_exact(u["vis_slots"])).all() and (u["vis_limit"] == u["vis_slots"] // 4 * 3).all(), name
        assert (u["vis_bytes"] == u["vis_slots"] * 4).all(), name
    for slots, nbits in sorted(modelled):
        ModelVisited(slots, nbits)  # its asserts are the device side's preconditions


def test_residency_and_heap_trim(sweep):
    opts, plan, _ = sweep
    B = plan["B_in"]
    merged = plan["mode"] != MODE_HEAPS
    for lds, bpc, rows in ((plan["lds"], plan["bpc"], np.ones(len(plan), bool)), (plan["slds"], plan["sbpc"], merged)):
        lds, bpc, cap_w = lds[rows], bpc[rows], plan["wave_cap"][rows]
        assert (lds <= LDS_PER_CU).all()
        bound = np.minimum(occupancy(lds, cap_w), 128 // -(-lds // GRANULE))
        assert ((1 <= bpc) & (bpc <= np.maximum(bound, 1))).all()
        if opts["blocks_per_cu"]:
            assert (bpc == np.minimum(np.maximum(bound, 1), opts["blocks_per_cu"])).all()
        else:
            assert (bpc == np.maximum(bound, 1)).all()
    # the exact search's LDS heap: never below B + 1 entries, never more than an eighth below its rule value; a pinned size is kept
    rule = np.maximum(opts["cand_slots"] if opts["cand_slots"] else opts["cand_factor"] * B + 192, B + 1)
    in_lds = merged & (plan["sorted.cand_slots"] > 0)  # (the merged-beam layouts that keep the heap in LDS at all)
    for cand, r, b in ((plan["heaps.cand_slots"], rule, B), (plan["sorted.cand_slots"][in_lds], rule[in_lds], B[in_lds])):
        assert ((cand >= b + 1) & (cand <= r) & (cand >= r - r // 8)).all()
        if opts["cand_slots"]:
            assert (cand == r).all()
    if opts["visited_slots"]:  # a forced table size is honoured, up to power-of-two rounding for untagged tables
        forced = opts["visited_slots"]
        pow2 = 1 << (forced - 1).bit_length()
        for prefix, rows in (("heaps.", np.ones(len(plan), bool)), ("sorted.", merged)):
            slots, tagged = plan[prefix + "vis_slots"][rows], plan[prefix + "vis_tag16"][rows]
            assert ((slots == forced) | ((tagged == 0) & (slots == pow2))).all()


def test_lds_granules():
    # measured with tools/dev/probes/lds_granule.cpp, quoted above configure_launch: LDS bytes -> resident slots per CU
    for lds, slots in ((7680, 21), (7681, 18), (8960, 18), (8961, 16), (10240, 16), (10241, 14), (32768, 4)):
        assert lib().lph_slots_per_cu(lds) == slots
    # ... and its worked example: 7712 bytes hold seven granules, 18 per CU, where the byte-wise count says 21
    assert lib().lph_slots_per_cu(7712) == 18 and int(occupancy(np.int64(7712), 32)) == 21


def test_plan_mode_follows_its_rules(sweep):
    opts, plan, _ = sweep
    B, mode = plan["B_in"], plan["mode"]
    must_be_heaps = (plan["capacity"] >= 2**31) | (opts["sorted_beam"] == 0) | (B < opts["sorted_beam_min"]) | (plan["heaps.vis_tag16"] == 0)
    assert (mode[must_be_heaps] == MODE_HEAPS).all()
    assert np.isin(mode, (MODE_HEAPS, MODE_MERGED_REGS, MODE_MERGED_LDS)).all()
    regs = mode == MODE_MERGED_REGS
    assert (B[regs] <= 256).all() and (opts["beam_registers"] != 0 or not regs.any())
    merged = mode != MODE_HEAPS
    assert (plan["sorted.cand_slots"][merged] + plan["sorted.spill_entries"][merged] >= 3 * B[merged] + 256).all()
    assert (plan["sorted.vis_tag16"][merged] == 1).all()
    if request_is_default(opts):
        assert merged.any() and regs.any() and (mode == MODE_MERGED_LDS).any() and (~merged).any()  # the sweep reaches every mode


def request_is_default(opts):
    return opts == DEFAULTS


def test_launch_shape(sweep):
    opts, _, launch = sweep
    nq, nslots, bpc = launch["nq"], launch["nslots"], launch["bpc"]
    shadow = launch["shadow"] == 1
    assert (bpc == np.where(launch["sorted"] == 1, launch["plan_sbpc"], launch["plan_bpc"])).all()
    assert (nslots[shadow] == 2 * nq[shadow]).all() and (4 * nq[shadow] <= bpc[shadow] * NUM_CUS).all()
    assert (nslots[~shadow] == np.minimum(nq, bpc * NUM_CUS)[~shadow]).all()
    assert (launch["sorted"][shadow] == 1).all() and (launch["small_launch"][shadow] == 1).all()
    assert (launch["tail_exact"] <= nq).all()
    assert (launch["max_slots"] >= nslots).all()
    live, n_scan, step = launch["capacity"], launch["n_scan"], launch["scan_step"]
    assert ((n_scan - 1) * step < live).all() and (live <= n_scan * step).all()
    direct = launch["direct"] == 1
    assert (launch["small_launch"][direct] == 1).all() and (launch["p.vis_w"][direct] == 1).all() and (launch["p.vis_w"][~direct] != 1).all()
    if opts["visited_slots"] or opts["visited_wide"] or opts["visited_tag_bits"]:
        assert not direct.any()  # the caller pinned the table's shape
    if request_is_default(opts):
        assert shadow.any() and direct.any() and (~shadow).any()


def test_exact_tails_and_tail_shadows_of_pinned_variants():
    L = lib()
    _, plan_cols, shape_cols = columns()
    opts = np.array(option_row({}), np.int64)
    for (dt, dim), B in itertools.product(ROWS, (52, 129, 800)):
        plan = np.empty(len(plan_cols), np.int64)
        h = L.lph_plan(dt, dim, M, 4096, 0, NUM_CUS, opts.ctypes.data, B, K, 16, plan.ctypes.data)
        try:
            p = dict(zip(plan_cols, plan.tolist()))
            assert p["rc"] == 0 and p["mode"] != MODE_HEAPS
            for nq, pinned in itertools.product(NQS, range(7)):
                row = np.empty(len(shape_cols), np.int64)
                L.lph_launch(h, nq, N_INIT, 4096, pinned, row.ctypes.data)
                s = dict(zip(shape_cols, row.tolist()))
                multi_round = nq > p["sbpc"] * NUM_CUS
                assert s["multi_round"] == multi_round and s["tail_exact"] <= nq
                assert s["variant"] == (pinned if pinned < 2 or (pinned == 6) or multi_round else 1)  # an exact tail needs a second round
                assert (s["tail_exact"] > 0) == (s["variant"] in (2, 3, 4, 5))
                assert s["tail_shadows"] == (min(nq, s["nslots"]) if s["variant"] == 6 and not s["shadow"] else 0)
                assert s["sorted"] == (s["variant"] != 0)
        finally:
            L.lph_free(h)


SCAN_CASE = ("dtype", "dim", "capacity", "num_cus", "scan_segment_rows", "filter_scan_max", "filter_scan_on_overflow", "nq", "K", "live",
             "filter_rows")


def scan_shapes(cases) -> Table:
    """Rows of SCAN_CASE -> the exhaustive scan's shape and the routing decision for each (lph_scan_columns), the case's own
    fields next to them."""
    cases = np.ascontiguousarray(cases, np.int64).reshape(-1, len(SCAN_CASE))
    cols = _names(lib().lph_scan_columns())
    out = np.empty((len(cases), len(cols)), np.int64)
    lib().lph_scan_sweep(cases.ctypes.data, len(cases), out.ctypes.data)
    return Table(out, cols, {n: cases[:, i] for i, n in enumerate(SCAN_CASE)})


def ceil_div(a, b):
    return -(-a // b)


def group_tile_bound(nq, rows, tile):
    """scan_select.hpp's bound on a grouped scan's tiles: ceil(nq / tile) + min(rows, nq), and never more than nq."""
    return np.minimum(ceil_div(nq, tile) + np.minimum(rows, nq), nq)


def test_scan_shape_and_routing():
    # scan_shape's own comment: queries per tile as the block's LDS budget (20 KB, less the grouped scan's id queue) holds them,
    # at most 32; segments to fill the device, at most 64, at most live / 1024, partial lists within 256 MB -- or what
    # "scan_segment_rows" asks for, at most 1024; plan_scan_routing: not where the scan cannot take the call
    grid = itertools.product(ROWS + [(F32, 40000)], (1, 31, 32, 33, 1000, 100000, 2**31 - 1), (1, 10, 1024), (0, 1, 1023, 1024, 10**6, 2**31 - 1),
                             (0, 2, 3, 1002, 2**31 + 1), (0, 1, 4096), ((0, 0), (5, 0), (0, 1)))
    s = scan_shapes([[dt, dim, max(live, 1), NUM_CUS, seg_rows, scan_max, on_ovf, nq, K_, live, frows]
                     for (dt, dim), nq, K_, live, frows, seg_rows, (scan_max, on_ovf) in grid])
    assert len(s) == 13 * 7 * 3 * 6 * 5 * 3 * 3
    nq, K_, live, frows, seg_rows = s["nq"], s["K"], s["live"], s["filter_rows"], s["scan_segment_rows"]
    tile, tiles, segments, lds = s["tile"], s["tiles"], s["segments"], s["lds"]
    grouped = frows > 0
    assert ((1 <= tile) & (tile <= np.minimum(32, nq))).all()
    assert (lds == tile * (s["q_chunks"] * 16 + K_ * 8) + np.where(grouped, SCAN_QUEUE_IDS * 4, 0)).all()
    assert (lds[tile > 1] <= 20 << 10).all()
    assert (tiles == np.where(grouped, group_tile_bound(nq, frows, tile), ceil_div(nq, tile))).all()
    assert (segments >= 1).all() and (tiles * segments <= 2**31 - 1).all()
    auto = seg_rows == 0
    assert (segments[auto] <= 64).all() and (segments[auto] <= np.maximum(1, live[auto] // 1024)).all()
    assert ((segments == 1) | (nq * segments * K_ * 8 <= 256 << 20))[auto].all()
    forced = ~auto
    assert (segments[forced] <= 1024).all() and (segments[forced] <= np.maximum(1, ceil_div(live[forced], seg_rows[forced]))).all()
    assert (auto & (segments > 1)).any() and (forced & (segments > 1)).any()
    assert (s["partial_bytes"] == nq * segments * K_ * 8).all() and (s["merge_lds"] == 3 * K_ * 8).all()
    # routing is off exactly when both options are off, or K > 1024, or the scan's LDS exceeds a block's 160 KB (and without a filter)
    options_off = (s["filter_scan_max"] <= 0) & (s["filter_scan_on_overflow"] == 0)
    too_long = lds > 160 << 10
    assert too_long.any() and (~too_long).any()  # the refusal is reached
    assert ((s["routed"] == 0) == (options_off | too_long | ~grouped)).all()
    wide = scan_shapes([[F32, 128, 4096, NUM_CUS, 0, 5, 1, 100, K_, 4096, 3] for K_ in (1024, 1025)])
    assert wide["routed"].tolist() == [1, 0]


def test_group_arrays():
    # GroupArrays' own comment: query_row | perm | counts | cursor | row_count | slot_start | tile_start | tiles [| route], as
    # uint32 offsets; counts | cursor | row_count are the prefix one memset clears
    names = ("query_row", "perm", "counts", "cursor", "row_count", "slot_start", "tile_start", "tiles", "route", "bytes", "cleared_bytes")
    out = np.empty(len(names), np.int64)
    for nq, rows, routed in itertools.product((1, 33, 100000), (0, 3, 1002), (0, 1)):
        bound = int(group_tile_bound(nq, rows, 32))
        lib().lph_group_arrays(nq, rows, bound, routed, out.ctypes.data)
        ga = dict(zip(names, out.tolist()))
        sizes = [nq, nq, rows, rows, rows, rows + 1, rows + 1, 3 * bound] + ([nq + 1] if routed else [])
        starts = [ga[n] for n in names[:9]]
        end = 0
        for start, size in zip(starts, sizes):  # in the documented order, each where the one before ends: disjoint
            assert start == end
            end = start + size
        assert starts[8] == ga["tiles"] + 3 * bound  # (unrouted: the route words' offset is the end)
        assert ga["bytes"] == 4 * end
        assert ga["cursor"] == ga["counts"] + rows and ga["row_count"] == ga["cursor"] + rows and ga["slot_start"] == ga["row_count"] + rows
        assert ga["cleared_bytes"] == 4 * (ga["slot_start"] - ga["counts"]) == 4 * 3 * rows


def test_entry_scan_tile():
    # entry_scan_tile's own comment: whole rows 16 bytes apart, as many as 64 KB hold (at least one), behind SCAN_WAVES staged
    # queries and SCAN_QPB results of 8 bytes
    L = lib()
    _, plan_cols, _ = columns()
    opts = np.array(option_row({}), np.int64)
    out = np.empty(4, np.int64)
    several = False
    for dt, dim in ROWS + [(F32, 40000)]:
        plan = np.empty(len(plan_cols), np.int64)
        L.lph_free(L.lph_plan(dt, dim, M, 4096, 0, NUM_CUS, opts.ctypes.data, 52, K, 16, plan.ctypes.data))
        p = dict(zip(plan_cols, plan.tolist()))
        row_bytes, q_chunks = p["row_bytes"], p["heaps.q_chunks"]
        for n_scan, nq in itertools.product((1, 2, 100, 4096, 2**31 - 1), (1, 32, 33, 100000)):
            L.lph_entry_scan_tile(row_bytes, q_chunks, n_scan, nq, out.ctypes.data)
            stride, rows, lds, grid = out.tolist()
            assert stride == row_bytes + 16 and 1 <= rows <= n_scan
            assert rows * stride <= 64 << 10 or rows == 1
            assert lds == SCAN_WAVES * q_chunks * 16 + SCAN_QPB * 8 + rows * stride
            assert grid == ceil_div(nq, SCAN_QPB)
            several |= 1 < rows < n_scan
    assert several


def test_slot_workspace(sweep):
    # slot_workspace: per query slot, what the plan's parameter blocks tell the kernels about each area
    _, plan, _ = sweep
    assert (plan["ws_bitmap"] == plan["heaps.bitmap_words"] * 4).all() and (plan["ws_ovf"] == plan["heaps.ovf_cap"] * 4).all()
    assert (plan["ws_spill"] == plan["heaps.spill_entries"] * 8).all() and (plan["ws_tielog"] == plan["heaps.log_entries"] * 8).all()
    merged = plan["mode"] != MODE_HEAPS
    assert (plan["sorted.log_entries"][merged] == plan["heaps.log_entries"][merged]).all()
    assert (plan["ws_bytes"] == plan["ws_bitmap"] + plan["ws_ovf"] + plan["ws_spill"] + plan["ws_tielog"]).all()


def test_row_layouts_the_comments_state():
    # row_layout: d = 97 ... 104 float32 keeps three whole lines (stride 384) + one or two 16-byte chunks in the side table, while
    # that table stays within 64 MB; row_stride_bytes: a 100-d float32 row is padded to 512 bytes otherwise
    L = lib()
    _, plan_cols, _ = columns()
    opts = np.array(option_row({}), np.int64)

    def layout(dt, dim, cap):
        plan = np.empty(len(plan_cols), np.int64)
        L.lph_free(L.lph_plan(dt, dim, M, cap, 0, NUM_CUS, opts.ctypes.data, 52, K, 16, plan.ctypes.data))
        p = dict(zip(plan_cols, plan.tolist()))
        return p["row_bytes"], p["tail_bytes"]

    assert layout(F32, 97, 4096) == (384, 16) and layout(F32, 100, 4096) == (384, 16) and layout(F32, 104, 4096) == (384, 32)
    assert layout(U8, 385, 4096) == (384, 16) and layout(U8, 416, 4096) == (384, 32)
    assert layout(F32, 100, 4 << 20) == (384, 16) and layout(F32, 100, (4 << 20) + 1) == (512, 0)


def variant(which, best=None, samples=None, multi_round=True, try_tail=True, shadows_on=True, pinned=-1):
    b = np.array(best if best is not None else [-1.0] * 7, np.float32)
    s = np.array(samples if samples is not None else [0] * 7, np.int32)
    return lib().lph_variant(which, b.ctypes.data, s.ctypes.data, int(multi_round), int(try_tail), int(shadows_on), pinned)


PINNED, LANE, NEXT_SAMPLE, FINAL = 0, 1, 2, 3


@pytest.mark.parametrize("multi_round,try_tail,shadows_on", list(itertools.product((False, True), repeat=3)))
def test_owner_samples_in_order_then_takes_the_fastest(multi_round, try_tail, shadows_on):
    allowed = [v for v in range(7) if lib().lph_variant_allowed(v, multi_round, try_tail, shadows_on, 0)]
    assert allowed == ([0, 1, 2, 3, 4, 5] if multi_round and try_tail else [0, 1])  # 6 is never part of the adaptive choice
    flags = dict(multi_round=multi_round, try_tail=try_tail, shadows_on=shadows_on)
    best, samples, order = [-1.0] * 7, [0] * 7, []
    time_of = {0: 5.0, 1: 5.0, 2: 4.0, 3: 3.5, 4: 6.0, 5: 3.5, 6: 0.1}
    while (v := variant(NEXT_SAMPLE, best, samples, **flags)) >= 0:
        order.append(v)
        best[v], samples[v] = time_of[v], samples[v] + 1
        assert len(order) <= 21
    assert order == [v for v in (1, 0, 6, 4, 3, 2, 5) if v in allowed for _ in range(3)]
    # the fastest; of equals the first in ordinal order -- except that the merged-beam kernel (1) wins a tie against the two-heap kernel (0)
    assert variant(FINAL, best, samples, **flags) == (3 if 3 in allowed else 1)
    # a measured variant 6 (pinned A/B runs leave none, but the rule must not depend on that) is still never picked
    best[6], samples[6] = 0.1, 3
    assert variant(FINAL, best, samples, **flags) != 6 and variant(LANE, best, samples, **flags) != 6
    assert variant(NEXT_SAMPLE, best, samples, **flags) == -1


def test_lane_never_explores():
    assert variant(LANE) == -1  # nothing measured: the lane keeps the plan's default and samples nothing
    best, samples = [2.0, 3.0, -1.0, 1.0, -1.0, -1.0, -1.0], [1, 3, 0, 2, 0, 0, 0]
    assert variant(LANE, best, samples) == 3 and variant(LANE, best, samples, multi_round=False) == 0
    assert variant(LANE, [2.0, 2.0] + [-1.0] * 5, [3, 3, 0, 0, 0, 0, 0]) == 0  # (the lane's tie rule: the lowest ordinal)
    assert variant(FINAL, [2.0, 2.0] + [-1.0] * 5, [3, 3, 0, 0, 0, 0, 0]) == 1  # (the owner's: the merged-beam kernel)
    for unsampled in range(2, 6):  # a variant without samples is never a lane's pick, however its slot reads
        b, s = [2.0] * 7, [1] * 7
        b[unsampled], s[unsampled] = 0.0, 0
        assert variant(LANE, b, s) != unsampled


def test_pinned_variants():
    for v in range(7):
        for multi_round, shadows_on in itertools.product((False, True), repeat=2):
            can_run = v < 2 or (shadows_on if v == 6 else multi_round)
            assert variant(PINNED, multi_round=multi_round, shadows_on=shadows_on, pinned=v) == (v if can_run else 1)


def test_tune_candidates_stay_in_the_ladder():
    out = np.empty(2 * 16, np.int64)
    for base, w, heap_lds in itertools.product((256, 384, 512, 768, 3072, 4096, 24576, 32768), (16, 21, 32), (0, 1)):
        n = lib().lph_tune_candidates(base, w, heap_lds, out.ctypes.data, 16)
        cands = out[: 2 * n].reshape(n, 2)
        assert n <= 16 and tuple(cands[0]) == (-1, 0)  # [0]: the rules' own layout
        assert (cands[1:, 0] == -1).any() == (base >= 512) and np.isin(cands[:, 0], (-1, 1 - heap_lds)).all()  # the heap home, flipped
        sized = cands[cands[:, 1] != 0, 1]
        assert ((sized >= 256) & (sized <= 1 << 15) & (sized != base)).all()
        assert all(s & (s - 1) == 0 or (s % 3 == 0 and (s // 3) & (s // 3 - 1) == 0) for s in sized.tolist())
