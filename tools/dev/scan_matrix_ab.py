#!/usr/bin/env python3
"""Developer tool: the exhaustive search's two engines -- the vector scan and the matrix engine ("scan_matrix" = 1,
csrc/scan_matrix.hpp) -- on ONE c2-uint8-like index, same handle, same process, alternating.  With --dtype float16: the vector
scan and the float16 matrix engine ("scan_matrix_float" = 1, csrc/scan_matrix_f16.hpp) on one float16 index of Gaussian rows of
--dim elements; the line then also carries the share of the scored pairs that the prefilter let through to the exact rescoring
(DeviceIndex.scan_rescored), and the peak is the 2517 TFLOP/s of the float16 matrix instructions.  With --dtype float32: the same
for the float32 matrix engine ("scan_matrix_float32" = 1, csrc/scan_matrix_f32.hpp) on one float32 index; the peak is that of the
bfloat16 matrix instructions, the same figure.

  python tools/dev/scan_matrix_ab.py [--dtype uint8|float16|float32] [--dim 128] [--n 1000000] [--nq 10000] [--fractions 1,0.1,0.01,0.001]
                                     [--rounds 3] [--steps 5] [--json out.json]

The SIFT-1M stand-in as uint8 (flatnav_amd.datasets.sift_like; rows stored without a graph: the scan does not read one),
device-resident queries, K = 10.  For every fraction of allowed labels (1 = unfiltered; else a random set) it times, HIP
events on the launch stream, `--rounds` rounds of `--steps` launches per engine, vector then matrix in every round.  Per line:
each engine's median, min and max over the rounds, the ratio of the medians, whether the matrix median lies below the vector
median by more than the vector engine's own max - min, the matrix engine's launch shape, its achieved integer op rate
(2 * nq * candidates * padded dim) against the 5033 TOP/s int8 matrix peak (256 CUs x 4 SIMDs x 1024 MAC per cycle at 2.4 GHz)
and the row bytes it moves (ceil(nq / tile) * candidates * row_bytes).  Before timing, both engines' outputs are compared byte
for byte at every fraction.

With --grouped N_FILTERS[,N_FILTERS...] the call is search_exhaustive_grouped instead ("scan_matrix_grouped" = 1 on top of the
engine's option against the grouped vector scan, csrc/scan_matrix_feed.hpp): for every filter count and every share of
--allowed SHARE[,SHARE...] a table of that many random filters, each allowing that share of the labels, the queries spread evenly
over the filters (query q uses filter q % N_FILTERS).  The line's candidates are then the mean per query, and --fractions is not read.

With --radius ROWS[,ROWS...] the comparison is the range search's (option "scan_radius"): for every target, a radius that admits
about that many rows per query; per engine, the unfiltered call with the radius against the same call without it, alternating in
every round -- medians, min and max, the ratio, whether the range call is slower by more than the other's own max - min, the mean
number of rows in range (out_ndist) and the share of pairs a float engine rescored in either call.  --fractions is not read.

With --block (float16 / float32, ungrouped, no radius) a THIRD engine runs in every round on the same handle: the block form of the
float engine ("scan_matrix_block" = 1 on top of its option, csrc/scan_matrix_block.hpp).  Its bytes are compared with the vector
scan's at every line, and the line carries its median, min and max, its launch shape, the row bytes it moves, its rescored share
and whether it beats the WAVE engine's median by more than the wave engine's own max - min."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flatnav_amd as flatnav  # noqa: E402
from flatnav_amd import datasets as ds  # noqa: E402
from flatnav_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--fractions", default="1,0.1,0.01,0.001")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--dtype", default="uint8", choices=["uint8", "float16", "float32"])
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--grouped", default="", help="filter counts of grouped calls, comma separated")
ap.add_argument("--allowed", default="0.5", help="grouped calls: the share of the labels a filter allows, comma separated")
ap.add_argument("--radius", default="", help="range search: rows per query the radius should admit, comma separated (e.g. 10,10000)")
ap.add_argument("--block", action="store_true", help="float engines: the block form as a third engine in every round")
args = ap.parse_args()

HALVES = args.dtype != "uint8"  # a float engine: Gaussian rows, a prefilter with rescoring
assert HALVES or args.dim == 128, "the uint8 index is the 128-d SIFT stand-in"
N, NQ, K, DIM = args.n, args.nq, 10, args.dim
ROW_BYTES = DIM * {"uint8": 1, "float16": 2, "float32": 4}[args.dtype]
PEAK_TOPS = 2517.0 if HALVES else 5033.0
OPTION, MODE = {"uint8": ("scan_matrix", 4), "float16": ("scan_matrix_float", 5), "float32": ("scan_matrix_float32", 6)}[args.dtype]
NP_T, DATA_T = {"uint8": (np.uint8, flatnav.data_type.DataType.uint8), "float16": (np.float16, flatnav.data_type.DataType.float16),
                "float32": (np.float32, flatnav.data_type.DataType.float32)}[args.dtype]
dev_t = torch.device("cuda", 0)
torch.cuda.set_device(0)
X, Q = ds.randn(N, NQ, DIM, seed=1) if HALVES else ds.sift_like(N, NQ)
index = flatnav.index.create("l2", DIM, N, 32, DATA_T)
index.set_device(0)
index.allocate_nodes(X.astype(NP_T))
scan = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)
tq = torch.from_numpy(Q.astype(NP_T)).to(dev_t)
out = {e: (torch.empty((NQ, K), dtype=torch.float32, device=dev_t), torch.empty((NQ, K), dtype=torch.int32, device=dev_t),
           torch.empty(NQ, dtype=torch.int32, device=dev_t), torch.empty(NQ, dtype=torch.int64, device=dev_t)) for e in (0, 1, 2)}
ENGINES = (0, 1, 2) if args.block else (0, 1)  # the vector scan, the (wave) matrix engine, the float engines' block form
assert not args.block or (args.dtype != "uint8" and not args.grouped and not args.radius), "--block: a float engine's ungrouped call"
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)


def launch(engine, bits, n_bits, qf=None):
    d, l, c, nd = out[engine]
    if qf is not None:  # a grouped call: `bits` is the filter table [filters][ceil(n_bits / 8)]
        scan.set_option("scan_matrix_grouped", engine)
        scan.search_device_exhaustive_grouped(tq.data_ptr(), NQ, K, bits.data_ptr(), bits.shape[0], bits.shape[1], n_bits, qf.data_ptr(),
                                              d.data_ptr(), l.data_ptr(), c.data_ptr(), nd.data_ptr(), stream=stream.cuda_stream)
        return
    scan.set_option(OPTION, int(engine != 0))
    scan.set_option("scan_matrix_block", int(engine == 2))
    scan.search_device_exhaustive(tq.data_ptr(), NQ, K, d.data_ptr(), l.data_ptr(), c.data_ptr(), nd.data_ptr(),
                                  bits_ptr=bits.data_ptr() if n_bits else 0, n_bits=n_bits, use_filter=n_bits > 0,
                                  stream=stream.cuda_stream)


def once(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def filter_table(n_filters, share):
    """(table uint8 [n_filters][ceil(N / 8)] on the device, labels allowed per filter): random filters, made and packed on the device."""
    torch.manual_seed(n_filters)
    weights = (2 ** torch.arange(8, device=dev_t)).to(torch.int32)
    table = torch.empty((n_filters, (N + 7) // 8), dtype=torch.uint8, device=dev_t)
    counts = torch.empty(n_filters, dtype=torch.int64, device=dev_t)
    for r in range(n_filters):
        mask = torch.zeros(table.shape[1] * 8, dtype=torch.int32, device=dev_t)
        mask[:N] = torch.rand(N, device=dev_t) < share
        counts[r] = mask.sum()
        table[r] = (mask.view(-1, 8) * weights).sum(1).to(torch.uint8)
    return table, counts


def radius_lines():
    """--radius: the unfiltered call with option "scan_radius" against the same call without it, per engine, alternating in every
    round.  The radius that admits `rows` rows per query on average: bisected on the scan's own out_ndist, between the smallest
    distance of the radius-off call and a radius that admits enough."""
    empty = torch.zeros(1, dtype=torch.uint8, device=dev_t)

    def mean_in_range(r):
        scan.set_option("scan_radius", int(np.array([r], np.float32).view(np.uint32)[0]))
        launch(1, empty, 0)
        torch.cuda.synchronize()
        return out[1][3].double().mean().item()

    scan.set_option("scan_radius", -1)
    launch(1, empty, 0)
    torch.cuda.synchronize()
    nearest, kth = float(out[1][0].min().item()), float(out[1][0][:, -1].max().item())
    found = []
    for rows in [int(x) for x in args.radius.split(",")]:
        lo, hi = nearest, kth
        while mean_in_range(hi) < rows:
            hi = lo + 2.0 * (hi - lo)
        for _ in range(16):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mean_in_range(mid) < rows else (lo, mid)
        r = hi
        for e in (0, 1):
            def call(radius_on, e=e, r=r):
                scan.set_option("scan_radius", int(np.array([r], np.float32).view(np.uint32)[0]) if radius_on else -1)
                launch(e, empty, 0)
            shares, ms = {}, {False: [], True: []}
            for on in (False, True):  # warm-up; the kernel that ran, the in-range rows, the pairs rescored
                once(lambda: call(on), 1)
                scan.status()
                g, rs = scan.launch_geometry(), scan.scan_rescored()
                assert g["kernel_mode"] == (MODE if e else 3) and g["range"] == int(on), g
                shares[on] = rs["rescored"] / max(1, rs["scored"])
            in_range = out[e][3].double().mean().item()
            for _ in range(args.rounds):
                for on in (False, True):
                    ms[on].append(once(lambda: call(on), args.steps))
            med = {on: statistics.median(ms[on]) for on in ms}
            spread = max(ms[False]) - min(ms[False])
            found.append(dict(dtype=args.dtype, dim=DIM, engine="matrix" if e else "vector", target_rows=rows, radius=r, in_range_mean=in_range,
                              off_ms=ms[False], range_ms=ms[True], off_median=med[False], range_median=med[True],
                              ratio=med[False] / med[True], off_spread=spread, slower_beyond_spread=bool(med[True] - med[False] > spread),
                              rescored_share_off=shares[False], rescored_share_range=shares[True]))
            print("radius %-12g (target %d rows, %.1f in range) %-6s | off %9.3f ms [%9.3f .. %9.3f] | range %9.3f ms [%9.3f .. %9.3f] | "
                  "off / range %5.2fx  slower beyond spread: %s | rescored %.5f -> %.5f of the pairs"
                  % (r, rows, in_range, found[-1]["engine"], med[False], min(ms[False]), max(ms[False]), med[True], min(ms[True]), max(ms[True]),
                     found[-1]["ratio"], found[-1]["slower_beyond_spread"], shares[False], shares[True]), flush=True)
    scan.set_option("scan_radius", -1)
    return found


GROUPED = [int(x) for x in args.grouped.split(",") if x]
CASES = [(f, g) for g in GROUPED for f in [float(x) for x in args.allowed.split(",")]] if GROUPED else [(float(x), 0) for x in args.fractions.split(",")]
if args.radius:  # (the range search's own comparison; no fractions, no grouped calls)
    CASES = []
scan.set_option(OPTION, 1 if GROUPED else 0)  # (grouped calls: the engine's own option stays on, "scan_matrix_grouped" alternates)
lines = []
for f, n_filters in CASES:
    qf = None
    if n_filters:
        bits, counts = filter_table(n_filters, f)
        n_bits, qf = N, (torch.arange(NQ, device=dev_t) % n_filters).to(torch.int32)
        per_query = counts[qf.long()]
        rows = range(int(round(per_query.double().mean().item())))  # (its length: the mean candidates of a query)
    else:
        rows = np.arange(N) if f >= 1 else np.sort(rng.choice(N, max(1, int(round(f * N))), replace=False))
        b, n_bits = hip.pack_allowed(rows) if f < 1 else (np.zeros(1, np.uint8), 0)
        bits = torch.from_numpy(b).to(dev_t)
        per_query = torch.full((NQ,), len(rows), dtype=torch.int64, device=dev_t)
    geom, pairs = {}, {}
    for e in ENGINES:  # warm-up, the launch shapes, and the same bytes from every engine
        once(lambda: launch(e, bits, n_bits, qf), 1)
        scan.status()
        geom[e] = scan.launch_geometry()
        pairs[e] = scan.scan_rescored() if HALVES else {"scored": 0, "rescored": 0}
    rescored = pairs[1]
    assert geom[0]["kernel_mode"] == 3 and geom[1]["kernel_mode"] == MODE and ("queue_ids" in geom[1]) == bool(n_filters), geom
    assert not args.block or geom[2]["kernel_mode"] in (MODE, MODE + 2), geom  # (MODE: the planner declined the shape)
    for e in ENGINES[1:]:
        assert not HALVES or pairs[e]["scored"] == int(per_query.sum().item()), pairs
        for x, y in zip(out[0], out[e]):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (f, e)
        assert torch.equal(out[e][3], per_query)
    ms = {e: [] for e in ENGINES}
    for _ in range(args.rounds):
        for e in ENGINES:
            ms[e].append(once(lambda: launch(e, bits, n_bits, qf), args.steps))
    med = {e: statistics.median(ms[e]) for e in ENGINES}
    spread = max(ms[0]) - min(ms[0])
    tile = geom[1]["tile_queries"]
    ops = 2.0 * NQ * len(rows) * DIM
    line = dict(fraction=f, filters=n_filters, candidates=len(rows), vector_ms=ms[0], matrix_ms=ms[1], vector_median=med[0], matrix_median=med[1],
                ratio=med[0] / med[1], vector_spread=spread, beats_by_more_than_spread=bool(med[0] - med[1] > spread),
                vector_geometry=geom[0], matrix_geometry=geom[1], matrix_tops=ops / (med[1] * 1e-3) / 1e12,
                matrix_of_peak=ops / (med[1] * 1e-3) / 1e12 / PEAK_TOPS, matrix_row_bytes=math.ceil(NQ / tile) * len(rows) * ROW_BYTES,
                rescored_share=rescored["rescored"] / max(1, rescored["scored"]), dtype=args.dtype, dim=DIM)
    if args.block:  # the block form against the WAVE engine of the same rounds
        wave_spread = max(ms[1]) - min(ms[1])
        line.update(block_ms=ms[2], block_median=med[2], block_geometry=geom[2], wave_spread=wave_spread, block_over_wave=med[1] / med[2],
                    block_beats_wave_by_more_than_spread=bool(med[1] - med[2] > wave_spread),
                    block_row_bytes=math.ceil(NQ / geom[2]["tile_queries"]) * len(rows) * ROW_BYTES,
                    block_rescored_share=pairs[2]["rescored"] / max(1, pairs[2]["scored"]))
    lines.append(line)
    print("filters %-5d f=%-6g cand %8d | vector %9.3f ms [%9.3f .. %9.3f] | matrix %9.3f ms [%9.3f .. %9.3f] | %6.2fx  beats spread: %s | "
          "matrix grid %d lds %d tile %d segments %d | %.1f TOP/s (%.4f of peak), row bytes %.3e | rescored %.4f of the pairs"
          % (n_filters, f, len(rows), med[0], min(ms[0]), max(ms[0]), med[1], min(ms[1]), max(ms[1]), line["ratio"], line["beats_by_more_than_spread"],
             geom[1]["grid_blocks"], geom[1]["lds_bytes"], tile, geom[1]["segments"], line["matrix_tops"], line["matrix_of_peak"],
             line["matrix_row_bytes"], line["rescored_share"]), flush=True)
    if args.block:
        print("        block  %9.3f ms [%9.3f .. %9.3f] | wave / block %5.2fx  beats the wave engine's spread (%.3f ms): %s | mode %d threads %d "
              "grid %d lds %d tile %d segments %d | row bytes %.3e | rescored %.4f of the pairs"
              % (med[2], min(ms[2]), max(ms[2]), line["block_over_wave"], line["wave_spread"], line["block_beats_wave_by_more_than_spread"],
                 geom[2]["kernel_mode"], geom[2]["block_threads"], geom[2]["grid_blocks"], geom[2]["lds_bytes"], geom[2]["tile_queries"],
                 geom[2]["segments"], line["block_row_bytes"], line["block_rescored_share"]), flush=True)
if args.radius:
    lines = radius_lines()
scan.set_option(OPTION, 0)
scan.set_option("scan_matrix_grouped", 0)
scan.set_option("scan_matrix_block", 0)
if args.json:
    json.dump(lines, open(args.json, "w"), indent=1)
