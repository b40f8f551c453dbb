#!/usr/bin/env python3
"""Developer tool: the exhaustive search (fnv_search_batch_exhaustive_device) against the filtered graph search
(fnv_search_batch_filtered_device) on ONE c2-like graph, in one process, alternating.

  python tools/dev/exhaustive_ab.py [--n 1000000] [--ef 52,200] [--fractions 1,0.5,0.1,0.01,0.001] [--rounds 3] [--steps 5]
                                    [--slow-ms 250] [--json out.json]

Builds the SIFT-1M stand-in (flatnav_amd.datasets.sift_like, labels = row numbers) with the device builder.  For every fraction
of allowed labels (a random set; a label range) it times, HIP events on the launch stream, `--rounds` rounds of `--steps`
launches of `--nq` device-resident queries, the best round counting:
  graph ef=<ef>   the filtered graph search on a view with spill_entries = 2^18 (the yardstick: the code as it was)
  scan            the exhaustive search
one after the other per round.  A graph launch whose warm-up took longer than --slow-ms is timed as ONE launch per round (a
1 % filter costs it ~0.6 s per launch).  Per line: ms, queries/s, the graph search's recall@10 against the exhaustive answer,
the scan's achieved FLOP/s (2 * dim per (query, candidate)) against the 157.3 TFLOP/s fp32 vector peak, and the row bytes it
moves (ceil(nq / tile) * candidates * row_bytes).  The exhaustive answers are also compared with a torch float64 brute force
over the allowed rows: every distance against the float64 distance of its own label and against the true sorted top K, to
DESIGN section 8's float bar (rtol 1e-5, atol 1e-6).  Last: the fraction at which the two cost the same, per ef, by log-log
interpolation between the measured fractions.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

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
ap.add_argument("--ef", default="52,200")
ap.add_argument("--fractions", default="1,0.5,0.1,0.01,0.001")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--slow-ms", type=float, default=250.0)
ap.add_argument("--json", default="")
args = ap.parse_args()

N, NQ, K, M, DIM = args.n, args.nq, 10, 32, 128
PEAK_TFLOPS = 157.3
RTOL, ATOL = 1e-5, 1e-6
dev_t = torch.device("cuda", 0)
torch.cuda.set_device(0)
t0 = time.time()
X, Q = ds.sift_like(N, NQ)
index = flatnav.index.create("l2", DIM, N, M)
index.set_num_threads(16)
index.set_device(0)
for s in range(0, N, 250_000):
    index.add(X[s:s + 250_000], 100, labels=list(range(s, min(N, s + 250_000))), device=True)
base = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)
print("# c2-like N=%d: graph built on the device in %.1fs" % (N, time.time() - t0), flush=True)
filt = base.view()
filt.set_option("spill_entries", 1 << 18)
scan = base.view()

tq = torch.from_numpy(Q).to(dev_t)
tx = torch.from_numpy(X).to(dev_t)
xn = (tx.double() ** 2).sum(1)
qn = (tq.double() ** 2).sum(1)
gd = torch.empty((NQ, K), dtype=torch.float32, device=dev_t)
gl = torch.empty((NQ, K), dtype=torch.int32, device=dev_t)
gc = torch.empty(NQ, dtype=torch.int32, device=dev_t)
sd = torch.empty((NQ, K), dtype=torch.float32, device=dev_t)
sl = torch.empty((NQ, K), dtype=torch.int32, device=dev_t)
sc = torch.empty(NQ, dtype=torch.int32, device=dev_t)
sn = torch.empty(NQ, dtype=torch.int64, device=dev_t)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)


def launch_graph(ef, bits, n_bits):
    filt.search_device_filtered(tq.data_ptr(), NQ, K, ef, 100, bits.data_ptr() if n_bits else 0, n_bits, gd.data_ptr(),
                                gl.data_ptr(), gc.data_ptr(), stream=stream.cuda_stream)


def launch_scan(bits, n_bits):
    scan.search_device_exhaustive(tq.data_ptr(), NQ, K, sd.data_ptr(), sl.data_ptr(), sc.data_ptr(), sn.data_ptr(),
                                  bits_ptr=bits.data_ptr() if n_bits else 0, n_bits=n_bits, use_filter=True,
                                  stream=stream.cuda_stream)


def once(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def brute_force(rows):
    """float64 distances [NQ, len(rows)] in blocks -> (true sorted top-K distances, and a lookup of any label's distance)."""
    r = torch.from_numpy(rows).to(dev_t)
    xs, xsn = tx[r].double(), xn[r]
    top = torch.empty((NQ, K), dtype=torch.float64, device=dev_t)
    for s in range(0, NQ, 500):
        d = qn[s:s + 500, None] + xsn[None, :] - 2.0 * (tq[s:s + 500].double() @ xs.T)
        top[s:s + 500] = torch.topk(d, min(K, len(rows)), dim=1, largest=False, sorted=True).values
    return top


def own_distance(labels):
    """float64 distance of every (query, reported label): labels = row numbers."""
    rows = tx[labels.long().clamp(min=0)].double()  # [NQ, K, DIM]
    return ((rows - tq.double()[:, None, :]) ** 2).sum(2)


filters = []
for f in [float(x) for x in args.fractions.split(",")]:
    k = max(1, int(round(f * N)))
    if f >= 1:
        filters.append((f, "all", np.arange(N)))
        continue
    filters.append((f, "random", np.sort(rng.choice(N, k, replace=False))))
    start = int(rng.integers(0, N - k + 1))
    filters.append((f, "contiguous", np.arange(start, start + k)))

efs = [int(x) for x in args.ef.split(",")]
out = []
geom = None
for f, how, rows in filters:
    b, n_bits = hip.pack_allowed(rows)
    bits = torch.from_numpy(b).to(dev_t)
    cands = len(rows)
    # warm-ups decide how the graph search is timed
    graph_steps = {}
    for ef in efs:
        warm = once(lambda: launch_graph(ef, bits, n_bits), 1)
        graph_steps[ef] = args.steps if warm <= args.slow_ms else 1
        try:
            filt.status()
        except RuntimeError as e:  # FNV_ERR_CAPACITY even with the raised spill area: no number for this line
            print("f=%-6g %-10s graph ef=%d: %s" % (f, how, ef, e), flush=True)
            graph_steps[ef] = 0
    once(lambda: launch_scan(bits, n_bits), 1)
    best = {}
    for _ in range(args.rounds):
        for ef in efs:
            if graph_steps[ef]:
                ms = once(lambda: launch_graph(ef, bits, n_bits), graph_steps[ef])
                best[ef] = min(best.get(ef, ms), ms)
        ms = once(lambda: launch_scan(bits, n_bits), args.steps)
        best["scan"] = min(best.get("scan", ms), ms)
    scan.status()
    geom = scan.launch_geometry()
    # agreement of the scan with float64
    launch_scan(bits, n_bits)
    torch.cuda.synchronize()
    assert int((sc != min(K, cands)).sum().item()) == 0 and int((sn != cands).sum().item()) == 0
    top = brute_force(rows)
    own = own_distance(sl)
    got = sd.double()
    e_own = float(((got - own).abs() / (ATOL + RTOL * own.abs())).max().item())
    e_top = float(((got - top).abs() / (ATOL + RTOL * top.abs())).max().item())
    assert e_own <= 1.0 and e_top <= 1.0, (f, how, e_own, e_top)
    tiles = math.ceil(NQ / max(1, (geom["lds_bytes"] // (DIM * 4 + K * 8))))
    row_bytes_moved = tiles * cands * DIM * 4
    tflops = 2.0 * DIM * NQ * cands / (best["scan"] * 1e-3) / 1e12
    line = dict(fraction=f, how=how, candidates=cands, scan_ms=best["scan"], scan_qps=NQ / best["scan"] * 1e3, scan_tflops=tflops,
                scan_of_peak=tflops / PEAK_TFLOPS, scan_row_bytes=row_bytes_moved, err_own_of_bar=e_own, err_topk_of_bar=e_top,
                grid_blocks=geom["grid_blocks"], lds_bytes=geom["lds_bytes"], graph={})
    print("f=%-6g %-10s scan %9.3f ms %11.0f q/s  %6.2f TFLOP/s (%.3f of peak)  row bytes %.3e  |err| own %.3f / top-K %.3f of the bar"
          % (f, how, best["scan"], line["scan_qps"], tflops, line["scan_of_peak"], row_bytes_moved, e_own, e_top), flush=True)
    for ef in efs:
        if not graph_steps[ef]:
            continue
        launch_graph(ef, bits, n_bits)
        torch.cuda.synchronize()
        filt.status()
        recall = float(((gl.long().unsqueeze(2) == sl.long().unsqueeze(1)) & (sl.long().unsqueeze(1) >= 0)).any(dim=2).float().sum().item()
                       / max(1, int(sc.sum().item())))
        line["graph"][ef] = dict(ms=best[ef], qps=NQ / best[ef] * 1e3, recall_vs_scan=recall, scan_speedup=best[ef] / best["scan"],
                                 steps=graph_steps[ef])
        print("         %-10s graph ef=%-4d %9.3f ms %11.0f q/s  recall@10 vs scan %.4f  scan is %.3f x  (%d launch(es) per round)"
              % ("", ef, best[ef], NQ / best[ef] * 1e3, recall, best[ef] / best["scan"], graph_steps[ef]), flush=True)
    out.append(line)

# the crossover: the fraction at which graph ms == scan ms, log-log between the measured fractions (random sets)
for ef in efs:
    pts = sorted((l["fraction"], math.log(l["graph"][ef]["ms"] / l["scan_ms"])) for l in out
                 if "how" in l and l["how"] in ("random", "all") and ef in l["graph"])
    cross = None
    for (f0, r0), (f1, r1) in zip(pts, pts[1:]):
        if r0 == 0 or (r0 > 0) != (r1 > 0):
            t = r0 / (r0 - r1) if r0 != r1 else 0.0
            cross = math.exp(math.log(f0) + t * (math.log(f1) - math.log(f0)))
    print("crossover ef=%d: %s" % (ef, "f = %.4g (scan faster below)" % cross if cross else
                                   "none inside the measured fractions (scan %s everywhere)" % ("faster" if pts[0][1] > 0 else "slower")), flush=True)
    out.append(dict(ef=ef, crossover_fraction=cross))
if args.json:
    json.dump(out, open(args.json, "w"), indent=1)
