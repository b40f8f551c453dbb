#!/usr/bin/env python3
"""Developer tool: grouped filters (fnv_search_batch_*_grouped_device: one allowed set per query, one launch) against what a
caller had to do without them -- one single-filter launch per allowed set on that set's sub-batch -- on ONE c2-like graph, in
one process, alternating.

  python tools/dev/grouped_filters_ab.py [--n 1000000] [--nq 10000] [--rounds 3] [--steps 5] [--json out.json]

Builds the SIFT-1M stand-in of tools/dev/exhaustive_ab.py (labels = row numbers) with the device builder and times, HIP events
on the launch stream, `--rounds` rounds of `--steps` repetitions, the best round counting, the two sides one after the other
per round:
  tenants, exhaustive   100 disjoint allowed sets of 1 % of the labels each -- a random partition, then label ranges -- 100
                        queries per set in shuffled order: ONE grouped launch against the loop of 100
                        fnv_search_batch_exhaustive_device launches on the 100-query sub-batches
  tenants, graph        10 sets of 10 %, 1 000 queries each, ef = 52: one grouped launch against 10
                        fnv_search_batch_filtered_device launches
  one group             every query on filter 0 of a one-filter table, 100 % / 10 % / 1 % of the labels: the grouped scan against
                        the single-filter scan (in-kernel bit extraction against the compacted id list)
Before it is timed, every grouped launch is compared with the loop it replaces: the same bytes in every row.
"""
import argparse
import ctypes
import json
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--json", default="")
args = ap.parse_args()

N, NQ, K, M, DIM, EF = args.n, args.nq, 10, 32, 128, 52
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
graph = base.view()
graph.set_option("spill_entries", 1 << 18)
scan = base.view()
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)


def once(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(steps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def best_of(sides):
    """sides: {name: callable}; alternating round by round -> {name: best ms}."""
    for fn in sides.values():
        once(fn, 1)
    best = {}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            ms = once(fn, args.steps)
            best[name] = min(best.get(name, ms), ms)
    return best


class Outputs:
    def __init__(self, nq):
        self.d = torch.empty((nq, K), dtype=torch.float32, device=dev_t)
        self.l = torch.empty((nq, K), dtype=torch.int32, device=dev_t)
        self.c = torch.empty(nq, dtype=torch.int32, device=dev_t)
        self.n = torch.zeros(nq, dtype=torch.int64, device=dev_t)
        self.h = torch.zeros(nq, dtype=torch.int64, device=dev_t)

    def rows(self, idx):
        return [t[idx] for t in (self.d.view(torch.int32), self.l, self.c, self.n, self.h)]


def tenants(sets, exhaustive):
    """One grouped launch against one single-filter launch per set; queries are dealt to the sets evenly, in shuffled order."""
    F = len(sets)
    table, n_bits = hip.pack_filters(sets)
    tt = torch.from_numpy(table).to(dev_t)
    qf = rng.permutation(np.arange(NQ) % F).astype(np.int32)
    tqf = torch.from_numpy(qf).to(dev_t)
    tq = torch.from_numpy(Q).to(dev_t)
    idx = [torch.from_numpy(np.flatnonzero(qf == f)).to(dev_t) for f in range(F)]
    sub_q = [tq[i].contiguous() for i in idx]
    sub_out = [Outputs(len(i)) for i in idx]
    out = Outputs(NQ)
    stride = table.shape[1]

    def grouped():
        if exhaustive:
            scan.search_device_exhaustive_grouped(tq.data_ptr(), NQ, K, tt.data_ptr(), F, stride, n_bits, tqf.data_ptr(), out.d.data_ptr(),
                                                  out.l.data_ptr(), out.c.data_ptr(), out.n.data_ptr(), stream=stream.cuda_stream)
        else:
            graph.search_device_filtered_grouped(tq.data_ptr(), NQ, K, EF, 100, tt.data_ptr(), F, stride, n_bits, tqf.data_ptr(),
                                                 out.d.data_ptr(), out.l.data_ptr(), out.c.data_ptr(), out.n.data_ptr(), out.h.data_ptr(),
                                                 stream=stream.cuda_stream)

    def loop():
        for f in range(F):
            o, q = sub_out[f], sub_q[f]
            if exhaustive:
                scan.search_device_exhaustive(q.data_ptr(), len(q), K, o.d.data_ptr(), o.l.data_ptr(), o.c.data_ptr(), o.n.data_ptr(),
                                              bits_ptr=tt.data_ptr() + f * stride, n_bits=n_bits, use_filter=True, stream=stream.cuda_stream)
            else:
                graph.search_device_filtered(q.data_ptr(), len(q), K, EF, 100, tt.data_ptr() + f * stride, n_bits, o.d.data_ptr(),
                                             o.l.data_ptr(), o.c.data_ptr(), o.n.data_ptr(), o.h.data_ptr(), stream=stream.cuda_stream)

    grouped()
    loop()
    torch.cuda.synchronize()
    (scan if exhaustive else graph).status()
    for f in range(F):  # the same bytes
        for a, b in zip(out.rows(idx[f]), sub_out[f].rows(slice(None))):
            assert torch.equal(a, b), ("grouped launch differs from the loop", f)
    best = best_of({"grouped": grouped, "loop": loop})
    grouped()
    torch.cuda.synchronize()
    handle = scan if exhaustive else graph
    best["geometry"] = handle.launch_geometry()
    # stages of the grouped launch: fnv_last_kernel_ms brackets the search kernel (the scan and its merge); what precedes it on
    # the stream -- the filter rows, for the scan also the grouping -- is the rest of one launch timed alone
    alone = min(once(grouped, 1) for _ in range(5))
    best["kernel_ms"] = handle.last_kernel_ms()
    best["prepare_ms"] = alone - best["kernel_ms"]
    loop()
    torch.cuda.synchronize()
    best["loop_last_kernel_ms"] = handle.last_kernel_ms()  # the search kernel of the loop's last launch
    return best


results = {}
for how in ("random", "contiguous"):
    labels = rng.permutation(N) if how == "random" else np.arange(N)
    sets = [np.sort(labels[f * (N // 100):(f + 1) * (N // 100)]) for f in range(100)]
    r = tenants(sets, exhaustive=True)
    results["tenants_exhaustive_" + how] = r
    print("tenants, exhaustive, %-10s labels: grouped %9.3f ms  loop of 100 %9.3f ms  grouped/loop %.3f  %s  %s"
          % (how, r["grouped"], r["loop"], r["grouped"] / r["loop"], "PASS" if r["grouped"] <= r["loop"] else "FAIL", r["geometry"]), flush=True)
    print("    grouped launch alone: filter rows + grouping %.3f ms, scan + merge %.3f ms; the loop's last launch: scan + merge %.3f ms"
          % (r["prepare_ms"], r["kernel_ms"], r["loop_last_kernel_ms"]), flush=True)
print("  contiguous / random, grouped launch: %.3f (the cost of cutting segments by node range)"
      % (results["tenants_exhaustive_contiguous"]["grouped"] / results["tenants_exhaustive_random"]["grouped"]), flush=True)

labels = rng.permutation(N)
r = tenants([np.sort(labels[f * (N // 10):(f + 1) * (N // 10)]) for f in range(10)], exhaustive=False)
results["tenants_graph"] = r
print("tenants, graph ef=%d, 10 x 10 %%: grouped %9.3f ms  loop of 10 %9.3f ms  grouped/loop %.3f  %s  %s"
      % (EF, r["grouped"], r["loop"], r["grouped"] / r["loop"], "PASS" if r["grouped"] <= r["loop"] else "FAIL", r["geometry"]), flush=True)
print("    grouped launch alone: filter rows %.3f ms, search kernel %.3f ms; the loop's last launch: search kernel %.3f ms"
      % (r["prepare_ms"], r["kernel_ms"], r["loop_last_kernel_ms"]), flush=True)

tq = torch.from_numpy(Q).to(dev_t)
zeros = torch.zeros(NQ, dtype=torch.int32, device=dev_t)
for f in (1.0, 0.1, 0.01):
    rows = np.arange(N) if f >= 1 else np.sort(rng.choice(N, int(round(f * N)), replace=False))
    b, n_bits = hip.pack_allowed(rows)
    bits = torch.from_numpy(b).to(dev_t)
    a, s = Outputs(NQ), Outputs(NQ)

    def grouped():
        scan.search_device_exhaustive_grouped(tq.data_ptr(), NQ, K, bits.data_ptr(), 1, len(b), n_bits, zeros.data_ptr(), a.d.data_ptr(),
                                              a.l.data_ptr(), a.c.data_ptr(), a.n.data_ptr(), stream=stream.cuda_stream)

    def single():
        scan.search_device_exhaustive(tq.data_ptr(), NQ, K, s.d.data_ptr(), s.l.data_ptr(), s.c.data_ptr(), s.n.data_ptr(),
                                      bits_ptr=bits.data_ptr(), n_bits=n_bits, use_filter=True, stream=stream.cuda_stream)

    grouped()
    single()
    torch.cuda.synchronize()
    for x, y in zip(a.rows(slice(None)), s.rows(slice(None))):
        assert torch.equal(x, y), ("grouped scan differs from the single-filter scan", f)
    r = best_of({"grouped": grouped, "single": single})
    results["one_group_%g" % f] = r
    print("one group, f=%-5g: grouped scan %9.3f ms  single-filter scan %9.3f ms  grouped/single %.3f"
          % (f, r["grouped"], r["single"], r["grouped"] / r["single"]), flush=True)

if args.json:
    json.dump(results, open(args.json, "w"), indent=1)
