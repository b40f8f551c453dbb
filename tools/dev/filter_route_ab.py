#!/usr/bin/env python3
"""Developer tool: filter routing ("filter_scan_max" / "filter_scan_on_overflow") on a tenant mix, against the two calls a caller
had before it -- everything through the graph form, everything through the scan form -- on ONE c2-like graph, in one process,
alternating.

  python tools/dev/filter_route_ab.py [--n 1000000] [--nq 10000] [--rounds 2] [--steps 2] [--json out.json]

Builds the SIFT-1M stand-in of tools/dev/exhaustive_ab.py (labels = row numbers) with the device builder.  The batch mixes
tenants whose filters allow 0.01 %, 0.1 %, 1 %, 5 %, 10 %, 20 % and 50 % of the labels (random subsets), the same number of queries
each, in shuffled order.  Timed with HIP events on the launch stream, `--rounds` rounds of `--steps` repetitions, the best round
counting, the sides alternating per round:
  per tenant class      its queries alone through fnv_search_batch_filtered_grouped_device (ef = 52, a spill area that holds the
                        whole graph) and through fnv_search_batch_exhaustive_grouped_device: where the two cross
  the whole batch       all-graph, all-scan, and routed at a threshold between every two classes (the threshold is a node count)
  the safety net        the library's default spill area, no threshold: all-graph (which may end in FNV_ERR_CAPACITY) against
                        overflow routing alone
Before it is timed, every routed launch is checked: n_hops = 0 exactly on the rows whose filter is at or below the threshold,
those rows equal the all-scan call's and the others the all-graph call's, byte for byte.
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
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--json", default="")
args = ap.parse_args()

N, NQ, K, M, DIM, EF = args.n, args.nq, 10, 32, 128, 52
FRACTIONS = (0.0001, 0.001, 0.01, 0.05, 0.1, 0.2, 0.5)
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
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)


def handle(spill, scan_max=0, on_overflow=0):
    h = base.view()
    h.set_option("spill_entries", spill)
    h.set_option("filter_scan_max", scan_max)
    h.set_option("filter_scan_on_overflow", on_overflow)
    return h


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

    def rows(self, idx, hops=True):
        return [t[idx] for t in (self.d.view(torch.int32), self.l, self.c, self.n) + ((self.h,) if hops else ())]


counts = [max(1, int(round(f * N))) for f in FRACTIONS]
sets = [np.sort(rng.choice(N, c, replace=False)) for c in counts]
F = len(sets)
table, n_bits = hip.pack_filters(sets)
stride = table.shape[1]
tt = torch.from_numpy(table).to(dev_t)
qf = rng.permutation(np.arange(NQ) % F).astype(np.int32)
tqf = torch.from_numpy(qf).to(dev_t)
tq = torch.from_numpy(Q).to(dev_t)
BIG = 1 << 20  # spill entries per query slot: a candidates heap that holds every node of the graph


def graph_call(h, q, nq, f, out):
    return lambda: h.search_device_filtered_grouped(q.data_ptr(), nq, K, EF, 100, tt.data_ptr(), F, stride, n_bits, f.data_ptr(),
                                                    out.d.data_ptr(), out.l.data_ptr(), out.c.data_ptr(), out.n.data_ptr(),
                                                    out.h.data_ptr(), stream=stream.cuda_stream)


def scan_call(h, q, nq, f, out):
    return lambda: h.search_device_exhaustive_grouped(q.data_ptr(), nq, K, tt.data_ptr(), F, stride, n_bits, f.data_ptr(), out.d.data_ptr(),
                                                      out.l.data_ptr(), out.c.data_ptr(), out.n.data_ptr(), stream=stream.cuda_stream)


def status_of(h):
    torch.cuda.synchronize()
    try:
        h.status()
        return "ok"
    except RuntimeError as e:
        return "FNV_ERR_CAPACITY" if "spill" in str(e) else repr(e)


results = {"fractions": FRACTIONS, "counts": counts, "nq": NQ, "n": N, "ef": EF}
graph, scan = handle(BIG), handle(16384)  # (one handle for the graph form and the routed calls: the spill area is 8 MB per query slot)


def routed_call(T, call):
    """The graph handle's call at threshold T (0: the plain graph form); an option change is a mutex and a store."""
    def run():
        graph.set_option("filter_scan_max", T)
        call()
    return run


# ---- per tenant class: where the graph form and the scan form cross ----------------------------------------------------------------
per_class = []
for g, (frac, count) in enumerate(zip(FRACTIONS, counts)):
    idx = torch.from_numpy(np.flatnonzero(qf == g)).to(dev_t)
    q, f = tq[idx].contiguous(), tqf[idx].contiguous()
    og, osc = Outputs(len(idx)), Outputs(len(idx))
    sides = {"graph": routed_call(0, graph_call(graph, q, len(idx), f, og)), "scan": scan_call(scan, q, len(idx), f, osc)}
    sides["graph"]()
    st = status_of(graph)
    r = best_of(sides if st == "ok" else {"scan": sides["scan"]})
    r.update(fraction=frac, allowed=count, queries=len(idx), graph_status=st)
    per_class.append(r)
    print("class %7.4f %% (%7d nodes, %5d queries): graph %10.3f ms  scan %9.3f ms  graph/scan %8.2f  %s"
          % (100 * frac, count, len(idx), r.get("graph", float("nan")), r["scan"], r.get("graph", float("nan")) / r["scan"], st), flush=True)
results["per_class"] = per_class

# ---- the whole batch: all-graph, all-scan, routed at every threshold ------------------------------------------------------------------
out_g, out_s = Outputs(NQ), Outputs(NQ)
all_graph, all_scan = routed_call(0, graph_call(graph, tq, NQ, tqf, out_g)), scan_call(scan, tq, NQ, tqf, out_s)
all_graph()
graph_status = status_of(graph)
all_scan()
torch.cuda.synchronize()
sides = {"all_scan": all_scan}
if graph_status == "ok":
    sides["all_graph"] = all_graph
allowed_of = torch.from_numpy(np.asarray(counts, np.int64)[qf]).to(dev_t)
for T in counts:
    o = Outputs(NQ)
    call = routed_call(T, graph_call(graph, tq, NQ, tqf, o))
    call()
    assert status_of(graph) == "ok", T
    scanned = allowed_of <= T
    assert torch.equal(o.h == 0, scanned), ("n_hops = 0 exactly on the rows at or below the threshold", T)
    for a, b in zip(o.rows(scanned, hops=False), out_s.rows(scanned, hops=False)):
        assert torch.equal(a, b), ("a scanned row differs from the scan form", T)
    if graph_status == "ok":
        for a, b in zip(o.rows(~scanned), out_g.rows(~scanned)):
            assert torch.equal(a, b), ("a graph row differs from the graph form", T)
    sides["routed_%d" % T] = call
r = best_of(sides)
r["all_graph_status"] = graph_status
results["whole_batch"] = r
for name in sides:
    print("whole batch, %-16s %10.3f ms" % (name, r[name]), flush=True)
best = min((k for k in r if k.startswith("routed_")), key=lambda k: r[k])
print("best threshold: %s (%.3f ms); all-scan / best %.2f; all-graph / best %s"
      % (best, r[best], r["all_scan"] / r[best], "%.2f" % (r["all_graph"] / r[best]) if "all_graph" in r else graph_status), flush=True)
for T in counts:
    sides["routed_%d" % T]()
    torch.cuda.synchronize()
    print("    routed_%d: both stages %.3f ms by the library's own events" % (T, graph.last_kernel_ms()), flush=True)
graph.set_option("filter_scan_max", 0)

# ---- the safety net: the default spill area ---------------------------------------------------------------------------------------------
plain, net = handle(16384), handle(16384, on_overflow=1)
out_p, out_n = Outputs(NQ), Outputs(NQ)
plain_call, net_call = graph_call(plain, tq, NQ, tqf, out_p), graph_call(net, tq, NQ, tqf, out_n)
plain_call()
plain_status = status_of(plain)
net_call()
assert status_of(net) == "ok"
handed = int((out_n.h == 0).sum().item())
for a, b in zip(out_n.rows(out_n.h == 0, hops=False), out_s.rows(out_n.h == 0, hops=False)):
    assert torch.equal(a, b), "a row handed over on overflow differs from the scan form"
r = best_of({"plain": plain_call, "overflow_routing": net_call})
r.update(plain_status=plain_status, handed_over=handed)
results["safety_net"] = r
print("default spill area: plain graph form %10.3f ms (%s); overflow routing alone %10.3f ms, %d of %d queries handed to the scan"
      % (r["plain"], plain_status, r["overflow_routing"], handed, NQ), flush=True)
by_class = {FRACTIONS[g]: int(((out_n.h == 0) & (tqf == g)).sum().item()) for g in range(F)}
print("    handed over per class: %s" % by_class, flush=True)
results["safety_net"]["handed_over_per_class"] = {str(k): v for k, v in by_class.items()}

if args.json:
    json.dump(results, open(args.json, "w"), indent=1, default=str)
