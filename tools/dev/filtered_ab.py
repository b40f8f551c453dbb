#!/usr/bin/env python3
"""Developer tool: filtered search (fnv_search_batch_filtered_device) against the unfiltered search on ONE c2-like graph.

  python tools/dev/filtered_ab.py [--n 1000000] [--ef 52,200] [--rounds 3] [--steps 5] [--json out.json]

Builds the SIFT-1M stand-in (flatnav_amd.datasets.sift_like, labels = row numbers) with the device builder, then for every ef
times `--rounds` rounds of `--steps` launches of `--nq` device-resident queries (HIP events on the launch stream; the best round
counts) for:
  default      the unfiltered search as a caller gets it (adaptive kernel choice, settled by fnv_tune)
  k1           the unfiltered search pinned to the two-heap kernel (sorted_beam = 0, on a view of the same index)
  f=<frac> random / contiguous   filtered searches with that fraction of the labels allowed (a random set; a label range)
and the recall@10 of each against the brute-force top 10 over the ALLOWED rows only (torch on the GPU).  Filtered searches
run on their own view with spill_entries = 2^18: a 1 % filter keeps the candidates heap growing until 200 allowed nodes are
in the beam, past the default 16384-entry spill area (FNV_ERR_CAPACITY).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flatnav_amd as flatnav  # noqa: E402
from flatnav_amd import datasets as ds  # noqa: E402
from flatnav_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--ef", default="52,200")
ap.add_argument("--fractions", default="1,0.5,0.1,0.01")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--json", default="")
args = ap.parse_args()

N, NQ, K, M, DIM = args.n, args.nq, 10, 32, 128
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
k1 = base.view()
k1.set_option("sorted_beam", 0)
filt = base.view()
filt.set_option("spill_entries", 1 << 18)

tq = torch.from_numpy(Q).to(dev_t)
tx = torch.from_numpy(X).to(dev_t)
xn = (tx.double() ** 2).sum(1)
od = torch.empty((NQ, K), dtype=torch.float32, device=dev_t)
ol = torch.empty((NQ, K), dtype=torch.int32, device=dev_t)
cnt = torch.empty(NQ, dtype=torch.int32, device=dev_t)
stream = torch.cuda.current_stream()
rng = np.random.default_rng(1)


def truth(rows):
    """Labels of the brute-force top K over X[rows] (float64 on the GPU)."""
    r = torch.from_numpy(rows).to(dev_t)
    out = torch.empty((NQ, K), dtype=torch.int64, device=dev_t)
    xs, xsn = tx[r].double(), xn[r]
    for s in range(0, NQ, 1000):
        d = xsn[None, :] - 2.0 * (tq[s:s + 1000].double() @ xs.T)
        out[s:s + 1000] = r[torch.topk(d, K, dim=1, largest=False).indices]
    return out


def launch(kind, ef, bits=None, n_bits=0):
    if kind == "default":
        base.search_device(tq.data_ptr(), NQ, K, ef, 100, od.data_ptr(), ol.data_ptr(), cnt.data_ptr(), stream=stream.cuda_stream)
    elif kind == "k1":
        k1.search_device(tq.data_ptr(), NQ, K, ef, 100, od.data_ptr(), ol.data_ptr(), cnt.data_ptr(), stream=stream.cuda_stream)
    else:
        filt.search_device_filtered(tq.data_ptr(), NQ, K, ef, 100, bits.data_ptr() if n_bits else 0, n_bits, od.data_ptr(),
                                    ol.data_ptr(), cnt.data_ptr(), stream=stream.cuda_stream)


def timed(kind, ef, bits=None, n_bits=0):
    best = None
    for _ in range(args.rounds):
        launch(kind, ef, bits, n_bits)  # warm
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.steps):
            launch(kind, ef, bits, n_bits)
        b.record(stream)
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / args.steps
        best = ms if best is None else min(best, ms)
    for h in (base, k1, filt):
        h.status()
    return best


rows_all = np.arange(N)
filters = []
for f in [float(x) for x in args.fractions.split(",")]:
    k = max(1, int(round(f * N)))
    if f >= 1:
        filters.append(("f=1", rows_all))
        continue
    filters.append(("f=%g random" % f, np.sort(rng.choice(N, k, replace=False))))
    start = int(rng.integers(0, N - k + 1))
    filters.append(("f=%g contiguous" % f, np.arange(start, start + k)))

out = []
for ef in [int(x) for x in args.ef.split(",")]:
    base.tune(int(tq.data_ptr()), K, ef, 100, nq=NQ)
    gt_all = truth(rows_all)
    cases = [("default", None, gt_all), ("k1", None, gt_all)] + [(name, rows, None) for name, rows in filters]
    ref_ms = None
    for name, rows, gt in cases:
        bits = None
        n_bits = 0
        kind = name
        if rows is not None:
            kind = "filtered"
            b, n_bits = hip.pack_allowed(rows)
            bits = torch.from_numpy(b).to(dev_t)
            gt = truth(rows)
        ms = timed(kind, ef, bits, n_bits)
        launch(kind, ef, bits, n_bits)
        torch.cuda.synchronize()
        recall = float((ol.long().unsqueeze(2) == gt.unsqueeze(1)).any(dim=2).float().mean().item())
        short = int((cnt < K).sum().item())
        if name == "default":
            ref_ms = ms
        qps = NQ / ms * 1e3
        print("ef=%-4d %-20s %8.3f ms  %10.0f q/s  %.3f x default  recall@10 %.4f  short rows %d"
              % (ef, name, ms, qps, ref_ms / ms, recall, short), flush=True)
        out.append(dict(ef=ef, case=name, ms=ms, qps=qps, vs_default=ref_ms / ms, recall=recall, short_rows=short,
                        info=(base if kind == "default" else k1 if kind == "k1" else filt).launch_info()["variant"]))
if args.json:
    json.dump(out, open(args.json, "w"), indent=1)
