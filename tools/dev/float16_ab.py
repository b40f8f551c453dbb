#!/usr/bin/env python3
"""Developer tool: float32 vs float16 rows on the SAME graph, in ONE process (alternating timed rounds, as knob_sweep.py does).

  python tools/dev/float16_ab.py --config c3-lowrank [--n 2000000] [--ef 200,700] [--rounds 3] [--json out.json]

Builds the configuration's graph once in float32 with bench.py's generator and the device builder, then uploads a float16
device index with the same links (the host node store with its data section narrowed, numpy round-to-nearest-even).  For
every ef: fnv_tune on each index, then `--rounds` x (f32 round, f16 round) of `--steps` timed launches over rotating query
batches (HIP events on the launch stream).  Prints per (ef, dtype): kernel ms of each round, queries/s of the best round,
algorithmic TB/s with that dtype's row bytes, recall@10 against the exact top-k of the ORIGINAL float32 data, and the launch
geometry (fnv_last_launch_geometry, fnv_last_launch_info).
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

import bench  # noqa: E402
import flatnav_amd as flatnav  # noqa: E402
from flatnav_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--ef", default="")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--nb", type=int, default=4)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--json", default="")
args = ap.parse_args()

cfg = dict(bench.CONFIGS[args.config])
N = args.n or cfg["n"]
NQ, NB, K, M, DIM, METRIC = args.nq, args.nb, 10, 32, cfg["dim"], cfg["metric"]
dev_t = torch.device("cuda", 0)
torch.cuda.set_device(0)
t0 = time.time()
data = bench.Data(cfg, N, NQ * NB, torch, dev_t)
index = flatnav.index.create(distance_type=METRIC, index_data_type=flatnav.data_type.DataType.float32, dim=DIM,
                             dataset_size=N, max_edges_per_node=M)
index.set_num_threads(16)
index.set_device(0)
for first, xh in data.chunks(1_000_000 if DIM > 256 else 5_000_000):
    index.add(data=xh, ef_construction=100, labels=list(range(first, first + len(xh))), device=True)
print("# %s N=%d dim=%d %s: float32 graph built in %.1fs" % (args.config, N, DIM, METRIC, time.time() - t0), flush=True)
d32 = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)

# the float16 index: the same node records, data section narrowed (2 * dim bytes), links and labels copied
t0 = time.time()
ns32 = index._node_size_bytes
ns16 = ns32 - 2 * DIM
src = np.asarray(index._raw_blob())[: N * ns32].reshape(N, ns32)
blob16 = np.empty((N, ns16), np.uint8)
for s in range(0, N, 1_000_000):
    e = min(N, s + 1_000_000)
    blob16[s:e, : 2 * DIM] = src[s:e, : 4 * DIM].copy().view(np.float32).astype(np.float16).view(np.uint8)
    blob16[s:e, 2 * DIM:] = src[s:e, 4 * DIM:]
d16 = hip.DeviceIndex.upload(blob16.reshape(-1), ns16, 2 * DIM, M, N, "float16", METRIC, DIM, device=0)
del blob16, src
print("# float16 copy uploaded in %.1fs: row_bytes %d | %d (f32 %d | %d)"
      % (time.time() - t0, d16.row_bytes, d16.tail_bytes, d32.row_bytes, d32.tail_bytes), flush=True)

Q = data.queries()
dq = {"float32": torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32).reshape(NB, NQ, DIM)).to(dev_t)}
dq["float16"] = dq["float32"].half()
DEVS = {"float32": d32, "float16": d16}
ESIZE = {"float32": 4, "float16": 2}
od = torch.empty((NQ, K), dtype=torch.float32, device=dev_t)
ol = torch.empty((NQ, K), dtype=torch.int32, device=dev_t)
nd = torch.zeros(NQ, dtype=torch.int64, device=dev_t)
nh = torch.zeros(NQ, dtype=torch.int64, device=dev_t)
stream = torch.cuda.current_stream()
gt = bench.exact_topk(torch, d32, dq["float32"][0], K, N, DIM, "float32", METRIC)  # the original float32 rows
step_nodes = max(1, N // 100)
n_scan = (N + step_nodes - 1) // step_nodes


def timed(dt, ef, steps):
    dev, evs = DEVS[dt], []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        dev.search_device(dq[dt][i % NB].data_ptr(), NQ, K, ef, 100, od.data_ptr(), ol.data_ptr(), 0, nd.data_ptr(),
                          nh.data_ptr(), stream=stream.cuda_stream)
        b.record(stream)
        evs.append((a, b))
    torch.cuda.synchronize()
    dev.status()
    return float(np.mean([a.elapsed_time(b) for a, b in evs]))


out = []
efs = [int(x) for x in args.ef.split(",")] if args.ef else sorted(set([100] + list(cfg.get("secondary") or [])))
for ef in efs:
    res = {}
    for dt in DEVS:
        DEVS[dt].tune(int(dq[dt][0].data_ptr()), K, ef, 100, nq=NQ)
    for rnd in range(args.rounds):
        for dt in DEVS:
            dev = DEVS[dt]
            timed(dt, ef, 2)
            ms = timed(dt, ef, args.steps)
            r = res.setdefault(dt, dict(ms=[]))
            r["ms"].append(round(ms, 4))
            if rnd == 0:
                r["bytes"] = float(((n_scan + nd.cpu().numpy()) * DIM * ESIZE[dt] + nh.cpu().numpy() * M * 4 + K * 4).sum())
                r["geom"], r["info"] = dev.launch_geometry(), dev.launch_info()
                dev.search_device(dq[dt][0].data_ptr(), NQ, K, ef, 100, od.data_ptr(), ol.data_ptr(), stream=stream.cuda_stream)
                torch.cuda.synchronize()
                r["recall"] = float((ol.long().unsqueeze(2) == gt.unsqueeze(1)).any(dim=2).float().mean().item())
    for dt in DEVS:
        r = res[dt]
        best = min(r["ms"])
        g = r["geom"]
        print("ef=%d %-8s ms %s  best %.0f q/s  %.2f TB/s alg  recall@10 %.4f  per_cu %s lds %s vis %s cand %s %s var %s"
              % (ef, dt, r["ms"], NQ / best * 1e3, r["bytes"] / best / 1e9, r["recall"], g.get("blocks_per_cu"),
                 g.get("lds_bytes"), g.get("visited_slots"), g.get("cand_slots"), g.get("kernel"), r["info"]["variant"]),
              flush=True)
        out.append(dict(config=args.config, n=N, ef=ef, dtype=dt, qps=NQ / best * 1e3, **r))
    print("ef=%d float16 / float32 q/s: %.3f" % (ef, min(res["float32"]["ms"]) / min(res["float16"]["ms"])), flush=True)
if args.json:
    json.dump(out, open(args.json, "w"), indent=1, default=str)
