"""What a call and a query pay around the hops changes no result (csrc/launch.hip next_dispenser_block, csrc/kernels.hpp
next_query / clear_next_dispenser): a search launch owns one of the handle's two dispenser blocks and zeroes the other from its
kernel, the host memsets a block only where that clear is not ordered against the launch (the first launch, another stream, after
an exhaustive search), and the library's events bracket a launch only where somebody reads them.

A 20 000 x 64 sift-like float32 index (64-d: the narrowest rows that have a half-width mirror -- 32-d float32 rows are the {8, 1}
row configuration, which has none -- searched at G = 8, CU = 2) and the same data as uint8, M = 16, K = 10, ef = 20 and 64,
against the oracle bit for bit: labels, distance bits, counts, n_dist, n_hops.
  * launch sizes around a small grid (`blocks_per_cu` = 1): 1, slots - 1, slots, slots + 1, 2 slots, 2 slots + 1, 2.44 slots, for
    every pinned kernel variant 0-6 (exact shadows and tail shadows change the number of work items) and the filtered kernel;
  * five launches back to back without a sync on one handle, on one stream, alternating between two streams (the case that keeps
    its memset), and with an exhaustive call and a one-node device insertion in the middle;
  * hand-over counters: what the handle reports after two launches back to back is the second launch's own count."""
import ctypes
import os

import numpy as np
import pytest

from flatnav_amd import datasets as ds
from flatnav_amd import hip

pytestmark = pytest.mark.gpu
N, DIM, M, K, EFC = 20000, 64, 16, 10, 64
EFS = (20, 64)
THREADS = min(16, os.cpu_count() or 1)
_WORLDS = {}


class World:
    """One device-built index of the shared data, its oracle twin, a pool of queries and the oracle's answers per ef."""

    def __init__(self, dtype, n=N, capacity=None):
        import flatnav_amd
        from oracle import oracle as orc

        assert hip.device_count() >= 1, "no MI355X visible"
        orc.build()
        self.orc, self.dtype, self.n = orc, dtype, n
        X, Q = ds.sift_like(N, 2048, dim=DIM)
        self.X, self.Q = X[:n].astype(dtype), Q.astype(dtype)
        self.capacity = capacity or n
        self.index = flatnav_amd.index.create("l2", DIM, self.capacity, M, getattr(flatnav_amd.data_type.DataType, dtype))
        self.index.set_num_threads(4)
        self.index.add(self.X, EFC, labels=list(range(n)), device=True)
        self.dev = hip.DeviceIndex(ctypes.c_void_p(self.index.device_handle()), owned=False)
        self.node_size = np.asarray(self.index._raw_blob()).size // self.capacity
        self.twin(n)
        self.dev.set_option("blocks_per_cu", 1)  # a small grid: a few hundred queries are several rounds of it
        self.dev.search(self.Q, K, 64)
        self.slots = self.dev.launch_geometry()["grid_blocks"]
        assert 64 <= self.slots <= 400, self.slots

    def twin(self, live):
        blob = np.asarray(self.index._raw_blob()).reshape(-1)[: live * self.node_size]
        self.oracle = self.orc.OracleIndex.from_blob("l2", self.dtype, DIM, live, live, M, blob)
        self._want = {}

    def want(self, ef, lo=0, hi=None):
        if ef not in self._want:
            self._want[ef] = self.oracle.search(self.Q, K, ef, threads=THREADS, stats=True)
        d, l, st = self._want[ef]
        return d[lo:hi], l[lo:hi], {k: v[lo:hi] for k, v in st.items()}

    def pin(self, variant):
        self.dev.set_option("sorted_beam", 0 if variant == 0 else 1)
        self.dev.set_option("sorted_variant", -1 if variant == 0 else variant)


def world(dtype):
    if dtype not in _WORLDS:
        _WORLDS[dtype] = World(dtype)
    return _WORLDS[dtype]


def _same(got, want, what):
    (gd, gl, gst), (wd, wl, wst) = got, want
    assert np.array_equal(gl, wl), "%s: labels differ in %d queries" % (what, int((gl != wl).any(axis=1).sum()))
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), "%s: distance bits differ" % (what,)
    for k in ("count", "n_dist", "n_hops"):
        assert np.array_equal(gst[k], wst[k]), (what, k)


def _sizes(s):
    return (1, s - 1, s, s + 1, 2 * s, 2 * s + 1, int(2.44 * s))


@pytest.mark.parametrize("variant", range(7))
def test_launch_sizes_against_the_grid(variant):
    w = world("float32")
    w.pin(variant)
    seen = set()
    for ef in EFS:
        for nq in _sizes(w.slots):
            got = w.dev.search(w.Q[:nq], K, ef, stats=True)
            info, geom = w.dev.launch_info(), w.dev.launch_geometry()
            assert w.dev.half_rows()["used_by_last_launch"], (variant, ef, nq)
            assert geom["grid_blocks"] == (2 * nq if info["shadow"] else min(nq, w.slots)), (variant, ef, nq, geom, info)
            seen.add((info["variant_id"], info["shadow"]))
            _same(got, w.want(ef, 0, nq), ("variant", variant, "ef", ef, "nq", nq))
    assert (variant, False) in seen, seen  # the multi-round launches ran what was pinned ...
    assert variant == 0 or any(shadow for _, shadow in seen), seen  # ... and the one-query launch had its exact shadow


def test_launch_sizes_against_the_grid_filtered_and_uint8():
    w = world("float32")
    everything = np.ones(N, dtype=np.bool_)
    for ef in EFS:
        for nq in _sizes(w.slots):
            got = w.dev.search_filtered(w.Q[:nq], K, ef, everything, stats=True)
            assert w.dev.launch_geometry()["kernel"] == "two_heaps"
            _same(got, w.want(ef, 0, nq), ("filtered", ef, nq))  # (every label allowed: the unfiltered answers)
    u = world("uint8")
    u.pin(1)
    for ef in EFS:
        for nq in _sizes(u.slots):
            _same(u.dev.search(u.Q[:nq], K, ef, stats=True), u.want(ef, 0, nq), ("uint8", ef, nq))


class Batches:
    """Five batches of the pool with output buffers of their own, on the device."""

    def __init__(self, w, torch):
        s = w.slots
        self.cuts = np.cumsum([0, s + 1, int(2.44 * s) - s, 37, 2 * s - 40, s - 1])
        assert self.cuts[-1] <= len(w.Q)
        cuda = torch.device("cuda", 0)
        self.q = [torch.from_numpy(np.ascontiguousarray(w.Q[a:b])).to(cuda) for a, b in zip(self.cuts[:-1], self.cuts[1:])]
        self.out = [(torch.empty((len(q), K), dtype=torch.float32, device=cuda), torch.empty((len(q), K), dtype=torch.int32, device=cuda),
                     torch.empty(len(q), dtype=torch.int32, device=cuda), torch.empty(len(q), dtype=torch.int64, device=cuda),
                     torch.empty(len(q), dtype=torch.int64, device=cuda)) for q in self.q]

    def launch(self, w, i, ef, stream):
        q, o = self.q[i], self.out[i]
        w.dev.search_device(q.data_ptr(), len(q), K, ef, 100, *[t.data_ptr() for t in o], stream=stream.cuda_stream)

    def result(self, i):
        d, l, c, nd, nh = [t.cpu().numpy() for t in self.out[i]]
        return d, l, {"count": c, "n_dist": nd, "n_hops": nh}

    def check(self, w, i, ef, what):
        _same(self.result(i), w.want(ef, self.cuts[i], self.cuts[i + 1]), (what, "launch", i))


@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("streams", ["one stream", "two streams"])
def test_five_launches_back_to_back(ef, streams):
    import torch
    w = world("float32")
    w.pin(1)
    b = Batches(w, torch)
    pool = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for i in range(5):
        s = pool[i % 2 if streams == "two streams" else 0]
        if i and streams == "two streams":
            s.wait_stream(pool[(i - 1) % 2])  # one launch in flight per handle: ordered on the device, no host sync
        b.launch(w, i, ef, s)
    torch.cuda.synchronize()
    w.dev.status()
    for i in range(5):
        b.check(w, i, ef, (streams, ef))


def test_exhaustive_call_and_device_insertion_between_launches():
    import torch
    n = 5000
    w = World("float32", n=n, capacity=n + 1)
    w.pin(1)
    b = Batches(w, torch)
    cuda = torch.device("cuda", 0)
    s = torch.cuda.Stream()
    ef = 20
    # the exhaustive search's own answer: exact integer distances, ties by node id (labels are node ids)
    xq = w.Q[:64]
    d2 = ((xq.astype(np.float64)[:, None, :] - w.X.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    order = np.lexsort((np.broadcast_to(np.arange(n), d2.shape), d2), axis=1)[:, :K]
    tq = torch.from_numpy(np.ascontiguousarray(xq)).to(cuda)
    td, tl = torch.empty((64, K), dtype=torch.float32, device=cuda), torch.empty((64, K), dtype=torch.int32, device=cuda)
    torch.cuda.synchronize()
    b.launch(w, 0, ef, s)
    b.launch(w, 1, ef, s)
    w.dev.search_device_exhaustive(tq.data_ptr(), 64, K, td.data_ptr(), tl.data_ptr(), stream=s.cuda_stream)
    b.launch(w, 2, ef, s)
    torch.cuda.synchronize()
    w.dev.status()
    for i in range(3):
        b.check(w, i, ef, "around the exhaustive call")
    assert np.array_equal(tl.cpu().numpy(), order.astype(np.int32))
    assert np.array_equal(td.cpu().numpy(), np.take_along_axis(d2, order, axis=1).astype(np.float32))
    # one node more, wired on the device; the launches after it see it
    w.index.add(ds.sift_like(N, 2048, dim=DIM)[0][n:n + 1], EFC, labels=[n], device=True)
    w.twin(n + 1)
    b.launch(w, 3, ef, s)
    b.launch(w, 4, ef, s)
    torch.cuda.synchronize()
    w.dev.status()
    for i in (3, 4):
        b.check(w, i, ef, "after the insertion")


def test_hand_over_counters_are_the_last_launch_s_own():
    import torch
    w = world("uint8")
    w.pin(1)  # every query through the merged beam: the tied ones are handed over
    b = Batches(w, torch)
    s = torch.cuda.Stream()
    alone = []
    for i in range(5):
        torch.cuda.synchronize()
        b.launch(w, i, 64, s)
        alone.append((w.dev.replayed_queries(), w.dev.handover_stats()))  # (both wait for the launch)
        b.check(w, i, 64, "alone")
    totals = [r["total"] for r, _ in alone]
    assert max(totals) > 0, totals
    pairs = [(i, j) for i in range(5) for j in range(5) if totals[i] != totals[j]]
    assert pairs, totals  # tie-dense data: the batches do not all hand over the same number of queries
    for i, j in pairs[:4]:
        torch.cuda.synchronize()
        b.launch(w, i, 64, s)
        b.launch(w, j, 64, s)
        assert (w.dev.replayed_queries(), w.dev.handover_stats()) == alone[j], (i, j, alone)
        w.dev.status()
        b.check(w, i, 64, "first of two")
        b.check(w, j, 64, "second of two")
