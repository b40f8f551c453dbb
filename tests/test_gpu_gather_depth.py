"""Gather depth of mirror rows, the double-buffered entry scan and the first work item of a slot (csrc/distance.hpp
gather_passes, csrc/kernels.hpp scan_rows / next_query): none of them changes a result.  On 20 000 x 128 float32 indexes of small
integers (lossless in binary16, so the mirror is live; tie-dense, so queries are handed over) searches that read the mirror return
the bytes of searches that read the float32 table and of the oracle -- labels, distance bits, result counts, n_dist, n_hops --
over beam widths, entry-scan lengths on both sides of a batch of 24 and of 32 rows, launch sizes around one and three rounds of
query slots, the pinned kernel variants and the small launches with exact shadows, for link rows of 32, 24 and 33."""
import ctypes
import os

import numpy as np
import pytest

from flatnav_amd import hip

pytestmark = pytest.mark.gpu
N, DIM, K, EFC = 20000, 128, 10, 64
THREADS = min(16, os.cpu_count() or 1)
_WORLDS = {}


class World:
    """One device-built index (link rows of M), its oracle twin, a pool of queries and the oracle's answers, computed once per
    (ef, entry-scan length) on the whole pool: every launch size is a prefix of it."""

    def __init__(self, M):
        import flatnav_amd

        assert hip.device_count() >= 1, "no MI355X visible"
        from oracle import oracle as orc

        orc.build()
        rng = np.random.default_rng(100 + M)
        self.M = M
        self.X = X = rng.integers(0, 4, (N, DIM)).astype(np.float32)
        self.index = flatnav_amd.index.create("l2", DIM, N, M)
        self.index.set_num_threads(4)
        self.index.add(X, EFC, labels=list(range(N)), device=True)
        self.dev = hip.DeviceIndex(ctypes.c_void_p(self.index.device_handle()), owned=False)
        st = self.dev.half_rows()
        assert st["state"] == "live" and st["rows"] == N, st
        self.oracle = orc.OracleIndex.from_blob("l2", "float32", DIM, N, N, M, np.asarray(self.index._raw_blob()))
        # the query slots of a full grid at ef = 52 (what the launches around one and three rounds are sized by)
        self.dev.search(rng.integers(0, 4, (8192, DIM)).astype(np.float32), K, 52)
        self.slots = self.dev.launch_geometry()["grid_blocks"]
        assert 1024 <= self.slots <= 8192, self.slots
        self.Q = rng.integers(0, 4, (3 * self.slots + 5, DIM)).astype(np.float32)
        self._want = {}

    def want(self, nq, ef, n_init):
        key = (ef, n_init)
        have = self._want.get(key)
        if have is None or len(have[1]) < nq:
            size = min(x for x in (2048, self.slots + 1, len(self.Q)) if x >= nq)
            have = self._want[key] = self.oracle.search(self.Q[:size], K, ef, n_init, threads=THREADS, stats=True)
        d, l, st = have
        return d[:nq], l[:nq], {k: v[:nq] for k, v in st.items()}

    def reset(self):
        for name, value in (("sorted_beam", 2), ("sorted_variant", -1), ("half_rows", 1)):
            self.dev.set_option(name, value)


def world(M):
    if M not in _WORLDS:
        _WORLDS[M] = World(M)
    w = _WORLDS[M]
    w.reset()
    return w


def _same(a, b, what):
    (ad, al, ast), (bd, bl, bst) = a, b
    assert np.array_equal(al, bl), "%s: labels differ in %d queries" % (what, int((al != bl).any(axis=1).sum()))
    assert np.array_equal(ad.view(np.uint32), bd.view(np.uint32)), "%s: distance bits differ" % (what,)
    for k in ("count", "n_dist", "n_hops"):
        assert np.array_equal(ast[k], bst[k]), (what, k)


def _pin(w, variant):
    w.dev.set_option("sorted_beam", 0 if variant == "two_heaps" else 1)
    if variant != "two_heaps":
        w.dev.set_option("sorted_variant", {"merged_beam": 1, "merged_beam_tail100": 4}[variant])


def _three_ways(w, nq, ef, n_init, what, pinned=True, Q=None):
    """Mirror on, mirror off, the oracle; returns the mirror launch's geometry, launch info and hand-over counters.  With the
    kernel variant pinned and no shadows racing the queries, the two launches have one shape and hand the same queries over.
    Q: queries of the test's own instead of the first nq of the pool."""
    dev = w.dev
    want = w.want(nq, ef, n_init) if Q is None else w.oracle.search(Q, K, ef, n_init, threads=THREADS, stats=True)
    Q = w.Q[:nq] if Q is None else Q
    dev.set_option("half_rows", 1)
    on = dev.search(Q, K, ef, n_init, stats=True)
    assert dev.half_rows()["used_by_last_launch"], what
    seen = dev.launch_geometry(), dev.launch_info(), dev.replayed_queries(), dev.handover_stats()
    dev.set_option("half_rows", 0)
    off = dev.search(Q, K, ef, n_init, stats=True)
    assert not dev.half_rows()["used_by_last_launch"], what
    if pinned and not seen[1]["shadow"]:
        assert (dev.replayed_queries(), dev.handover_stats()) == seen[2:], what  # the same queries tie, the same are resumed
        assert dev.launch_geometry() == seen[0], what
    dev.set_option("half_rows", 1)
    _same(on, off, (what, "mirror on / off"))
    _same(want, on, (what, "oracle"))
    return seen + (on,)


@pytest.mark.parametrize("ef", [10, 52, 100, 200])
def test_beam_widths_and_entry_scan_lengths(ef):
    # entry scans of 1 ... 100 rows: less than a batch, a batch of 24 (the float32 rows' three passes) and of 32 (the mirror's
    # four) to the row, one more, and the default's four batches; then the first row past the four batches that the
    # double-buffered scan runs as straight-line code, and many turns of its loop
    w = world(32)
    _pin(w, "merged_beam")
    for n_init in (1, 7, 24, 25, 32, 33, 100, 129, 1000):
        _three_ways(w, 2048, ef, n_init, ("M=32", ef, n_init))


@pytest.mark.parametrize("variant", ["two_heaps", "merged_beam", "merged_beam_tail100"])
def test_launch_sizes_around_the_query_slots(variant):
    w = world(32)
    s = w.slots
    _pin(w, variant)
    resumed = 0
    for nq in (1, 63, s - 1, s, s + 1, 3 * s + 5):
        geom, info, replayed, handed, _ = _three_ways(w, nq, 52, 100, (variant, nq))
        assert geom["kernel"] == ("two_heaps" if variant == "two_heaps" else "merged_beam_registers"), (variant, nq, geom)
        if variant != "two_heaps":  # (the two-heap layout keeps another number of slots resident)
            assert geom["grid_blocks"] == (min(nq, s) if not info["shadow"] else 2 * nq), (variant, nq, geom, info)
        if variant == "merged_beam_tail100" and nq > s:  # the whole last round goes straight to the exact search
            assert info["variant"] == variant and geom["tail_exact"] == s, (nq, info, geom)
        if variant == "merged_beam" and nq >= s - 1:  # every query through the merged beam: the tied ones come back from their logs
            assert handed["resumed"] > 0 and handed["resumed"] + handed["from_scratch"] == replayed["total"], (nq, replayed, handed)
            resumed += handed["resumed"]
    assert variant != "merged_beam" or resumed > 0


def test_small_launches_with_shadows():
    # few queries on a small index: every query has an exact shadow, the visited set is the DIRECT bitmap in LDS
    w = world(32)
    for nq in (1, 63, 500):
        for ef in (10, 52, 200):
            geom, info, _, _, _ = _three_ways(w, nq, ef, 100, ("small launch", nq, ef), pinned=False)
            assert info["shadow"] and geom["grid_blocks"] == 2 * nq, (nq, ef, geom, info)


@pytest.mark.parametrize("M", [24, 33])
def test_link_rows_of_three_passes_and_of_two_batches(M):
    # M = 24: a row fits the three passes the float32 form has; M = 33: one more than the mirror's four, the batch loop runs twice
    w = world(M)
    _pin(w, "merged_beam")
    for ef in (10, 52, 100, 200):
        for n_init in (1, 100):
            _three_ways(w, 2048, ef, n_init, ("M=%d" % M, ef, n_init))
    _, _, replayed, handed, _ = _three_ways(w, w.slots + 1, 52, 100, ("M=%d" % M, "merged beam, two rounds"))
    assert handed["resumed"] > 0, (replayed, handed)
    w.dev.set_option("sorted_beam", 0)
    _three_ways(w, 2048, 52, 100, ("M=%d" % M, "two heaps"))


def test_rows_with_more_than_24_new_neighbours_occur():
    # A query that IS a node's vector, with every node in the entry scan, starts at that node (distance 0), and the first hop
    # finds all the node's links unvisited.  For nodes with more than 24 links that hop's gather is the four-pass batch, and the
    # query's n_dist counts at least those rows -- in the oracle and, bit for bit, on the GPU.
    w = world(32)
    links = np.asarray(w.dev.read_links(0, N)).reshape(N, -1).astype(np.int64)
    own = np.arange(N)[:, None]
    srt = np.sort(np.where((links == own) | (links < 0) | (links >= N), -1, links), axis=1)  # (unused slots hold the node itself)
    degree = ((srt >= 0) & np.concatenate([np.ones((N, 1), bool), srt[:, 1:] != srt[:, :-1]], axis=1)).sum(axis=1)
    _, first, counts = np.unique(w.X, axis=0, return_index=True, return_counts=True)
    unique = np.zeros(N, bool)
    unique[first[counts == 1]] = True
    nodes = np.flatnonzero((degree > 24) & unique)[:256]
    assert len(nodes) > 0, "no node of this index has more than 24 links: %s" % np.bincount(degree)
    _pin(w, "merged_beam")
    *_, on = _three_ways(w, len(nodes), 10, N, "ef=10 from nodes with more than 24 links", Q=w.X[nodes])
    n_dist, n_hops = on[2]["n_dist"], on[2]["n_hops"]
    assert np.array_equal(on[1][:, 0], nodes) and (on[0][:, 0] == 0).all()  # each query found its own node
    assert (n_dist.astype(np.int64) >= degree[nodes]).all() and (n_hops >= 1).all()
    assert (n_dist.astype(np.int64) > 24).all()
