"""The half-width mirror of float32 rows on the GPU (include/flatnav_hip.h, csrc/half_rows.hpp): searches that read it return the
bytes of searches that read the float32 table -- distances as uint32, labels, result counts, n_dist and n_hops -- for float32
queries that binary16 does NOT represent, in every kernel form; the mirror follows the rows as they are written, is dropped
(and its memory returned) by the first value that is not lossless, and is seen by views, rebuilt for replicas and built on
request for handles whose rows the library did not write."""
import ctypes
import os

import numpy as np
import pytest

from flatnav_amd import hip

pytestmark = pytest.mark.gpu
N, M, K, EFC = 3000, 16, 10, 48
EFS = (16, 100, 200, 300)  # beams of one / two / four register chunks, and the LDS form


@pytest.fixture(scope="module")
def flatnav():
    import flatnav_amd

    assert hip.device_count() >= 1, "no MI355X visible"
    return flatnav_amd


def _lossless_rows(rng, n, dim):
    X = rng.normal(size=(n, dim)).astype(np.float16).astype(np.float32)
    X[5, 0], X[6, 1], X[7, 2], X[8, 3] = 65504.0, -65504.0, 2.0 ** -24, -0.0
    return X


def _build(flatnav, metric, X, batches=1):
    """Device-built index -> (index, handle of its device buffers)."""
    ix = flatnav.index.create(metric, X.shape[1], len(X), M)
    ix.set_num_threads(4)
    edges = np.linspace(0, len(X), batches + 1).astype(int)
    for a, b in zip(edges[:-1], edges[1:]):
        ix.add(X[a:b], EFC, labels=list(range(a, b)), device=True)
    return ix, hip.DeviceIndex(ctypes.c_void_p(ix.device_handle()), owned=False)


def _search(dev, Q, K, ef, half, **kw):
    dev.set_option("half_rows", half)
    got = dev.search(Q, K, ef, stats=True, **kw)
    return got, dev.half_rows()["used_by_last_launch"]


def _same(a, b, what):
    (ad, al, ast), (bd, bl, bst) = a, b
    assert np.array_equal(al, bl), "%s: labels differ in %d queries" % (what, int((al != bl).any(axis=1).sum()))
    assert np.array_equal(ad.view(np.uint32), bd.view(np.uint32)), "%s: distance bits differ" % (what,)
    for k in ("count", "n_dist", "n_hops"):
        assert np.array_equal(ast[k], bst[k]), (what, k)


@pytest.mark.parametrize("metric", ["l2", "angular"])
@pytest.mark.parametrize("dim", [64, 120, 128, 256, 512, 1024, 2048])
def test_mirror_on_equals_mirror_off_in_every_kernel_form(flatnav, dim, metric):
    rng = np.random.default_rng(dim + (metric == "l2"))
    X = _lossless_rows(rng, N, dim)
    Q = rng.normal(size=(256, dim)).astype(np.float32)
    assert not np.array_equal(Q, Q.astype(np.float16).astype(np.float32))  # the queries are plain float32
    ix, dev = _build(flatnav, metric, X)
    st = dev.half_rows()
    assert st["state"] == "live" and st["rows"] == N and st["bytes"] == N * dev.row_bytes // 2, st
    for ef in EFS:
        on, used_on = _search(dev, Q, K, ef, 1)
        geom = dev.launch_geometry()["kernel"]
        off, used_off = _search(dev, Q, K, ef, 0)
        assert (used_on, used_off) == (True, False), (dim, metric, ef)
        assert geom == dev.launch_geometry()["kernel"]
        _same(on, off, (dim, metric, ef, geom))
    dev.set_option("sorted_beam", 0)  # the two-heap kernel
    on, used_on = _search(dev, Q, K, 100, 1)
    off, used_off = _search(dev, Q, K, 100, 0)
    assert (used_on, used_off) == (True, False)
    _same(on, off, (dim, metric, "two heaps"))


def test_many_rounds_ties_and_hand_over_equal_the_oracle(flatnav, oracle_mod):
    rng = np.random.default_rng(11)
    dim = 128
    X = rng.integers(0, 4, (N, dim)).astype(np.float32)  # tie-dense
    Q = rng.integers(0, 4, (6000, dim)).astype(np.float32)  # more than one round of query slots
    ix, dev = _build(flatnav, "l2", X)
    o = oracle_mod.OracleIndex.from_blob("l2", "float32", dim, N, N, M, np.asarray(ix._raw_blob()))
    want = o.search(Q, K, 52, stats=True, threads=min(16, os.cpu_count() or 1))
    dev.set_option("sorted_beam", 1)
    for variant in (1, 3):  # the merged-beam kernel for every query; with 75 % of the last round straight to the exact search
        dev.set_option("sorted_variant", variant)
        on, used_on = _search(dev, Q, K, 52, 1)
        assert dev.launch_geometry()["kernel"].startswith("merged_beam")
        handed = dev.replayed_queries()["total"]
        off, used_off = _search(dev, Q, K, 52, 0)
        assert (used_on, used_off) == (True, False)
        assert handed > 0  # ties were met: queries went through the hand-over
        _same(on, off, ("variant", variant))
        _same(want, on, ("oracle, variant", variant))


def test_small_launch_and_filtered_search(flatnav):
    rng = np.random.default_rng(12)
    X = _lossless_rows(rng, N, 128)
    Q = rng.normal(size=(8, 128)).astype(np.float32)
    ix, dev = _build(flatnav, "l2", X)
    for ef in (16, 100):
        on, _ = _search(dev, Q, K, ef, 1)
        off, used = _search(dev, Q, K, ef, 0)
        assert not used
        _same(on, off, ("small launch", ef))
    allowed = rng.choice(N, N // 10, replace=False)
    dev.set_option("half_rows", 1)
    on = dev.search_filtered(Q, K, 64, allowed, stats=True)
    dev.set_option("half_rows", 0)
    _same(on, dev.search_filtered(Q, K, 64, allowed, stats=True), "filtered")


def test_a_value_that_is_not_lossless_drops_the_mirror(flatnav):
    rng = np.random.default_rng(13)
    X = _lossless_rows(rng, N, 128)
    X[1999, 77] = 1.0 / 3.0  # the last row of the second of three batches
    Q = rng.normal(size=(256, 128)).astype(np.float32)
    ix = flatnav.index.create("l2", 128, N, M)
    ix.set_num_threads(4)
    ix.add(X[:1000], EFC, labels=list(range(1000)), device=True)

    def handle(index):  # (asked for again after every add: the host index may replace its device handle)
        return hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)

    dev = handle(ix)

    def total_bytes(d):  # fnv_index_info's total device bytes: the index buffers, the mirror, the launch workspace
        info = (ctypes.c_uint64 * 8)()
        hip.check(hip.lib().fnv_index_info(d._h, info))
        return int(info[7])

    st = dev.half_rows()
    assert st["state"] == "live" and st["rows"] == 1000 and st["bytes"] == N * dev.row_bytes // 2, st
    assert total_bytes(dev) >= N * (dev.row_bytes + 4 * M + 4) + N * dev.row_bytes // 2
    ix.add(X[1000:2000], EFC, labels=list(range(1000, 2000)), device=True)
    dev = handle(ix)
    st = dev.half_rows()
    assert st["state"] == "dropped" and st["rows"] == 0 and st["bytes"] == 0, st
    ix.add(X[2000:], EFC, labels=list(range(2000, N)), device=True)
    dev = handle(ix)
    assert dev.half_rows()["state"] == "dropped" and dev.half_rows()["bytes"] == 0
    got, used = _search(dev, Q, K, 100, 1)
    assert not used
    # the same build with the mirror switched off when the index is made: same graph, same answers
    os.environ["FLATNAV_HALF_ROWS"] = "0"
    try:
        ix0 = flatnav.index.create("l2", 128, N, M)
        ix0.set_num_threads(4)
        for a, b in ((0, 1000), (1000, 2000), (2000, N)):
            ix0.add(X[a:b], EFC, labels=list(range(a, b)), device=True)
    finally:
        del os.environ["FLATNAV_HALF_ROWS"]
    dev0 = handle(ix0)
    assert dev0.half_rows()["state"] == "none" and dev0.half_rows()["bytes"] == 0
    assert np.array_equal(dev.read_links(0, N), dev0.read_links(0, N))
    want, used0 = _search(dev0, Q, K, 100, 1)
    assert not used0
    assert total_bytes(dev) == total_bytes(dev0)  # back to the float32-only figure (same launches: same workspace)
    _same(want, got, "dropped mirror vs never built")


def test_views_adopted_handles_raw_copies_and_replicas(flatnav):
    rng = np.random.default_rng(14)
    dim = 128
    X = _lossless_rows(rng, N, dim)
    Q = rng.normal(size=(256, dim)).astype(np.float32)
    ix, dev = _build(flatnav, "l2", X)
    want, used = _search(dev, Q, K, 100, 1)
    assert used
    # a view reads its source's mirror
    view = dev.view()
    got = view.search(Q, K, 100, stats=True)
    assert view.half_rows()["used_by_last_launch"] and view.half_rows()["state"] == "live"
    _same(want, got, "view")
    view.close()
    # an adopted handle: nothing until it is asked to build one
    adopted = hip.DeviceIndex.adopt(dev.device_buffers(), M, N, "float32", "l2", dim, keep_alive=dev)
    got = adopted.search(Q, K, 100, stats=True)
    assert adopted.half_rows()["state"] == "none" and not adopted.half_rows()["used_by_last_launch"]
    _same(want, got, "adopted, no mirror")
    assert adopted.build_half_rows()
    got = adopted.search(Q, K, 100, stats=True)
    assert adopted.half_rows()["state"] == "live" and adopted.half_rows()["used_by_last_launch"]
    _same(want, got, "adopted, mirror built")
    adopted.close()
    # a copy filled through raw pointers
    import torch

    from flatnav_amd.multigpu import _DevView

    copy = hip.DeviceIndex.alloc(M, N, "float32", "l2", dim)
    for (src, nbytes), (dst, _) in zip(dev.device_buffers(), copy.device_buffers()):
        torch.as_tensor(_DevView(dst, nbytes), device="cuda:0").copy_(torch.as_tensor(_DevView(src, nbytes), device="cuda:0"))
    torch.cuda.synchronize()
    got = copy.search(Q, K, 100, stats=True)
    assert copy.half_rows()["state"] == "none" and not copy.half_rows()["used_by_last_launch"]
    _same(want, got, "raw copy, no mirror")
    assert copy.build_half_rows()
    got = copy.search(Q, K, 100, stats=True)
    assert copy.half_rows()["used_by_last_launch"]
    _same(want, got, "raw copy, mirror built")
    copy.close()
    # a replica gets its own
    (replica,) = dev.replicate([0])
    got = replica.search(Q, K, 100, stats=True)
    assert replica.half_rows()["state"] == "live" and replica.half_rows()["used_by_last_launch"]
    _same(want, got, "replica")
    replica.close()
