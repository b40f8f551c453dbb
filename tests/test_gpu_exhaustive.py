"""Exhaustive search on the GPU (fnv_search_batch_exhaustive[_device], DeviceIndex.search_exhaustive, _core search_exhaustive).

The reference is plain numpy in this file: distances of the candidate rows, then the contract's order -- (distance, node id)
ascending, NaN last.  On integer-valued data every distance is an exact integer in any summation order, so labels, distance
bits, count and n_dist must match exactly; such data ties often, which is what exercises the id tie-break.  Float data is held
to DESIGN section 8's float bar against float64, and to the graph search's own distance bits."""
import ctypes
import threading

import numpy as np
import pytest

from flatnav_amd import datasets as ds
from flatnav_amd import hip
from test_gpu_filtered import _int_data, _pair

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6  # the float bar


@pytest.fixture(scope="module")
def flatnav():
    import flatnav_amd

    return flatnav_amd


def _build(oracle_mod, metric, dtype, X, labels=None, **kw):
    """_pair's index, and what the scan sees: (rows in NODE order, the nodes' labels, device index).  _pair builds with several
    threads, which hand out node ids in arrival order -- and the contract breaks distance ties by node id, not by row number."""
    n = len(X)
    labels = np.arange(n, dtype=np.int32) if labels is None else labels
    o, dev = _pair(oracle_mod, metric, dtype, X, labels=labels, **kw)
    node_labels = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)[:, o.node_size - 4:].copy().view(np.int32).ravel()
    row_of_label = np.empty(int(labels.max()) + 1, np.int64)
    row_of_label[labels] = np.arange(n)
    return X[row_of_label[node_labels]], node_labels, dev


def _dist64(X, Q, metric):
    """[nq][n] float64 distances (exact on the integer data: every sum is an integer below 2^24)."""
    X, Q = X.astype(np.float64), Q.astype(np.float64)
    if metric == "l2":
        return (Q * Q).sum(1)[:, None] - 2.0 * (Q @ X.T) + (X * X).sum(1)[None, :]
    return 1.0 - Q @ X.T


def _topk(D, nodes, labels, K):
    """The contract on a distance matrix D[:, nodes] already restricted to the ascending candidate ids `nodes`:
    (dist float32 [nq, K], labels int32 [nq, K], count, n_dist).  Stable argsort of ascending ids = lexsort((id, dist))."""
    nq, m = D.shape[0], len(nodes)
    d = np.full((nq, K), np.inf, np.float32)
    l = np.full((nq, K), -1, np.int32)
    k = min(K, m)
    if k:
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        d[:, :k] = np.take_along_axis(D, order, 1).astype(np.float32)
        l[:, :k] = labels[nodes[order]]
    return d, l, np.full(nq, k, np.int32), np.full(nq, m, np.uint64)


def _reference(X, Q, metric, labels, K, allowed=None, n_live=None):
    n = len(X) if n_live is None else n_live
    nodes = np.arange(n)
    if allowed is not None:
        ok = np.zeros(int(max(labels.max(), np.max(allowed, initial=0))) + 1, bool)
        ok[np.asarray(allowed, np.int64)] = True
        nodes = nodes[ok[labels[:n]]]
    return _topk(_dist64(X[nodes], Q, metric), nodes, labels, K)


def _equal(got, want, what):
    gd, gl, gst = got
    wd, wl, wc, wn = want
    assert np.array_equal(gl, wl), what
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what
    assert np.array_equal(gst["count"], wc), what
    assert np.array_equal(gst["n_dist"].astype(np.uint64), wn), what


def _same_results(a, b, what):
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), what
    for key in ("count", "n_dist"):
        assert np.array_equal(a[2][key], b[2][key]), (what, key)


# ---- 1. every kernel shape, exact -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["float32", "float16", "uint8", "int8"])
@pytest.mark.parametrize("dim", [7, 100, 128, 200, 768])
def test_every_kernel_shape_exact(oracle_mod, dtype, metric, dim):
    rng = np.random.default_rng(dim * 11 + len(dtype) + len(metric))
    n = 1500 if dim >= 200 else 2500
    X, Q = _int_data(rng, n, 48, dim, dtype, metric)
    labels = (rng.permutation(n) + 3).astype(np.int32)  # labels are not node ids
    X, labels, dev = _build(oracle_mod, metric, dtype, X, labels, efc=32)
    allowed = rng.choice(n, n // 10, replace=False) + 3
    D = _dist64(X, Q, metric)  # once; the filtered reference takes its columns
    ok = np.zeros(n + 3, bool)
    ok[allowed] = True
    nodes_f = np.flatnonzero(ok[labels])
    for K in (1, 10, 100):
        want_all = _topk(D, np.arange(n), labels, K)
        want_f = _topk(D[:, nodes_f], nodes_f, labels, K)
        results = []
        for seg in (0, 256):  # automatic, and many segments with a real merge
            dev.set_option("scan_segment_rows", seg)
            got_all = dev.search_exhaustive(Q, K, stats=True)
            got_f = dev.search_exhaustive(Q, K, allowed=allowed, stats=True)
            _equal(got_all, want_all, (dtype, metric, dim, K, seg, "all"))
            _equal(got_f, want_f, (dtype, metric, dim, K, seg, "10 %"))
            results.append((got_all, got_f))
        _same_results(results[0][0], results[1][0], (dtype, metric, dim, K, "segments"))
        _same_results(results[0][1], results[1][1], (dtype, metric, dim, K, "segments, filtered"))


# ---- 2. edges of tiles and of K ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_edges_of_tiles_and_of_k(oracle_mod, n):
    rng = np.random.default_rng(100 + n)
    dim = 32
    X, Qall = _int_data(rng, n, 257, dim, "float32", "l2")
    labels = (rng.permutation(n) + 3).astype(np.int32)
    X, labels, dev = _build(oracle_mod, "l2", "float32", X, labels, M=8, efc=16)
    for nq in (1, 3, 257):
        Q = Qall[:nq]
        D = _dist64(X, Q, "l2")
        for K in sorted({1, n, n + 5, 1024}):
            if K > 1024:
                continue
            want = _topk(D, np.arange(n), labels, K)
            got = dev.search_exhaustive(Q, K, stats=True)
            _equal(got, want, (n, nq, K))
            assert (got[2]["count"] == min(K, n)).all()
            if K > n:  # padding
                assert np.isposinf(got[0][:, n:]).all() and (got[1][:, n:] == -1).all()
    Q = Qall[:3]
    # the empty filter
    d, l, st = dev.search_exhaustive(Q, 5, allowed=np.zeros(0, np.int64), stats=True)
    assert (st["count"] == 0).all() and (st["n_dist"] == 0).all() and np.isposinf(d).all() and (l == -1).all()
    # one allowed label
    one = int(labels[n // 2])
    got = dev.search_exhaustive(Q, 5, allowed=np.array([one]), stats=True)
    _equal(got, _reference(X, Q, "l2", labels, 5, allowed=[one]), (n, "one label"))
    assert (got[2]["count"] == 1).all() and (got[1][:, 0] == one).all()
    # allowed labels beyond the index's labels are ignored
    beyond = np.concatenate([labels[: max(1, n // 3)], np.arange(n + 3, n + 60)])
    got = dev.search_exhaustive(Q, 5, allowed=beyond, stats=True)
    _equal(got, _reference(X, Q, "l2", labels, 5, allowed=labels[: max(1, n // 3)]), (n, "beyond"))
    # K outside [1, 1024]
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            dev.search_exhaustive(Q, bad)
        out_d, out_l = np.empty((3, max(bad, 1)), np.float32), np.empty((3, max(bad, 1)), np.int32)
        rc = hip.lib().fnv_search_batch_exhaustive(dev._h, Q.ctypes.data, 3, bad, 0, None, 0, out_d.ctypes.data, out_l.ctypes.data,
                                                   None, None)
        assert rc == hip.FNV_ERR_INVALID and b"1024" in hip.lib().fnv_last_error()


# ---- 3. same distance bits as the graph search, float data -----------------------------------------------------------------
def _float_pair(oracle_mod, dtype, metric, dim, n, nq):
    X, Q = ds.randn(n, nq, dim, seed=dim, normalize=metric == "ip")
    if dtype == "float16":  # the rows and queries the float16 index really holds
        X, Q = X.astype(np.float16), Q.astype(np.float16)
    _, _, dev = _build(oracle_mod, metric, dtype, X)  # labels = row numbers
    return X, Q, dev


def _sorted_by_key(d, l):
    """Every row ascending by (distance, node id), NaN last; `l` holds node ids."""
    for row_d, row_l in zip(d, l):
        if not np.array_equal(np.lexsort((row_l, row_d)), np.arange(len(row_d))):
            return False
    return True


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("dim", [64, 100, 768])
def test_same_distance_bits_as_the_graph_search(oracle_mod, dtype, metric, dim):
    X, Q, dev = _float_pair(oracle_mod, dtype, metric, dim, 1000, 64)
    gd, gl, gst = dev.search(Q, 1000, 1000, stats=True)
    ed, el = dev.search_exhaustive(Q, 1000)
    dev.set_option("output_node_ids", 1)
    nd, nl = dev.search_exhaustive(Q, 1000)
    assert np.array_equal(nd.view(np.uint32), ed.view(np.uint32)) and (nl >= 0).all() and _sorted_by_key(nd, nl)
    assert (gst["count"] > 900).all()  # the graph search reaches (nearly) every node: the comparison is not vacuous
    by_label = np.empty((len(Q), 1000), np.uint32)
    np.put_along_axis(by_label, el.astype(np.int64), ed.view(np.uint32), 1)
    for q in range(len(Q)):
        c = int(gst["count"][q])
        assert np.array_equal(by_label[q, gl[q, :c]], gd[q, :c].view(np.uint32)), (dtype, metric, dim, q)


# ---- 4. the float bar with nothing left out -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", [64, 100, 768])
def test_float_bar_with_nothing_left_out(oracle_mod, metric, dim):
    """Every reported distance within rtol 1e-5 / atol 1e-6 of the float64 distance of its own label; the list within the same
    tolerance of the true sorted top-K distances; every returned row truly among the K nearest up to that tolerance.  (A float32
    scan in another summation order stays >= 14 x inside the bar on these inputs on the CPU: worst 0.07 of it, 768-d l2.)"""
    n, nq, K = 3000, 64, 10
    X, Q, dev = _float_pair(oracle_mod, "float32", metric, dim, n, nq)
    D = _dist64(X, Q, metric)  # (float64: its own rounding is nine orders of magnitude below the bar)
    rng = np.random.default_rng(dim)
    one_pct = np.sort(rng.choice(n, n // 100, replace=False))
    for allowed in (None, one_pct):
        nodes = np.arange(n) if allowed is None else allowed
        d, l, st = dev.search_exhaustive(Q, K, allowed=allowed, stats=True)
        assert (st["count"] == K).all() and (st["n_dist"] == len(nodes)).all()
        assert np.isin(l, nodes).all() and all(len(set(row)) == K for row in l)
        own = np.take_along_axis(D, l.astype(np.int64), 1)
        tol = ATOL + RTOL * np.abs(own)
        err = np.abs(d.astype(np.float64) - own)
        print("exhaustive float bar: dim %d %s %s: worst |error| / tolerance = %.4f" %
              (dim, metric, "all" if allowed is None else "1 %", float((err / tol).max())))
        assert (err <= tol).all()
        true_sorted = np.sort(D[:, nodes], axis=1)[:, :K]
        assert (np.abs(d.astype(np.float64) - true_sorted) <= ATOL + RTOL * np.abs(true_sorted)).all()
        kth = true_sorted[:, K - 1:K]
        assert (own <= kth + ATOL + RTOL * np.abs(kth)).all()


# ---- 5. NaN and inf -----------------------------------------------------------------------------------------------------------
def test_nan_and_inf_rank_last(oracle_mod):
    rng = np.random.default_rng(5)
    n, dim = 200, 16
    X, Q = _int_data(rng, n, 8, dim, "float32", "l2")
    X2 = X.copy()  # (the graph is built on finite rows; the two rows are rewritten in the node store before the upload)
    X2[17, 3] = np.nan
    X2[90, 5] = 3e38  # (3e38 - q)^2 overflows float32: +inf
    o2 = oracle_mod.OracleIndex.create("l2", dim, n, 8, "float32")
    o2.add(X, 16)
    blob = np.asarray(o2.blob()).copy()[: n * o2.node_size].reshape(n, o2.node_size)
    blob[:, : 4 * dim] = X2.view(np.uint8).reshape(n, 4 * dim)
    dev = hip.DeviceIndex.upload(blob.reshape(-1), o2.node_size, o2.data_size, o2.M, n, "float32", "l2", dim)
    d, l, st = dev.search_exhaustive(Q, n, stats=True)
    assert (st["count"] == n).all() and (st["n_dist"] == n).all()
    assert (l[:, -1] == 17).all() and np.isnan(d[:, -1]).all()
    assert (l[:, -2] == 90).all() and np.isposinf(d[:, -2]).all()
    assert np.isfinite(d[:, :-2]).all()
    finite = np.delete(np.arange(n), [17, 90])
    want = _topk(_dist64(X[finite], Q, "l2"), finite, np.arange(n, dtype=np.int32), n - 2)
    assert np.array_equal(l[:, :-2], want[1]) and np.array_equal(d[:, :-2].view(np.uint32), want[0].view(np.uint32))


# ---- 6. state the scan must respect -------------------------------------------------------------------------------------------
def test_live_nodes_views_and_node_ids(oracle_mod):
    rng = np.random.default_rng(6)
    n = 2000
    X, Q = _int_data(rng, n, 40, 48, "float32", "l2")
    labels = (rng.permutation(n) + 3).astype(np.int32)
    X, labels, dev = _build(oracle_mod, "l2", "float32", X, labels, efc=32)
    allowed = rng.choice(n, n // 5, replace=False) + 3
    dev.set_live_nodes(n // 2)
    view = dev.view()
    for handle in (dev, view):
        _equal(handle.search_exhaustive(Q, 10, stats=True), _reference(X, Q, "l2", labels, 10, n_live=n // 2), "live half")
        _equal(handle.search_exhaustive(Q, 10, allowed=allowed, stats=True),
               _reference(X, Q, "l2", labels, 10, allowed=allowed, n_live=n // 2), "live half, filtered")
    view.close()
    dev.set_live_nodes(n)
    dev.set_option("output_node_ids", 1)
    nodes = np.flatnonzero(np.isin(labels, allowed))
    _equal(dev.search_exhaustive(Q, 10, allowed=allowed, stats=True),
           _topk(_dist64(X[nodes], Q, "l2"), nodes, np.arange(n, dtype=np.int32), 10), "node ids")


def test_device_built_index(flatnav):
    rng = np.random.default_rng(66)
    n, dim = 4000, 64
    X, Q = _int_data(rng, n, 40, dim, "float32", "l2")
    index = flatnav.index.create("l2", dim, n, 16)
    index.add(X, 64, device=True)
    # node order is the builder's business: compare by label (label i = row i of X) on distances that do not tie at the cut
    D = _dist64(X, Q, "l2")
    d, l = index.search_exhaustive(Q, 10)
    own = np.take_along_axis(D, l.astype(np.int64), 1).astype(np.float32)
    assert np.array_equal(own.view(np.uint32), d.view(np.uint32))
    assert np.array_equal(d, np.sort(D, axis=1)[:, :10].astype(np.float32))
    assert all(len(set(row)) == 10 for row in l)
    allowed = rng.choice(n, n // 10, replace=False)
    d, l = index.search_exhaustive(Q, 10, allowed=allowed)
    assert np.isin(l, allowed).all()
    assert np.array_equal(d, np.sort(D[:, np.sort(allowed)], axis=1)[:, :10].astype(np.float32))


# ---- 7. the entry points agree --------------------------------------------------------------------------------------------------
def test_device_entry_point_on_a_side_stream(oracle_mod):
    import torch

    rng = np.random.default_rng(7)
    n, K = 3000, 10
    X, Q = _int_data(rng, n, 100, 64, "float32", "l2")
    _, dev = _pair(oracle_mod, "l2", "float32", X, efc=32)
    allowed = rng.choice(n, n // 10, replace=False)
    bits, n_bits = hip.pack_allowed(allowed)
    cuda = torch.device("cuda", dev.device)
    tq = torch.from_numpy(Q).to(cuda)
    tb = torch.from_numpy(bits).to(cuda)
    stream = torch.cuda.Stream(cuda)
    for use_filter in (False, True):
        want = dev.search_exhaustive(Q, K, allowed=allowed if use_filter else None, stats=True)
        td = torch.empty((len(Q), K), dtype=torch.float32, device=cuda)
        tl = torch.empty((len(Q), K), dtype=torch.int32, device=cuda)
        tc = torch.empty(len(Q), dtype=torch.int32, device=cuda)
        tnd = torch.empty(len(Q), dtype=torch.int64, device=cuda)
        torch.cuda.synchronize(cuda)
        with torch.cuda.stream(stream):
            dev.search_device_exhaustive(tq.data_ptr(), len(Q), K, td.data_ptr(), tl.data_ptr(), tc.data_ptr(), tnd.data_ptr(),
                                         bits_ptr=tb.data_ptr(), n_bits=n_bits, use_filter=use_filter, stream=stream.cuda_stream)
        stream.synchronize()
        dev.status()
        got = (td.cpu().numpy(), tl.cpu().numpy(), {"count": tc.cpu().numpy(), "n_dist": tnd.cpu().numpy().astype(np.uint64)})
        _same_results(got, want, ("device entry point", use_filter))


def test_core_module_entry_point(flatnav):
    rng = np.random.default_rng(77)
    n, dim = 2000, 32
    X, Q = _int_data(rng, n, 30, dim, "float32", "l2")
    index = flatnav.index.create("l2", dim, n, 16)
    index.set_num_threads(1)  # node i = row i = label i
    index.add(X, 32)
    allowed = rng.choice(n, n // 4, replace=False)
    d, l = index.search_exhaustive(Q, 10)
    df, lf = index.search_exhaustive(Q, 10, allowed=allowed)
    D = _dist64(X, Q, "l2")
    want = _topk(D, np.arange(n), np.arange(n, dtype=np.int32), 10)  # host builds keep node i = label i
    assert np.array_equal(l, want[1]) and np.array_equal(d.view(np.uint32), want[0].view(np.uint32))
    nodes = np.sort(allowed)
    want = _topk(D[:, nodes], nodes, np.arange(n, dtype=np.int32), 10)
    assert np.array_equal(lf, want[1]) and np.array_equal(df.view(np.uint32), want[0].view(np.uint32))
    dev = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)  # the same device index through the C ABI
    sd, sl = dev.search_exhaustive(Q, 10, allowed=allowed)
    assert np.array_equal(sl, lf) and np.array_equal(sd.view(np.uint32), df.view(np.uint32))
    short = index.search_exhaustive(Q, 10, allowed=allowed[:4])
    assert np.isposinf(short[0][:, 4:]).all() and (short[1][:, 4:] == -1).all()
    for bad_k in (0, 1025):
        with pytest.raises(ValueError):
            index.search_exhaustive(Q, bad_k)
    with pytest.raises(ValueError):
        index.search_exhaustive(Q[:, :5], 10)
    with pytest.raises(ValueError):
        index.search_exhaustive(Q, 10, allowed=np.array([1, -2]))


def test_concurrent_callers_on_one_handle(oracle_mod):
    rng = np.random.default_rng(8)
    n = 4000
    X, Q = _int_data(rng, n, 256, 32, "float32", "l2")
    _, dev = _pair(oracle_mod, "l2", "float32", X, efc=32)
    filters = [np.arange(0, n, 2), np.arange(1, n, 2), rng.choice(n, n // 20, replace=False), None]
    want = [dev.search_exhaustive(Q, 10, allowed=f, stats=True) for f in filters]
    errors = []

    def worker(i):
        try:
            for _ in range(8):
                got = dev.search_exhaustive(Q, 10, allowed=filters[i], stats=True)
                _same_results(got, want[i], i)
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(filters))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []


# ---- 8. it really is the selective-filter answer -----------------------------------------------------------------------------
def test_equals_the_filtered_graph_search_at_one_percent(oracle_mod):
    rng = np.random.default_rng(9)
    n, K = 5000, 10
    X, Q = _int_data(rng, n, 40, 64, "float32", "l2")
    labels = (rng.permutation(n) + 3).astype(np.int32)
    _, dev = _pair(oracle_mod, "l2", "float32", X, labels=labels)
    allowed = rng.choice(n, n // 100, replace=False) + 3
    view = dev.view()
    view.set_option("spill_entries", 1 << 18)
    fd, fl, fst = view.search_filtered(Q, K, 5000, allowed, stats=True)
    ed, el, est = dev.search_exhaustive(Q, K + 1, allowed=allowed, stats=True)
    assert (fst["count"] == K).all() and (est["count"] == K + 1).all()
    assert np.array_equal(fd.view(np.uint32), ed[:, :K].view(np.uint32))
    clear = ed[:, K - 1] != ed[:, K]  # the K-th and (K+1)-th distances differ: the set of the K nearest is unique
    assert clear.any()
    for q in np.flatnonzero(clear):
        assert set(fl[q]) == set(el[q, :K]), q
    view.close()
