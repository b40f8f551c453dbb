"""float16 indexes on the GPU.  Every check searches one graph twice: the oracle on the float32 data the float16 values widen to,
and the device on the float16 blob of the same graph (same links, data section narrowed).  On integer-valued data every
distance is exact, so ids, distances, n_dist and n_hops must be bit-identical; on float data the DESIGN §8 bar holds."""
import os
import subprocess

import numpy as np
import pytest

from flatnav_amd import datasets as ds
from flatnav_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def flatnav():
    import flatnav_amd

    return flatnav_amd


def _f16_blob(o, n, dim):
    """The oracle's float32 node store with its data section narrowed to float16 (exact: the rows are widened float16
    values): same links, same labels.  (A multi-threaded build does not put row i into node i: take each node's own row.)"""
    nodes = np.asarray(o.blob())[: n * o.node_size].reshape(n, o.node_size)
    out = np.empty((n, 2 * dim + o.node_size - o.data_size), np.uint8)
    out[:, : 2 * dim] = nodes[:, : 4 * dim].copy().view(np.float32).astype(np.float16).view(np.uint8)
    out[:, 2 * dim:] = nodes[:, o.data_size:]
    return out.reshape(-1)


def _pair(oracle_mod, metric, X16, M, efc):
    """(oracle on the widened data, device index on the float16 blob of the oracle's graph)."""
    n, dim = X16.shape
    o = oracle_mod.OracleIndex.create(metric, dim, n, M, "float32")
    o.add(X16.astype(np.float32), efc, threads=min(8, os.cpu_count() or 1))
    dev = hip.DeviceIndex.upload(_f16_blob(o, n, dim), 2 * dim + 4 * M + 4, 2 * dim, M, n, "float16", metric, dim)
    return o, dev


def _exact(want, got, what):
    (od, ol, ost), (gd, gl, gst) = want, got
    assert np.array_equal(gl, ol), what
    assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), what
    assert np.array_equal(gst["n_dist"], ost["n_dist"]) and np.array_equal(gst["n_hops"], ost["n_hops"]), what


def _int16(rng, shape, metric):
    lo, hi = (-6, 7) if metric == "ip" else (0, 40)  # sums stay far below 2^24 up to d = 2100
    return rng.integers(lo, hi, shape).astype(np.float16)


# every row configuration: (8,1) (8,2) (8,4) (16,4) (32,4) (64,4) + multi-span rows; 200 / 208 = split rows (3 lines + 16 / 32 B)
DIMS = [8, 40, 64, 128, 200, 208, 256, 512, 768, 1000, 2100]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", DIMS)
def test_integer_data_bit_exact_every_kernel(oracle_mod, metric, dim):
    rng = np.random.default_rng(dim * 3 + (metric == "ip"))
    N, M = 1500 if dim <= 512 else 800, 16
    X, Q = _int16(rng, (N, dim), metric), _int16(rng, (200, dim), metric)
    o, dev = _pair(oracle_mod, metric, X, M, 40)
    if dim in (200, 208):
        assert (dev.row_bytes, dev.tail_bytes) == (384, 2 * dim - 384)
    for K, ef in ((10, 64), (1, 8), (20, 300)):
        want = o.search(Q, K, ef, stats=True, threads=8)
        _exact(want, dev.search(Q, K, ef, stats=True), "default K=%d ef=%d" % (K, ef))
    want = o.search(Q, 10, 64, stats=True, threads=8)
    dev.set_option("sorted_beam", 0)  # K1, the two-heap kernel
    _exact(want, dev.search(Q, 10, 64, stats=True), "sorted_beam=0")
    dev.set_option("sorted_beam", 1)
    for v in range(7):
        dev.set_option("sorted_variant", v)
        _exact(want, dev.search(Q, 10, 64, stats=True), "sorted_variant=%d" % v)
    dev.set_option("sorted_variant", -1)
    dev.set_option("sorted_beam", 2)
    dev.set_option("entry_kernel", 1)  # K0: the entry scan as a batch kernel
    _exact(want, dev.search(Q, 10, 64, stats=True), "entry_kernel=1")
    dev.set_option("entry_kernel", 0)
    for vd in (0, 1):
        dev.set_option("visited_direct", vd)
        _exact(want, dev.search(Q, 10, 64, stats=True), "visited_direct=%d" % vd)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_large_magnitudes_and_tie_dense_data(oracle_mod, metric):
    rng = np.random.default_rng(17)
    # magnitudes up to 2^9 / 2^10 (sums < 2^24 at d = 8) and tie-dense values 0..3: bit-exact, ties included
    big = rng.integers(-512, 513, (2000, 8)).astype(np.float16) if metric == "l2" else \
        rng.integers(-1024, 1025, (2000, 8)).astype(np.float16)
    ties = rng.integers(0, 4, (3000, 64)).astype(np.float16)
    for X in (big, ties):
        Q = X[rng.integers(0, len(X), 300)] + np.float16(1) * (rng.random((300, X.shape[1])) < 0.1)
        o, dev = _pair(oracle_mod, metric, X, 16, 48)
        for K, ef in ((10, 52), (5, 200)):
            _exact(o.search(Q, K, ef, stats=True, threads=8), dev.search(Q, K, ef, stats=True), (X.shape, K, ef))


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", [128, 768])
def test_float_data_within_tolerance(oracle_mod, metric, dim):
    X, Q = ds.randn(12000, 1000, dim, seed=5, normalize=(metric == "ip"))
    X16, Q16 = X.astype(np.float16), Q.astype(np.float16)
    o, dev = _pair(oracle_mod, metric, X16, 32, 64)
    od, ol = o.search(Q16, 10, 100, threads=8)
    gd, gl = dev.search(Q16, 10, 100)
    same = (ol == gl).all(axis=1)
    assert same.mean() >= 0.999, same.mean()
    assert np.allclose(od[same], gd[same], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("wiring", [True, False], ids=["device_wiring", "host_wiring"])
@pytest.mark.parametrize("metric", ["l2", "angular"])
@pytest.mark.parametrize("dim", [40, 200])
def test_sequential_device_build_equals_oracle_graph(flatnav, oracle_mod, metric, dim, wiring):
    rng = np.random.default_rng(dim + 1)
    N, M, efc = 1200, 8, 40
    X = _int16(rng, (N, dim), "ip" if metric == "angular" else "l2")
    o = oracle_mod.OracleIndex.create(metric, dim, N, M, "float32")
    o.add(X.astype(np.float32), efc)
    ix = flatnav.index.create(metric, dim, N, M, flatnav.data_type.DataType.float16)
    ix.add(X, efc, device=True, device_max_batch=1, device_bootstrap=40, device_wiring=wiring)
    want = np.asarray(o.blob())[: N * o.node_size].reshape(N, o.node_size)[:, o.data_size:]
    got = np.asarray(ix._raw_blob()).reshape(N, -1)[:, 2 * dim:]
    bad = np.flatnonzero((want != got).any(axis=1))
    assert bad.size == 0, "first differing node %d of %d differing" % (bad[0], bad.size)


def test_python_end_to_end(flatnav, oracle_mod, tmp_path):
    import torch

    rng = np.random.default_rng(2)
    N, dim, M, K = 8000, 96, 24, 10
    X = rng.integers(0, 30, (N, dim)).astype(np.float32)
    Q = rng.integers(0, 30, (700, dim)).astype(np.float32)
    ix = flatnav.index.create("l2", dim, N, M, flatnav.data_type.DataType.float16)
    ix.set_num_threads(4)
    ix.add(X, 64, device=True)
    d16, l16 = ix.search(Q.astype(np.float16), K, 80)
    d32, l32 = ix.search(Q, K, 80)  # float32 queries are narrowed first: integer values, the same rows
    d64, l64 = ix.search(Q.astype(np.float64), K, 80)
    assert np.array_equal(l16, l32) and np.array_equal(l16, l64) and np.array_equal(d16, d32) and np.array_equal(d16, d64)
    o = oracle_mod.OracleIndex.from_blob("l2", "float32", dim, N, N, M, _widened_blob(ix, N, dim, M))
    od, ol = o.search(Q, K, 80, threads=8)
    assert np.array_equal(l16, ol) and np.array_equal(d16.view(np.uint32), od.view(np.uint32))
    for i in (0, 5, 699):
        sd, sl = ix.search_single(Q[i].astype(np.float16), K, 80)
        assert np.array_equal(sl, ol[i]) and np.array_equal(sd, od[i])
        sd, sl = ix.search_single(Q[i], K, 80)
        assert np.array_equal(sl, ol[i])
    p = str(tmp_path / "f16.bin")
    ix.save(p)
    loaded = flatnav.index.IndexL2Float16.load_index(p)
    ld, ll = loaded.search(Q, K, 80)
    assert np.array_equal(ll, ol) and np.array_equal(ld.view(np.uint32), od.view(np.uint32))
    # the ctypes handle on the same buffers: small zero-copy calls, pinned callers, two replicas on one device
    dev = hip.DeviceIndex.upload(np.asarray(ix._raw_blob()), ix._node_size_bytes, 2 * dim, M, N, "float16", "l2", dim)
    assert dev.dtype == "float16"
    Q16 = Q.astype(np.float16)
    for zc in (1 << 20, 0):
        dev.set_option("host_zero_copy", zc)
        for nq in (1, 3, 64):
            gd, gl = dev.search(Q16[:nq], K, 80)
            assert np.array_equal(gl, ol[:nq]) and np.array_equal(gd.view(np.uint32), od[:nq].view(np.uint32)), (zc, nq)
    dev.set_option("host_zero_copy", 1 << 20)
    qpin = torch.from_numpy(Q16).pin_memory()
    dpin = torch.empty((len(Q), K), dtype=torch.float32).pin_memory()
    lpin = torch.empty((len(Q), K), dtype=torch.int32).pin_memory()
    dev.search_into(qpin.numpy(), K, 80, dpin.numpy(), lpin.numpy())
    assert np.array_equal(lpin.numpy(), ol) and np.array_equal(dpin.numpy().view(np.uint32), od.view(np.uint32))
    reps = dev.replicate([0, 0])
    md, ml = hip.search_multi([dev] + reps, Q16, K, 80)
    assert np.array_equal(ml, ol) and np.array_equal(md.view(np.uint32), od.view(np.uint32))


def _widened_blob(ix, N, dim, M):
    nodes = np.asarray(ix._raw_blob())[: N * ix._node_size_bytes].reshape(N, ix._node_size_bytes)
    out = np.empty((N, 4 * dim + 4 * M + 4), np.uint8)
    out[:, : 4 * dim] = nodes[:, : 2 * dim].copy().view(np.float16).astype(np.float32).view(np.uint8)
    out[:, 4 * dim:] = nodes[:, 2 * dim:]
    return out.reshape(-1)


def test_cli_pair_on_float16_npy(tmp_path):
    from flatnav_amd import build_host

    tools = build_host.build_tools()
    rng = np.random.default_rng(4)
    X = rng.standard_normal((3000, 48)).astype(np.float16)
    Q = rng.standard_normal((200, 48)).astype(np.float16)
    gt = ds.exact_topk_l2(X.astype(np.float32), Q.astype(np.float32), 10).astype(np.int32)
    for name, a in (("x", X), ("q", Q), ("gt", gt)):
        np.save(tmp_path / (name + ".npy"), a)
    idx = str(tmp_path / "f16.bin")
    r = subprocess.run([tools["flatnav_construct"], "0", "0", str(tmp_path / "x.npy"), "16", "64", "4", idx],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert np.frombuffer(open(idx, "rb").read(4), np.int32)[0] == 8
    r = subprocess.run([tools["flatnav_query"], "0", idx, str(tmp_path / "q.npy"), str(tmp_path / "gt.npy"), "64,200", "10", "0",
                        "0", "--dtype", "f16"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    recalls = [float(l.split("Mean Recall: ")[1].split(",")[0]) for l in r.stdout.splitlines() if "Mean Recall" in l]
    assert len(recalls) == 2 and recalls[1] >= 0.95, r.stdout
