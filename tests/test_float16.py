"""float16 indexes without a GPU: the Python surface, the vector-table layout of 2-byte rows, the host builder (its graph
equals the float32 graph of the widened data), the float -> float16 input conversion and the file format."""
import struct

import numpy as np
import pytest


@pytest.fixture(scope="module")
def flatnav():
    from flatnav_amd import build_host

    build_host.build()
    import flatnav_amd

    return flatnav_amd


def _links(blob, node_size, data_size, n):
    """[n][M links + label] bytes of an AoS node store: everything but the vectors."""
    return np.asarray(blob)[: n * node_size].reshape(n, node_size)[:, data_size:]


def _vectors(blob, node_size, data_size, n):
    return np.asarray(blob)[: n * node_size].reshape(n, node_size)[:, :data_size]


def _int_data(n, dim, seed, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi, (n, dim)).astype(np.float16)


def test_surface(flatnav):
    from flatnav_amd import hip

    DT = flatnav.data_type.DataType
    assert int(DT.float16) == 8 and DT.float16.name == "float16"
    assert {"IndexL2Float16", "IndexIPFloat16"} <= set(dir(flatnav.index))
    for metric, cls in (("l2", "IndexL2Float16"), ("angular", "IndexIPFloat16")):
        ix = flatnav.index.create(distance_type=metric, index_data_type=DT.float16, dim=16, dataset_size=10,
                                  max_edges_per_node=8)
        assert type(ix).__name__ == cls
        assert ix._data_size_bytes == 32 and ix._node_size_bytes == 32 + 4 * 8 + 4
    assert hip.DTYPE_ORD["float16"] == 8 and hip.ORD_DTYPE[8] == "float16"
    assert hip._np_dtype("float16") is np.float16


LAYOUT = {7: (16, 0), 64: (128, 0), 100: (256, 0), 128: (256, 0), 192: (384, 0), 200: (384, 16), 208: (384, 32),
          209: (512, 0), 768: (1536, 0)}


@pytest.mark.parametrize("d", sorted(LAYOUT))
def test_row_layout(d, monkeypatch):
    # 2-byte rows follow the byte rule of csrc/launch_plan.hpp row_layout: 193 ... 208-d float16 = three lines + <= 32 bytes is
    # split; a float16 row of d elements is laid out exactly like a float32 row of d / 2
    from flatnav_amd import build, hip

    build.build()
    for k in ("FLATNAV_ROW_PAD_PCT", "FLATNAV_SPLIT_ROWS", "FLATNAV_SPLIT_TAIL_MAX_MB"):
        monkeypatch.delenv(k, raising=False)
    cap = 100_000
    assert hip.row_layout(d, "float16", cap) == LAYOUT[d]
    if d % 2 == 0:
        assert hip.row_layout(d, "float16", cap) == hip.row_layout(d // 2, "float32", cap)


@pytest.mark.parametrize("metric", ["l2", "angular"])
def test_host_build_on_integer_data_equals_oracle_graph(flatnav, oracle_mod, tmp_path, metric):
    # integer-valued float16 data: every distance is exact, so the graph is the oracle's graph of the widened float32 data
    N, dim, M = 1200, 40, 16
    X = _int_data(N, dim, 11, -8 if metric == "angular" else -200, 8 if metric == "angular" else 200)
    ix = flatnav.index.create(distance_type=metric, index_data_type=flatnav.data_type.DataType.float16, dim=dim,
                              dataset_size=N, max_edges_per_node=M)
    ix.add(data=X, ef_construction=64)
    o = oracle_mod.OracleIndex.create(metric, dim, N, M, "float32")
    o.add(X.astype(np.float32), 64)
    blob = np.asarray(ix._raw_blob())
    assert np.array_equal(_links(blob, ix._node_size_bytes, 2 * dim, N), _links(o.blob(), o.node_size, 4 * dim, N))
    assert np.array_equal(_vectors(blob, ix._node_size_bytes, 2 * dim, N).view(np.float16), X)


@pytest.mark.parametrize("metric", ["l2", "angular"])
def test_host_build_on_gaussian_data_equals_widened_float32_build(flatnav, metric):
    # any data: the host distances widen both operands and run the float32 kernels, so links equal a float32 build
    N, dim, M = 1000, 24, 12
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, dim)).astype(np.float16)
    if metric == "angular":
        X = (X.astype(np.float32) / np.linalg.norm(X.astype(np.float32), axis=1, keepdims=True)).astype(np.float16)
    DT = flatnav.data_type.DataType
    a = flatnav.index.create(distance_type=metric, index_data_type=DT.float16, dim=dim, dataset_size=N, max_edges_per_node=M)
    b = flatnav.index.create(distance_type=metric, index_data_type=DT.float32, dim=dim, dataset_size=N, max_edges_per_node=M)
    a.add(X, 50)
    b.add(X.astype(np.float32), 50)
    la = _links(a._raw_blob(), a._node_size_bytes, 2 * dim, N)
    lb = _links(b._raw_blob(), b._node_size_bytes, 4 * dim, N)
    assert np.array_equal(la, lb)


def test_float_inputs_are_rounded_to_nearest_even(flatnav):
    N, dim, M = 300, 20, 8
    rng = np.random.default_rng(3)
    X64 = rng.standard_normal((N, dim)) * 10.0
    X64[0, :4] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 1e-6]  # ties to even, the largest finite, a subnormal

    def blob(X):
        ix = flatnav.index.create("l2", dim, N, M, flatnav.data_type.DataType.float16)
        ix.add(X, 32)
        return np.array(ix._raw_blob())

    ref = X64.astype(np.float16)  # numpy: one rounding, nearest even (float64 -> float32 -> float16 may round twice)
    for X in (X64, X64.astype(np.float32), np.asfortranarray(X64)):
        b = blob(X)
        assert np.array_equal(b, blob(X.astype(np.float16))), X.dtype
    assert np.array_equal(_vectors(blob(X64), 2 * dim + 4 * M + 4, 2 * dim, N).view(np.float16), ref)
    # allocate_nodes stores float16 rows too
    ix = flatnav.index.create("l2", dim, N, M, flatnav.data_type.DataType.float16)
    ix.allocate_nodes(X64[:5])
    assert np.array_equal(_vectors(ix._raw_blob(), 2 * dim + 4 * M + 4, 2 * dim, 5).view(np.float16), ref[:5])


@pytest.mark.parametrize("metric", ["l2", "angular"])
def test_save_and_load(flatnav, tmp_path, metric):
    N, dim, M = 500, 33, 12
    X = np.random.default_rng(8).standard_normal((N, dim)).astype(np.float16)
    ix = flatnav.index.create(metric, dim, N, M, flatnav.data_type.DataType.float16)
    ix.add(X, 40)
    p = str(tmp_path / "f16.bin")
    ix.save(p)
    raw = open(p, "rb").read()
    hdr = struct.unpack("<i7Q", raw[:60])
    assert hdr == (8, M, 2 * dim, 2 * dim + 4 * M + 4, N, N, dim, 2 * dim)
    cls = flatnav.index.IndexL2Float16 if metric == "l2" else flatnav.index.IndexIPFloat16
    loaded = cls.load_index(p)
    assert np.array_equal(np.asarray(loaded._raw_blob()), np.asarray(ix._raw_blob()))
    assert loaded._data_size_bytes == 2 * dim


def test_npy_reader_and_host_conversions(tmp_path):
    # the C++ float16 helpers (widen exact, narrow nearest-even) and the '<f2' .npy path, against numpy, with and without F16C
    import subprocess

    from flatnav_amd import build_host

    src = tmp_path / "f16.cpp"
    src.write_text(r'''
#include <cstdio>
#include <vector>
#include <flatnav/util/NpyReader.h>
using namespace flatnav::util;
int main(int, char** argv) {
  NpyArray h = loadNpy(argv[1]), f = loadNpy(argv[2]);
  std::vector<float> wide = h.as<float>();
  std::vector<float16_t> nar = f.as<float16_t>(), same = h.as<float16_t>();
  std::vector<float> bulk(wide.size());
  widen(same.data(), bulk.data(), same.size());
  std::vector<float16_t> bulk_n(f.numValues());
  narrow(reinterpret_cast<const float*>(f.bytes.data()), bulk_n.data(), bulk_n.size());
  saveNpy(argv[3], wide.data(), {wide.size()}, "<f4", 4);
  saveNpy(argv[4], nar.data(), {nar.size()}, "<f2", 2);
  saveNpy(argv[5], bulk.data(), {bulk.size()}, "<f4", 4);
  saveNpy(argv[6], bulk_n.data(), {bulk_n.size()}, "<f2", 2);
  return 0;
}
''')
    every_half = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32)
    fl = np.concatenate([bits.view(np.float32), rng.standard_normal(10_000).astype(np.float32),
                         (np.arange(-70000, 70000, 0.25)).astype(np.float32),
                         every_half.astype(np.float32) * np.float32(1 + 2.0 ** -12)])  # near ties
    fl = fl[~np.isnan(fl)]
    np.save(tmp_path / "h.npy", every_half)
    np.save(tmp_path / "f.npy", fl)
    for flags in ([], ["-mno-f16c"]):
        exe = str(tmp_path / ("conv" + "".join(flags)))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-march=x86-64-v3"] + flags + [
            "-I" + build_host.ROOT + "/include", str(src), "-o", exe])
        outs = [str(tmp_path / ("o%d.npy" % i)) for i in range(4)]
        subprocess.check_call([exe, str(tmp_path / "h.npy"), str(tmp_path / "f.npy")] + outs)
        wide, nar, bulk, bulk_n = (np.load(o) for o in outs)
        want_w = every_half.astype(np.float32)
        assert np.array_equal(wide.view(np.uint32), want_w.view(np.uint32)) or \
            np.array_equal(np.isnan(wide), np.isnan(want_w)) and np.array_equal(wide[~np.isnan(wide)], want_w[~np.isnan(want_w)])
        assert np.array_equal(bulk.view(np.uint32), wide.view(np.uint32))
        assert np.array_equal(nar.view(np.uint16), fl.astype(np.float16).view(np.uint16)), flags
        assert np.array_equal(bulk_n.view(np.uint16), nar.view(np.uint16)), flags
