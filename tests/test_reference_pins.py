"""The cereal-free parts of the reference that the product re-implements on the host, pinned against the EXECUTED reference
(oracle/_ref = the reference's own headers compiled where they lie, oracle/ref_cereal_free.cpp; its answers on these inputs
are stored in tests/golden/reference/answers.npz, see conftest.ReferenceAnswers):

  * include/flatnav/util/Reordering.h  gOrder / rcmOrder  == reference Reordering.h:27-200 + GorderPriorityQueue.h:14-109 --
    the SAME PERMUTATION, element for element, ties in score / degree included ("pinned, not isomorphic");
  * include/flatnav/util/Multithreading.h  executeInParallel  == reference Multithreading.h:19-48 (every index exactly once,
    extra arguments forwarded, zero threads -> std::invalid_argument);
  * include/flatnav/util/Datatype.h  ordinals / names / sizes  == reference Datatype.h:11-186 (the ordinal is the first
    int32 of a saved index file and the C ABI's FNV_DTYPE_*).

The product side is compiled by this test from the product's headers (tests/cpp/host_utils_shim.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def own(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim") / "libhost_utils_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_utils_shim.cpp"), "-o", out])
    L = C.CDLL(out)
    L.own_gorder.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    L.own_rcm.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.own_execute_in_parallel.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.own_datatype_name.restype = C.c_char_p
    L.own_datatype_name.argtypes = [C.c_int]
    L.own_datatype_ordinal.argtypes = [C.c_char_p]
    for name in ("own_datatype_size", "own_datatype_ctype_bytes"):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_int]
    L.own_datatype_enum_bytes.restype = C.c_uint64
    return L


def _csr(table):
    offsets = np.zeros(len(table) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in table])
    flat = np.array([v for r in table for v in r] + [0], dtype=np.uint32)  # (+ one element: never an empty buffer)
    return flat, offsets


def _random_graph(rng, kind):
    """Out-degree tables as Index::getGraphOutdegreeTable leaves them (no self-loops in a row, ids < n), in several shapes:
    equal degrees everywhere (every comparison a tie), ragged rows, isolated nodes, a ring, duplicate edges."""
    n = int(rng.integers(2, 400))
    if kind == "regular":
        M = int(rng.integers(1, min(n, 9)))
        return [list(rng.choice([u for u in range(n) if u != v] or [v], size=min(M, n - 1), replace=False)) for v in range(n)]
    if kind == "ragged":
        return [list(rng.choice(n, size=int(rng.integers(0, min(n, 12))), replace=False)) for v in range(n)]
    if kind == "ring":
        return [[(v + 1) % n, (v + 2) % n] for v in range(n)]
    if kind == "sparse":  # many isolated nodes and components
        return [list(rng.choice(n, size=int(rng.integers(0, 2)), replace=False)) if rng.random() < 0.6 else [] for v in range(n)]
    return [list(rng.integers(0, n, size=int(rng.integers(0, 8)))) for v in range(n)]  # "dupes": repeated targets allowed


KINDS = ["regular", "ragged", "ring", "sparse", "dupes"]


def _ref_orders(ref, flat, offsets, n, ws):
    """The reference's gOrder(table, w) for every w of `ws`, then its rcmOrder(table): one row each."""
    out = np.empty((len(ws) + 1, n), np.uint32)
    for j, w in enumerate(ws):
        ref.ref_gorder(flat.ctypes.data, offsets.ctypes.data, n, w, out[j].ctypes.data)
    ref.ref_rcm(flat.ctypes.data, offsets.ctypes.data, n, out[-1].ctypes.data)
    return out


def test_gorder_and_rcm_return_the_references_permutation(own, ref_answers):
    rng = np.random.default_rng(60)
    checked = 0
    WS = (5, 1, 0, 2, 17)  # Index.h:418,429 uses w = 5
    for trial in range(60):
        table = _random_graph(rng, KINDS[trial % len(KINDS)])
        n = len(table)
        flat, offsets = _csr(table)
        want = ref_answers("reordering/random_graph/%d" % trial, lambda ref: _ref_orders(ref, flat, offsets, n, WS))
        for j, w in enumerate(WS):
            a, b = want[j], np.empty(n, np.uint32)
            own.own_gorder(flat.ctypes.data, offsets.ctypes.data, n, w, b.ctypes.data)
            assert np.array_equal(a, b), (trial, KINDS[trial % len(KINDS)], n, w)
            assert sorted(a.tolist()) == list(range(n))
        a, b = want[-1], np.empty(n, np.uint32)
        own.own_rcm(flat.ctypes.data, offsets.ctypes.data, n, b.ctypes.data)
        assert np.array_equal(a, b), (trial, KINDS[trial % len(KINDS)], n)
        assert sorted(a.tolist()) == list(range(n))
        checked += 1
    assert checked == 60


def test_gorder_and_rcm_on_a_real_index_graph(own, ref_answers, oracle_mod):
    # the out-degree table of a built index (Index.h:240-260: links that are not self-loops), 3000 nodes, M = 16
    from flatnav_amd import datasets as ds

    X, _ = ds.sift_like(3000, 1)
    ix = oracle_mod.OracleIndex.create("l2", 128, 3000, 16)
    ix.add(X, 48)
    blob = np.asarray(ix.blob()).reshape(3000, ix.node_size)
    links = blob[:, ix.data_size:ix.data_size + 64].copy().view(np.uint32)
    table = [[int(v) for v in links[u] if v != u] for u in range(3000)]
    flat, offsets = _csr(table)
    want = ref_answers("reordering/index_graph_3000", lambda ref: _ref_orders(ref, flat, offsets, 3000, (5,)))
    for a, fn_own, args in ((want[0], own.own_gorder, (5,)), (want[1], own.own_rcm, ())):
        b = np.empty(3000, np.uint32)
        fn_own(flat.ctypes.data, offsets.ctypes.data, 3000, *args, b.ctypes.data)
        assert np.array_equal(a, b)


def test_execute_in_parallel_covers_every_index_once(own, ref_answers):
    def run(fn, start, end, threads, extra):  # -> [return code] + the hit count of every index
        hits = np.zeros(max(1, end - start), dtype=np.uint32)
        return np.concatenate([[fn(start, end, threads, extra, hits.ctypes.data)], hits]).astype(np.int64)

    for start, end, threads, extra in ((0, 1000, 4, 0), (7, 8, 3, 2), (5, 5, 2, 0), (9, 3, 2, 1), (0, 50000, 8, 3), (0, 13, 1, 0)):
        n = max(0, end - start)
        args = (start, end, threads, extra)
        got = [ref_answers("execute_in_parallel/%d_%d_%d_%d" % args, lambda ref: run(ref.ref_execute_in_parallel, *args)),
               run(own.own_execute_in_parallel, *args)]
        assert got[0][0] == 0 and got[1][0] == 0
        assert np.array_equal(got[0], got[1])
        assert (got[1][1:n + 1] == 1 + extra).all()  # each index handed out exactly once, the extra argument forwarded by value
    # Multithreading.h:22-24: zero threads -> an error, nothing run
    assert ref_answers("execute_in_parallel/zero_threads", lambda ref: run(ref.ref_execute_in_parallel, 0, 4, 0, 0)).tolist() == [1, 0, 0, 0, 0]
    assert run(own.own_execute_in_parallel, 0, 4, 0, 0).tolist() == [1, 0, 0, 0, 0]


LABELS = ("uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64", "float16", "float32", "float64", "undefined",
          "bfloat16", "")


def _datatype_numbers(L, p):
    """enum size, then size / ctype bytes of ordinals 0..13, then the ordinal of every label -- of the reference (p = "ref_")
    or of the product's header (p = "own_")."""
    f = lambda name: getattr(L, p + name)  # noqa: E731
    return np.array([f("datatype_enum_bytes")()] + [v for o in range(14) for v in (f("datatype_size")(o), f("datatype_ctype_bytes")(o))] +
                    [f("datatype_ordinal")(label.encode()) for label in LABELS], dtype=np.int64)


def _datatype_names(L, p):
    return np.array([getattr(L, p + "datatype_name")(o) or b"<null>" for o in range(14)])


def test_datatype_ordinals_names_and_sizes(own, ref_answers):
    from flatnav_amd import hip
    from oracle import oracle as orc

    want_numbers = ref_answers("datatype/numbers", lambda ref: _datatype_numbers(ref, "ref_"))
    want_names = ref_answers("datatype/names", lambda ref: _datatype_names(ref, "ref_"))
    assert want_numbers[0] == 4  # the int32 at offset 0 of an index file
    assert np.array_equal(_datatype_numbers(own, "own_"), want_numbers)
    assert np.array_equal(_datatype_names(own, "own_"), want_names)
    # the three index element types: the ordinals the oracle, the ctypes binding and the C ABI use are the reference's
    ordinal_of = dict(zip(LABELS, want_numbers[1 + 2 * 14:].tolist()))
    for label, ordinal in (("uint8", 0), ("int8", 4), ("float32", 9)):
        assert ordinal_of[label] == ordinal == orc.DTYPE_ORD[label] == hip.DTYPE_ORD[label]


@pytest.mark.parametrize("methods", [["gorder"], ["rcm"], ["gorder", "rcm"]], ids=["gorder", "rcm", "gorder+rcm"])
def test_index_reorder_applies_the_references_permutation(ref_answers, methods):
    # The whole product path Index::doGraphReordering -> relabel (reference Index.h:412-440, 872-926) through the Python
    # surface: after reorder(methods) node u sits at P[u] with every link rewritten through P and its label travelling along,
    # where P is what the REFERENCE's gOrder(table, 5) / rcmOrder(table) return on the table before.  No GPU involved.
    import hashlib

    from flatnav_amd import build_host

    build_host.build()
    import flatnav_amd as flatnav

    rng = np.random.default_rng(len(methods) * 7 + len(methods[0]))
    N, dim, M = 1500, 16, 8
    X = rng.integers(0, 12, (N, dim)).astype(np.uint8)  # tie-heavy: many equal degrees and equal scores
    ix = flatnav.index.create("l2", dim, N, M, flatnav.data_type.DataType.uint8)
    ix.add(X, 32, labels=[int(v) for v in rng.permutation(N) + 100])
    node = ix._node_size_bytes

    def rows():
        blob = np.asarray(ix._raw_blob()).reshape(N, node)
        return (blob[:, :dim].copy(), blob[:, dim:dim + 4 * M].copy().view(np.uint32), blob[:, dim + 4 * M:].copy().view(np.int32).ravel())

    vec, links, labels = rows()
    for method in methods:
        table = ix.get_graph_outdegree_table()
        assert table == [[int(v) for v in links[u] if v != u] for u in range(N)]  # Index.h:240-260
        flat, offsets = _csr(table)
        # (keyed by the table itself: a stored permutation only ever answers the table it was computed on)
        key = hashlib.sha256(flat.tobytes() + offsets.tobytes()).hexdigest()[:16]
        P = ref_answers("reordering/index_reorder/%s/%s" % (method, key),
                        lambda ref: _ref_orders(ref, flat, offsets, N, (5,))[0 if method == "gorder" else 1])
        want_vec, want_links, want_labels = np.empty_like(vec), np.empty_like(links), np.empty_like(labels)
        want_vec[P], want_links[P], want_labels[P] = vec, P[links], labels
        ix.reorder([method])
        vec, links, labels = rows()
        assert np.array_equal(vec, want_vec) and np.array_equal(labels, want_labels)
        assert np.array_equal(links, want_links)
