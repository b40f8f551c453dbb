"""The row geometry classes of tests/row_classes.py, on the CPU: what the planner can produce over dims 1 .. 9000, that the
pinned class list is exactly that, which kernel slots are reachable at all -- and that DESIGN section 8's float bar is one a
float32 sum can meet at every class's dim, before tests/test_gpu_row_classes.py holds the kernels to it."""
import numpy as np
import pytest

import row_classes as rc

RTOL, ATOL = 1e-5, 1e-6  # the float bar
SHAPE_TEST_DIMS = (7, 100, 128, 200, 768)  # test_gpu_filtered / test_gpu_exhaustive / test_gpu_grouped_filters: "every kernel shape"


@pytest.fixture(autouse=True)
def default_layout(monkeypatch):
    for name in rc.LAYOUT_ENV:
        monkeypatch.delenv(name, raising=False)
    rc.walk.cache_clear()
    yield
    rc.walk.cache_clear()


def test_the_walk_finds_the_pinned_classes():
    """A planner change that creates (or loses) a class fails here until CLASSES -- the list the GPU file is parametrised
    over -- names it."""
    print("\nsmallest dim of each reachable row geometry class, dims 1 .. %d\n%s" % (rc.MAX_DIM, rc.format_table()))
    for dtype in rc.TYPES:
        found = rc.walk(dtype)
        assert len(found) == 18, (dtype, sorted(found))
        assert sorted(found) == sorted(rc.CLASSES), (dtype, set(found) ^ set(rc.CLASSES))
        assert sum(c.n_dims for c in found.values()) == rc.MAX_DIM  # every dim is in exactly one class
        scale = {"float32": 1, "float16": 2, "uint8": 4, "int8": 4}[dtype]
        # a class is a property of the row's bytes: the same table for every element size, in dims of that size
        assert {n: c.dim for n, c in found.items()} == {n: (c.dim - 1) * scale + 1 for n, c in rc.walk("float32").items()}, dtype
    assert rc.walk("uint8") == rc.walk("int8")


def test_reachable_kernel_slots():
    """Every [cfg][full] slot of the kernel table but one is reached; rows of exactly 192 chunks are never clamped (their
    configuration is picked by that very length), and a clamped three-line row does not exist: non-FULL there IS the split
    row, with one or two side-table chunks."""
    table = rc.cfgs()
    for dtype in rc.TYPES:
        keys = set(rc.keys_of(dtype, np.arange(1, rc.MAX_DIM + 1)))
        slots = {(cfg, full) for cfg, full, _, _ in keys}
        g64x3, g8x3 = table.index((64, 3)), table.index((8, 3))
        assert slots == {(c, f) for c in range(len(table)) for f in (0, 1)} - {(g64x3, 0)}, dtype
        assert (g64x3, 0, 0, False) not in keys and (g8x3, 0, 0, False) not in keys
        assert {k for k in keys if k[0] == g8x3} == {(g8x3, 1, 0, False), (g8x3, 0, 1, False), (g8x3, 0, 2, False)}
        assert all(tail == 0 for cfg, _, tail, _ in keys if cfg != g8x3)
        assert {k[0] for k in keys if k[3]} == {table.index((64, 4))}  # only the widest configuration loops over spans


def test_dims_of_the_shape_tests_fall_in_listed_classes():
    reached = {}
    for dtype in rc.TYPES:
        reached[dtype] = {rc.class_of(dtype, d) for d in SHAPE_TEST_DIMS}
        assert reached[dtype] <= set(rc.CLASSES), dtype
    # what those five dims reach, of eighteen: the reason tests/test_gpu_row_classes.py exists
    assert reached["float32"] == {"8x1-clamped", "8x3-tail1", "8x4-full", "16x4-clamped", "64x3-full"}
    assert reached["float16"] == {"8x1-clamped", "8x2-full", "8x3-tail1", "32x4-clamped"}
    assert reached["uint8"] == reached["int8"] == {"8x1-clamped", "8x1-full", "8x2-full", "16x4-clamped"}


def test_representative_dims_are_the_smallest_of_their_class():
    for dtype in rc.TYPES:
        for c in rc.walk(dtype).values():
            assert rc.class_of(dtype, c.dim) == c.name
            assert c.dim == 1 or rc.class_of(dtype, c.dim - 1) != c.name
    # the long-row case of the GPU file
    assert rc.class_of("float32", 5200) == "64x4-clamped-spans"


def test_clamped_classes_have_a_dense_dim():
    """At the smallest dim of a class whose rows are padded to whole lines the row's last chunk is zero padding: a clamped lane
    re-reads zeros there.  The dense dim is the smallest of the same class whose last chunk is data."""
    for dtype in rc.TYPES:
        esize = rc.ELEM_BYTES[dtype]
        for c in rc.walk(dtype).values():
            if c.full or c.tail_chunks:
                assert [n for n, _ in rc.representatives(dtype, c.name)] == [c.name]
                continue
            assert c.dense_dim is not None and rc.class_of(dtype, c.dense_dim) == c.name, (dtype, c.name)
            assert rc.geometry(dtype, [c.dense_dim])[2][0] == c.dense_dim * esize
            between = np.arange(c.dim, c.dense_dim)
            assert (rc.geometry(dtype, between)[2] != between * esize).all(), (dtype, c.name)  # ... and no smaller dim is dense
            assert rc.representatives(dtype, c.name) == [(c.name, c.dim), (c.name + "-dense", c.dense_dim)]
            assert rc.dim_of(dtype, c.name + "-dense") == c.dense_dim and rc.dim_of(dtype, c.name) == c.dim
            padded_to_lines = rc.geometry(dtype, [c.dim])[2][0] % 128 == 0
            last_chunk_is_padding = rc.geometry(dtype, [c.dim])[2][0] - c.dim * esize >= 16
            assert last_chunk_is_padding == (padded_to_lines and c.G > 8), (dtype, c.name)  # 16x4, 32x4, 64x4: both spans forms
    assert len(rc.CASES) == 18 + 7 and sorted(set(rc.CASES)) == sorted(rc.CASES)


def test_a_float32_sum_in_another_order_stays_inside_the_float_bar():
    """Before the kernels are held to rtol 1e-5 / atol 1e-6 against float64 at every class's dim: a plain float32 evaluation on
    the CPU -- numpy's pairwise sum, and the strictly sequential sum, the worst order there is -- stays inside that bar on the
    rows of the GPU file's float cases and the first 8 of their 40 queries, at every dim that file uses.  Measured: worst |error| / tolerance = 0.060 pairwise (float32 ip, dim 4), 0.36 sequential (float16 l2, dim 4033:
    the longest sum of the largest terms); a kernel, which sums partial sums of lanes, sits between the two."""
    worst = {"pairwise": (0.0, None), "sequential": (0.0, None)}
    for dtype in ("float32", "float16"):
        for metric in ("l2", "ip"):
            for name, dim in [r for c in rc.CLASSES for r in rc.representatives(dtype, c)]:
                X, Q = rc.float_case(dtype, metric, dim)
                X32, X64 = X.astype(np.float32), X.astype(np.float64)
                per_class = {"pairwise": 0.0, "sequential": 0.0}
                for q in Q[:8]:  # (the first 8 of the GPU file's 40 queries)
                    terms32 = (X32 - q.astype(np.float32)) ** 2 if metric == "l2" else X32 * q.astype(np.float32)
                    terms64 = (X64 - q.astype(np.float64)) ** 2 if metric == "l2" else X64 * q.astype(np.float64)
                    want = terms64.sum(1) if metric == "l2" else 1.0 - terms64.sum(1)
                    tol = ATOL + RTOL * np.abs(want)
                    for how, s in (("pairwise", terms32.sum(1, dtype=np.float32)), ("sequential", np.cumsum(terms32, axis=1, dtype=np.float32)[:, -1])):
                        got = s if metric == "l2" else np.float32(1.0) - s
                        per_class[how] = max(per_class[how], float((np.abs(got.astype(np.float64) - want) / tol).max()))
                print("float bar on the CPU: %-8s %-2s %-24s dim %4d: worst |error| / tolerance = %.4f pairwise, %.4f sequential" %
                      (dtype, metric, name, dim, per_class["pairwise"], per_class["sequential"]))
                for how, v in per_class.items():
                    if v > worst[how][0]:
                        worst[how] = (v, (dtype, metric, name, dim))
    print("float bar on the CPU: worst of all: %r" % (worst,))
    assert worst["pairwise"][0] <= 1.0 and worst["sequential"][0] <= 1.0, worst
