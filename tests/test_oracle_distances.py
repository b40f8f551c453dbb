"""Pin the oracle's distance functions against the REFERENCE's own compiled code
(oracle/_ref, built from the reference's include/ in the dev container; its answers on these inputs are stored in
tests/golden/reference/answers.npz, see conftest.ReferenceAnswers) and the reference's known answers
(include/flatnav/tests/test_distances.cpp:31-179)."""
import ctypes as C

import numpy as np
import pytest

DIMS = [128, 100, 37, 7, 768, 500, 64, 16, 4]


def _call(fn, x, y):
    return float(fn(x.ctypes.data, y.ctypes.data, x.shape[0]))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_float_integer_valued_is_bit_exact(oracle_mod, ref_answers, dim, metric):
    # Integer-valued float32 (SIFT-like 0..255): every partial sum is an exact integer < 2^24,
    # so the reference's SIMD order, the oracle's order and the GPU's order must agree exactly.
    rng = np.random.default_rng(dim * 7 + (metric == "ip"))
    hi = 256 if metric == "l2" else 16  # keep |sum| < 2^24 for inner products too
    pairs = [(rng.integers(0, hi, dim).astype(np.float32), rng.integers(0, hi, dim).astype(np.float32)) for _ in range(200)]
    want = ref_answers("distances/int_valued/%s_f32/%d" % (metric, dim),
                       lambda ref: [_call(getattr(ref, "ref_%s_f32" % metric), x, y) for x, y in pairs])
    for (x, y), w in zip(pairs, want):
        assert oracle_mod.distance(metric, x, y) == w


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_float_general_within_tolerance(oracle_mod, ref_answers, dim, metric):
    # Same inputs as the reference's own test (N(0,10^2)); its tolerance is 1e-2 absolute at ~2.5e4
    # (test_distances.cpp:31).  We hold the tighter contract stated in DESIGN.md: rtol 1e-5.
    rng = np.random.default_rng(1000 + dim)
    pairs = [(rng.normal(0, 10, dim).astype(np.float32), rng.normal(0, 10, dim).astype(np.float32)) for _ in range(100)]
    want = ref_answers("distances/general/%s_f32/%d" % (metric, dim), lambda ref: [
        [_call(getattr(ref, "ref_%s_f32" % metric), x, y), _call(getattr(ref, "ref_default_%s_f32" % metric), x, y)] for x, y in pairs])
    for (x, y), (w, wd) in zip(pairs, want):
        o = oracle_mod.distance(metric, x, y)
        scale = float(np.abs(x.astype(np.float64) * y).sum() + (x.astype(np.float64) ** 2).sum()) + 1.0
        assert abs(o - w) <= 1e-5 * scale
        assert abs(o - wd) <= 1e-5 * scale
        exact = ((x.astype(np.float64) - y) ** 2).sum() if metric == "l2" else 1.0 - (x.astype(np.float64) * y).sum()
        assert abs(o - exact) <= 1e-5 * scale


@pytest.mark.parametrize("dim", [128, 64, 100, 37, 7, 500])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dt", ["uint8", "int8"])
def test_integer_dtypes_exact_below_2p24(oracle_mod, ref_answers, dim, metric, dt):
    rng = np.random.default_rng(dim)
    lo, hi = (0, 256) if dt == "uint8" else (-128, 128)
    if dim * 255 * 255 >= 2 ** 24:  # keep the reference's float accumulation exact
        lo, hi = (0, 100) if dt == "uint8" else (-100, 100)
    name = "ref_%s_%s" % (metric, "u8" if dt == "uint8" else "i8")
    pairs = [(rng.integers(lo, hi, dim).astype(dt), rng.integers(lo, hi, dim).astype(dt)) for _ in range(200)]
    answers = ref_answers("distances/%s/%d" % (name, dim), lambda ref: [_call(getattr(ref, name), x, y) for x, y in pairs])
    for (x, y), want in zip(pairs, answers):
        assert oracle_mod.distance(metric, x, y) == want
        xi, yi = x.astype(np.int64), y.astype(np.int64)
        exact = float(((xi - yi) ** 2).sum()) if metric == "l2" else 1.0 - float((xi * yi).sum())
        assert want == np.float32(exact)


def test_reference_known_answers(ref_answers):
    # test_distances.cpp:84-100 -- reduce_add of (1..8) == 36 and (1..4) == 10.
    v8 = np.arange(1, 9, dtype=np.float32)
    v4 = np.arange(1, 5, dtype=np.float32)
    got = ref_answers("reduce_add/8_4", lambda ref: [ref.ref_reduce_add8(v8.ctypes.data), ref.ref_reduce_add4(v4.ctypes.data)])
    assert got[0] == 36.0
    assert got[1] == 10.0


def test_reference_simd_matches_its_scalar_definition(ref_answers):
    # The reference's own assertion (SIMD == scalar +- 1e-2) re-run on its compiled code for the
    # dimension classes its dispatcher distinguishes (dim%16, dim%4, residuals).
    rng = np.random.default_rng(5)
    for dim in (128, 100, 37, 7):
        x = rng.normal(0, 10, dim).astype(np.float32)
        y = rng.normal(0, 10, dim).astype(np.float32)
        l2, l2d, ip, ipd = ref_answers("simd_vs_scalar/%d" % dim, lambda ref: [
            _call(ref.ref_l2_f32, x, y), _call(ref.ref_default_l2_f32, x, y), _call(ref.ref_ip_f32, x, y),
            _call(ref.ref_default_ip_f32, x, y)])
        assert abs(l2 - l2d) < 1e-2
        assert abs(ip - ipd) < 1e-2


def test_visited_set_matches_reference(ref_answers):
    # util/VisitedSetPool.h:16-50: 8-bit epoch mark, memset on wrap (every 255th clear).
    n = 64
    rng = np.random.default_rng(0)
    inserts = [rng.integers(0, n, 5) for _ in range(600)]

    def trace(ref):  # per clear: the mark, then is_visited of every slot after that round's inserts
        vs = ref.ref_vs_new(n)
        try:
            out = np.zeros((600, n + 1), dtype=np.uint8)
            for it in range(600):
                ref.ref_vs_clear(vs)
                out[it, 0] = ref.ref_vs_mark(vs)
                for i in inserts[it]:
                    ref.ref_vs_insert(vs, int(i))
                out[it, 1:] = [bool(ref.ref_vs_is_visited(vs, i)) for i in range(n)]
            return out
        finally:
            ref.ref_vs_free(vs)

    got = ref_answers("visited_set/trace", trace)
    mark = 1
    table = np.zeros(n, dtype=np.uint8)
    for it in range(600):
        mark = (mark + 1) & 0xFF
        if mark == 0:
            table[:] = 0
            mark = 1
        assert got[it, 0] == mark
        for i in inserts[it]:
            table[i] = mark
        for i in range(n):
            assert bool(got[it, 1 + i]) == (table[i] == mark)
