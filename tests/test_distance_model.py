"""The CPU model of the float distance arithmetic (tests/distance_model.py, tests/distance_model_harness.cpp) before a GPU sees
it: for every case of row_classes.CASES, float32 and float16, L2 and IP --

* the model meets DESIGN section 8's float bar against float64 on the data tests/test_gpu_distance_bits.py uses;
* on FULL float32 rows its batched entry point equals hrh_dist_f32, and hrh_dist_half on the mirror of lossless rows, in all
  five mirror configurations;
* on integer-valued data with sums below 2^24 it gives the exact integer -- float16 IP also under every candidate semantics of
  the two-element dot, so the mode in force cannot disturb the integer contract;
* the recorded probe of v_dot2_f32_f16 (tests/golden/probes/dot2_probe.npz) still says what profiles/distance_bits.md says;
* each of six deviations a kernel could have (the harness's mutants) changes distance bits wherever it can."""
import fractions
import os

import numpy as np
import pytest

import distance_model as dm
import row_classes as rc
import test_half_rows as thr

TYPES = ("float32", "float16")
METRICS = ("l2", "ip")
NP_T = {"float32": np.float32, "float16": np.float16}
EPC = {"float32": 4, "float16": 8}
PARAMS = [(t, m, c) for t in TYPES for m in METRICS for c in rc.CASES]
QUERIES = np.r_[0:dm.NQ:4, 1:dm.NQ:8]  # every query a row copies, and five others
MIRROR_CASES = ("8x2-full", "8x4-full", "16x4-full", "32x4-full", "64x4-full", "64x4-full-spans")


def data_sets(dtype, metric, case):
    """[(name, rows, queries)] of one case as the GPU file builds them."""
    dim = rc.dim_of(dtype, case)
    out = [("real", *rc.float_case(dtype, metric, dim)), ("edges", *dm.edge_case(dtype, metric, dim, dtype == "float32" and case in MIRROR_CASES))]
    return dim, out


@pytest.mark.parametrize("dtype,metric,case", PARAMS, ids=lambda p: str(p))
def test_the_model_meets_the_float_bar(dtype, metric, case):
    dim, sets = data_sets(dtype, metric, case)
    for name, X, Q in sets:
        Q = Q[QUERIES]
        D = dm.dist64(X, Q, metric)
        dm.assert_finite(D, (dtype, metric, case, name))
        bits = dm.distances(dtype, metric, X, Q)
        ok, worst = dm.within_float_bar(bits, D)
        print("distance model, float bar: %s %s %s dim %d %s: worst |error| / tolerance = %.4f" % (dtype, metric, case, dim, name, worst))
        assert ok, (dtype, metric, case, name, worst)
        if name == "edges" and metric == "l2":  # a row that copies its query is at +0
            for i in range(1, len(X), 10):
                col = np.flatnonzero(QUERIES == dm.copies_of(i))
                assert (bits[col, i] == 0).all(), (dtype, case, i)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", [c for c in rc.CASES if c.endswith("full") or c.endswith("full-spans")])
def test_full_float32_rows_equal_the_two_emulations(case, metric):
    """The batched entry point on FULL rows = hrh_dist_f32 pair by pair; where the rows have a mirror (five configurations, one
    of them at one span and at several) = hrh_dist_half on the converted rows: what tests/test_half_rows.py checks between the
    two emulations on its own shapes, here on the GPU file's rows."""
    L, H = dm.lib(), thr.lib()
    dim = rc.dim_of("float32", case)
    geo = rc.walk_of_row("float32", dim)
    assert geo["full"] and not geo["tail_chunks"]
    G, CU, nchunks = geo["G"], geo["CU"], geo["nchunks"]
    has_mirror = bool(H.hrh_eligible_cfg(thr.F32, geo["cfg"], 1, 0))
    assert has_mirror == (case in MIRROR_CASES)
    X, Q = dm.edge_case("float32", metric, dim, has_mirror)
    X, Q = X[:60], Q[:12]
    bits = dm.distances("float32", metric, X, Q)
    Xp, Qp = dm.padded(X, geo), dm.padded(Q, geo)
    m = dm.METRIC_ORD[metric]
    f32 = np.array([[L.hrh_dist_f32(q.ctypes.data, x.ctypes.data, nchunks, G, CU, m) for x in Xp] for q in Qp], np.float32)
    assert np.array_equal(bits, f32.view(np.uint32))
    if has_mirror:
        mirror = np.zeros((len(Xp), nchunks * 4), np.uint16)
        for x, u in zip(Xp, mirror):
            assert H.hrh_convert_row(x.ctypes.data, u.ctypes.data, nchunks, G, CU) == 1  # lossless
        half = np.array([[L.hrh_dist_half(q.ctypes.data, u.ctypes.data, nchunks, G, CU, m, 0) for u in mirror] for q in Qp], np.float32)
        assert np.array_equal(bits, half.view(np.uint32))
        swapped = np.array([[L.hrh_dist_half(q.ctypes.data, u.ctypes.data, nchunks, G, CU, m, 1) for u in mirror] for q in Qp], np.float32)
        assert not np.array_equal(bits, swapped.view(np.uint32))


@pytest.mark.parametrize("dtype,metric,case", PARAMS, ids=lambda p: str(p))
def test_integer_valued_data_gives_the_exact_integer(dtype, metric, case):
    dim = rc.dim_of(dtype, case)
    rng = np.random.default_rng(dim + 17)
    if metric == "ip":
        lo, hi = -8, 9
    else:
        lo, hi = 0, min(60, int(np.sqrt((2 ** 24 - 1) / dim))) + 1
    X, Q = rng.integers(lo, hi, (80, dim)), rng.integers(lo, hi, (10, dim))
    want = ((Q[:, None, :] - X[None, :, :]) ** 2).sum(2) if metric == "l2" else 1 - Q @ X.T
    assert np.abs(want).max() < 2 ** 24
    want = want.astype(np.float32).view(np.uint32)
    X, Q = X.astype(NP_T[dtype]), Q.astype(NP_T[dtype])
    modes = [dm.DOT_NONE] + dm.DOT_MODES if (dtype, metric) == ("float16", "ip") else [dm.DOT_MODE]
    for mode in modes:
        assert np.array_equal(dm.distances(dtype, metric, X, Q, dot_mode=mode), want), (dtype, metric, case, dm.mode_name(mode))


# ---- the two-element dot's candidates -------------------------------------------------------------------------------------------
def _round_f32(v: fractions.Fraction) -> np.uint32:
    """v, a whole number of 2^-149, rounded to float32 (nearest, ties to even): the bits."""
    n = v * 2 ** 149
    assert n.denominator == 1
    n, sign = abs(n.numerator), 0x80000000 if v < 0 else 0
    shift = max(n.bit_length() - 24, 0)
    keep, rest = n >> shift, n & ((1 << shift) - 1)
    if shift and (rest > (1 << (shift - 1)) or (rest == (1 << (shift - 1)) and keep & 1)):
        keep += 1
    return np.float32(np.ldexp(np.float64(keep), shift - 149)).view(np.uint32) | np.uint32(sign)


def test_the_exact_dot_is_exact_and_the_candidates_differ():
    rng = np.random.default_rng(5)
    h = rng.integers(0, 1 << 16, (4000, 4)).astype(np.uint16)
    h = h[(h & 0x7C00 != 0x7C00).all(1)].view(np.float16)  # finite
    c = (rng.integers(0, 1 << 32, len(h)).astype(np.uint32) & np.uint32(0xBFFFFFFF)).view(np.float32)  # |c| < 2
    c[::3] = (rng.integers(0, 1 << 23, len(c[::3])).astype(np.uint32)).view(np.float32)  # f32 subnormals
    F = fractions.Fraction
    seen = {m: 0 for m in (dm.DOT_FMA_01, dm.DOT_FMA_10, dm.DOT_PAIR_THEN_ADD)}
    for (a0, b0, a1, b1), cc in zip(h.tolist(), c.tolist()):
        exact = F(a0) * F(b0) + F(a1) * F(b1) + F(cc)
        got = dm.dot2(a0, b0, a1, b1, cc, dm.DOT_EXACT)
        if exact != 0:
            assert got == _round_f32(exact), (a0, b0, a1, b1, cc)
        for m in seen:
            seen[m] += dm.dot2(a0, b0, a1, b1, cc, m) != got
    assert all(seen.values()), seen  # every other form rounds differently somewhere
    # the switches: a binary16 subnormal input, an f32 subnormal accumulator
    sub, acc = 2.0 ** -20, np.uint32(0x00400000).view(np.float32)
    for form in dm.DOT_FORMS:
        assert dm.dot2(sub, 1024.0, 0.0, 0.0, 0.0, form) == np.float32(2.0 ** -10).view(np.uint32)
        assert dm.dot2(sub, 1024.0, 0.0, 0.0, 0.0, form | dm.DOT_FLUSH_IN) == 0
        assert dm.dot2(0.0, 0.0, 0.0, 0.0, acc, form) == 0x00400000
        assert dm.dot2(0.0, 0.0, 0.0, 0.0, acc, form | dm.DOT_FLUSH_F32) == 0


def test_the_recorded_probe_matches_no_candidate():
    """tests/golden/probes/dot2_probe.npz: what an MI355X returned for a float16 IP index of dim 8 while Dist<_Float16, IP> was four
    v_dot2_f32_f16 per chunk (rows and queries as bit patterns, rows in node order; distance bits by (query, node)).  No
    candidate is the instruction; it keeps binary16 subnormals (a single product arrives exactly, flushing would give 1.0)."""
    z = np.load(os.path.join(dm.ROOT, "tests", "golden", "probes", "dot2_probe.npz"))
    X, Q, got = z["X"].view(np.float16), z["Q"].view(np.float16), z["bits"]
    readable = dm.dot2_readable(X, Q)
    assert readable.sum() > 500
    miss = {}
    for mode in dm.DOT_MODES:
        miss[mode] = int(((dm.distances("float16", "ip", X, Q, dot_mode=mode) != got) & readable).sum())
        print("two-element dot: %-90s misses %4d of %d readable dots" % (dm.mode_name(mode), miss[mode], int(readable.sum())))
    assert min(miss.values()) > 0
    assert all(miss[m | dm.DOT_FLUSH_IN] > miss[m] + 50 for m in dm.DOT_FORMS)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    single = ((X64[None, :, :] * Q64[:, None, :]) != 0).sum(2) == 1
    sub = (np.abs(X64[:, 1]) < 2.0 ** -14) & (X64[:, 1] != 0) & (X64[:, 0] == 0)
    assert single[30:, sub].all() and sub.sum() > 50
    assert np.array_equal(got[single], (1.0 - Q64 @ X64.T).astype(np.float32).view(np.uint32)[single])
    assert (got[30:, sub] != np.float32(1.0).view(np.uint32)).all()


# ---- mutants -----------------------------------------------------------------------------------------------------------------------
def _applies(mutant, dtype, metric):
    if mutant == 4:  # products of two binary16 values are exact in f32: fusing them or not is the same arithmetic
        return (dtype, metric) != ("float16", "ip")
    if mutant == 5:  # see test_skipping_clamped_steps_changes_no_bit
        return False
    if mutant == 6:
        return dtype == "float16"
    return True


def _must_differ(mutant, dtype, case):
    """Whether this case's rows leave the mutant no way to hide."""
    dim = rc.dim_of(dtype, case)
    geo = rc.walk_of_row(dtype, dim)
    data_chunks = -(-dim // EPC[dtype])
    if mutant in (1, 2):  # some lane meets two data chunks (m1: inside one span, so a lane has more than one step per span)
        return data_chunks > geo["G"] and (mutant == 2 or geo["CU"] >= 2)
    if mutant == 3:
        # a left-to-right sum of up to three non-zero lanes followed by zeros is the butterfly's (l0 + l1) + (l2 + 0): the first
        # order that can differ has four.  No case has two or three data chunks, so this is "more than one non-zero lane".
        assert data_chunks == 1 or data_chunks >= 4, (dtype, case)
        return data_chunks >= 4
    if mutant == 4:
        return dim >= 8
    return False


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", TYPES)
def test_every_mutant_is_told_apart(dtype, metric):
    told = {m: [] for m in dm.MUTANTS}
    for case in rc.CASES:
        dim, sets = data_sets(dtype, metric, case)
        changed = {}
        for name, X, Q in sets:
            X, Q = X[:200], Q[QUERIES[:6]]  # (every kind of row the edge data has recurs within 10 rows)
            base = dm.distances(dtype, metric, X, Q)
            for m in dm.MUTANTS:
                changed[m] = changed.get(m, 0) + int((dm.distances(dtype, metric, X, Q, mutant=m) != base).sum())
        print("distance model, mutants: %s %s %-24s dim %4d: %s" % (dtype, metric, case, dim, "  ".join(
            "m%d %s" % (m, "-" if not changed[m] else "%d bits" % changed[m]) for m in dm.MUTANTS)))
        for m in dm.MUTANTS:
            if changed[m]:
                told[m].append(case)
            if _applies(m, dtype, metric) and _must_differ(m, dtype, case):
                assert changed[m], (dtype, metric, case, dm.MUTANTS[m])
    for m in dm.MUTANTS:
        if _applies(m, dtype, metric):
            assert told[m], (dtype, metric, dm.MUTANTS[m])
    # Skipping a clamped step instead of running it on zeros can only turn a lane's -0 partial sum into +0 or leave it.  L2
    # sums are never -0 (squares are added to +0), and IP ends in 1 - s, which is 1 for either zero: no reported bit can tell.
    assert not told[5], (dtype, metric, told[5])
