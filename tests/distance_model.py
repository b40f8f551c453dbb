"""The lane-by-lane CPU model of the float distance arithmetic (tests/distance_model_harness.cpp, compiled with g++ and loaded
with ctypes), its data sets, and the one constant that says how the float16 inner product's two-element dot rounds (test
infrastructure; not a conftest).

`distances` gives the float32 BITS the kernels must report for every (query, row): the model restates batch_dists
(flatnav_amd/csrc/distance.hpp) and takes the row's geometry from the launch planner through tests/row_classes.py, so no
layout rule is stated twice.  tests/test_distance_model.py checks the model on the CPU (float bar, the emulations of
tests/test_half_rows.py, exact integers, six mutants); tests/test_gpu_distance_bits.py holds every kernel family to it."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import row_classes as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "distance_model_harness.cpp")
FLAGS = ["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"]
METRIC_ORD = {"l2": 0, "ip": 1}  # FNV_METRIC_* (include/flatnav_hip.h)
NQ = 40
RTOL, ATOL = 1e-5, 1e-6  # the float bar

# float16 IP.  DOT_NONE: what the kernels compute, one fused multiply-add per element.  The rest: the candidate semantics of
# v_dot2_f32_f16 (dot2 in the harness), which the float16 inner product rested on until the instruction was read off an MI355X
# (profiles/distance_bits.md, tests/golden/probes/dot2_probe.npz): the form, + 4 if binary16 subnormal inputs are flushed, + 8 if an
# f32 subnormal accumulator or result is.  No candidate was the instruction bit for bit, so the kernels no longer use it.
DOT_NONE = -1
DOT_EXACT, DOT_FMA_01, DOT_FMA_10, DOT_PAIR_THEN_ADD, DOT_FLUSH_IN, DOT_FLUSH_F32 = 0, 1, 2, 3, 4, 8
DOT_FORMS = {DOT_EXACT: "(a) exact sum, one rounding", DOT_FMA_01: "(b) fma(a1,b1,fma(a0,b0,c))", DOT_FMA_10: "(c) fma(a0,b0,fma(a1,b1,c))",
             DOT_PAIR_THEN_ADD: "(d) round(a0*b0+a1*b1) + c"}
DOT_MODES = [form | fin | f32 for form in DOT_FORMS for fin in (0, DOT_FLUSH_IN) for f32 in (0, DOT_FLUSH_F32)]
# THE MODE IN FORCE: the one constant the model's float16 IP uses.
DOT_MODE = DOT_NONE

MUTANTS = {1: "m1 chunk order reversed", 2: "m2 accumulator assignment", 3: "m3 left-to-right lane sum", 4: "m4 unfused multiply-add",
           5: "m5 clamped steps skipped", 6: "m6 binary16 subnormals flushed"}
_lib = None


def mode_name(mode: int) -> str:
    return DOT_FORMS[mode & 3] + (", binary16 subnormal inputs flushed" if mode & DOT_FLUSH_IN else "") + \
        (", f32 subnormals flushed" if mode & DOT_FLUSH_F32 else "")


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="flatnav_distance_model_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libdistance_model_harness.so")
        subprocess.check_call(FLAGS + ["-fPIC", "-shared", SRC, "-o", out])
        L = C.CDLL(out)
        L.dm_cfg.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dm_dot2.argtypes = [C.c_uint16] * 4 + [C.c_uint32, C.c_int]
        L.dm_dot2.restype = C.c_uint32
        L.dm_distances.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_int, C.c_int, C.c_void_p]
        L.hrh_dist_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int]
        L.hrh_dist_f32.restype = C.c_float
        L.hrh_dist_half.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        L.hrh_dist_half.restype = C.c_float
        _lib = L
    return _lib


def dot2(a0, b0, a1, b1, c=0.0, mode=DOT_EXACT) -> int:
    """Bits of one two-element dot of binary16 values onto the f32 accumulator c, under candidate `mode`."""
    h = lambda v: int(np.array(v, np.float16).view(np.uint16))
    return lib().dm_dot2(h(a0), h(b0), h(a1), h(b1), int(np.array(c, np.float32).view(np.uint32)), mode)


def padded(A: np.ndarray, geo: dict) -> np.ndarray:
    """Rows of A zero padded to the staged query's q_chunks chunks of 16 bytes."""
    epc = 16 // A.dtype.itemsize
    out = np.zeros((len(A), geo["q_chunks"] * epc), A.dtype)
    out[:, : A.shape[1]] = A
    return out


def distances(dtype: str, metric: str, X: np.ndarray, Q: np.ndarray, mutant: int = 0, dot_mode=None, capacity: int = rc.N_ROWS) -> np.ndarray:
    """uint32 [len(Q), len(X)]: the bits every kernel family reports for (query, row), rows and queries as the index holds them."""
    np_t = {"float32": np.float32, "float16": np.float16}[dtype]
    assert X.dtype == np_t and Q.dtype == np_t and X.shape[1] == Q.shape[1]
    geo = rc.walk_of_row(dtype, X.shape[1], capacity)
    Xp, Qp = padded(X, geo), padded(Q, geo)
    out = np.empty((len(Q), len(X)), np.uint32)
    rc_ = lib().dm_distances(int(dtype == "float16"), METRIC_ORD[metric], Qp.ctypes.data, len(Qp), Xp.ctypes.data, len(Xp), geo["cfg"],
                             int(geo["full"]), geo["tail_chunks"], geo["nchunks"], geo["q_chunks"], mutant,
                             DOT_MODE if dot_mode is None else dot_mode, out.ctypes.data)
    assert rc_ == 0, ("batch_dists has no branch for this geometry", dtype, X.shape[1], geo)
    return out


def dist64(X: np.ndarray, Q: np.ndarray, metric: str) -> np.ndarray:
    """[nq][n] float64 distances of the values the index holds, every difference taken before it is squared (the expanded form
    loses everything on a row that copies its query)."""
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    if metric == "ip":
        return 1.0 - Q64 @ X64.T
    return np.stack([((X64 - q) ** 2).sum(1) for q in Q64])


def within_float_bar(bits: np.ndarray, D: np.ndarray):
    """(all inside DESIGN section 8's float bar, worst |error| / tolerance)."""
    err = np.abs(bits.view(np.float32).astype(np.float64) - D)
    tol = ATOL + RTOL * np.abs(D)
    return bool((err <= tol).all()), float((err / tol).max())


# ---- the finite edge data ----------------------------------------------------------------------------------------------------------
def _vals(rng, shape, p, e):
    """+- m * 2^(e - p + 1) with a random p-bit mantissa m whose top bit is set: magnitudes in [2^e, 2^(e+1)), exact in float64."""
    m = (1 << (p - 1)) + rng.integers(0, 1 << (p - 1), shape)
    return rng.choice([-1.0, 1.0], shape) * np.ldexp(m.astype(np.float64), np.broadcast_to(np.asarray(e) - (p - 1), shape))


def _f16(A):
    with np.errstate(over="ignore"):
        h = A.astype(np.float16)
    return np.where(np.isfinite(h), h, np.float16(0))


def copies_of(i: int) -> int:
    """The query that row i copies (i % 10 == 1) or negates (i % 10 == 2)."""
    return (i // 10 * 4) % NQ


def edge_case(dtype: str, metric: str, dim: int, lossless: bool = False, n: int = rc.N_ROWS):
    """(rows, queries) at the value edges, finite everywhere.  Elements are +- m * 2^e with a random 24-bit (float32) or 11-bit
    (float16) mantissa.  `lossless`: a float32 index whose rows binary16 holds exactly (the half-width mirror's precondition);
    its queries stay float32 but for every fourth, which the copy rows copy.

    L2: exponents uniform over [-20, 20] (float32) or the whole finite binary16 range, subnormals included.  Nothing needs
    scaling: every term is a square, so float32 sums keep a relative error of a few 2^-24 per addition, and the largest
    distance is far below 2^128.
    IP: DESIGN section 8's bar is absolute near d = 0 (1e-6), and a float32 sum errs by (roundings) * 2^-24 * sum |x_i q_i|, so
    the data keeps sum |x_i q_i| below 1/4 for every pair: position i has a budget exponent b_i, uniform over the query type's
    range; |q_i| < 2^b_i and |x_i| < 2^(-b_i - L) with 2^L >= 16 dim.  Queries cover their whole range, rows meet large query
    elements with small ones and the reverse.

    Rows by number (where dim allows):  i % 10 == 1 copies query copies_of(i) and i % 10 == 2 negates it (L2: the copy is at +0;
    IP: the query's signs and mantissas at the row's exponents, so all products have one sign);  3 is all +0, 13 all -0;
    IP, i % 5 == 4: the products of neighbouring elements cancel for query (i // 5) % 40 to the last bits of the row's precision;
    float32 IP, i % 5 == 0: float32 subnormals at positions 3, 11, 19 .. against query elements of 2^100 .. 2^111 (all other rows
    are zero there);  binary16 rows, i % 10 == 6: nothing but binary16 subnormals, against query elements in [1, 2) (L2) or
    [1024, 2048) (IP) at positions 3, 11, ..;  binary16 rows, row 0: +-65504, 2^-14, 2^-24, -2^-15 and -0."""
    rng = np.random.default_rng(dim * 16 + 4 * int(lossless) + 2 * (dtype == "float16") + (metric == "ip") + 1000003)
    half_q, half_x = dtype == "float16", dtype == "float16" or lossless
    pq, px = (11 if half_q else 24), (11 if half_x else 24)
    S = np.arange(3, dim, 8)
    rows = np.arange(n)
    if metric == "l2":
        Q = _vals(rng, (NQ, dim), pq, rng.integers(-24, 16, (NQ, dim)) if half_q else rng.integers(-20, 21, (NQ, dim)))
        X = _vals(rng, (n, dim), px, rng.integers(-24, 16, (n, dim)) if half_x else rng.integers(-20, 21, (n, dim)))
        if lossless:
            Q[::4] = _vals(rng, Q[::4].shape, 11, rng.integers(-24, 16, Q[::4].shape))
        if half_x:
            Q[:, S] = _vals(rng, (NQ, len(S)), pq, 0)
            sub = rows % 10 == 6
            X[sub] = rng.choice([-1.0, 1.0], (sub.sum(), dim)) * rng.integers(1, 1024, (sub.sum(), dim)) * 2.0 ** -24 * (rng.random((sub.sum(), dim)) < 0.5)
            if dim >= 8:
                X[0, [0, 1]], Q[0, [0, 1]] = [65504.0, -65504.0], [-65504.0, 65504.0]
                X[0, 4:8] = [2.0 ** -14, 2.0 ** -24, -(2.0 ** -15), -0.0]
        scale = None
    else:
        L = int(np.ceil(np.log2(max(dim, 1)))) + 4
        b = rng.integers(-23, 17, dim) if half_x else rng.integers(-19, 22, dim)
        if half_x:
            b[S] = 11
            if dim >= 8:
                b[4:8] = np.minimum(b[4:8], 14 - L)
                b[2] = 16
        Q = _vals(rng, (NQ, dim), pq, b - 1 - rng.integers(0, 2, (NQ, dim)))
        if lossless:
            Q[::4] = _vals(rng, Q[::4].shape, 11, b - 1 - rng.integers(0, 2, Q[::4].shape))
        X = _vals(rng, (n, dim), px, np.minimum(-b - L - 1 - rng.integers(0, 2, (n, dim)), 15 if half_x else 127))
        scale = np.ldexp(1.0, -2 * b - L)  # a query element at the row's exponent
        if half_x:
            Q[:, S] = _vals(rng, (NQ, len(S)), pq, 10)
            if dim >= 8:
                Q[:, 0], Q[:, 1], Q[0, 2] = 0.0, -0.0, 65504.0
                X[:, 2] = np.where(rows % 2 == 0, 0.0, -0.0)
        else:
            Q[:, S] = _vals(rng, (NQ, len(S)), 24, rng.integers(100, 111, (NQ, len(S))))
            X[:, S] = 0.0
    if lossless:
        Q[::4] = _f16(Q[::4]).astype(np.float64)
    for i in rows[rows % 10 == 1]:
        X[i] = Q[copies_of(i)] * (1.0 if scale is None else scale)
    for i in rows[rows % 10 == 2]:
        X[i] = -Q[copies_of(i)] * (1.0 if scale is None else scale)
    X[3], X[13] = 0.0, -0.0
    if metric == "ip":
        for i in rows[rows % 5 == 4]:
            q = Q[(i // 5) % NQ]
            even, odd = np.arange(0, dim - 1, 2), np.arange(1, dim, 2)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                t = -(X[i, even] * q[even]) / q[odd]
            X[i, odd] = np.where(np.isfinite(t) & (np.abs(t) < (6e4 if half_x else 1e30)), t, 0.0)
        if half_x:
            sub = rows[rows % 10 == 6]
            X[sub] = 0.0
            for i in sub:
                at = S[(i // 10 + np.arange(2)) % len(S)] if len(S) else S
                X[i, at] = rng.choice([-1.0, 1.0], len(at)) * rng.integers(1, 1024, len(at)) * 2.0 ** -24
            if dim >= 8:
                X[0, [0, 1]] = [65504.0, -65504.0]
                X[0, 4:8] = [2.0 ** -14, 2.0 ** -24, -(2.0 ** -15), -0.0]
        else:
            X[:, S] = 0.0
            sub = rows[rows % 5 == 0]
            X[np.ix_(sub, S)] = rng.choice([-1.0, 1.0], (len(sub), len(S))) * rng.integers(1, 1 << 23, (len(sub), len(S))) * 2.0 ** -149
    if dtype == "float16":
        return _f16(X), _f16(Q)
    X = _f16(X).astype(np.float32) if lossless else X.astype(np.float32)
    return X, Q.astype(np.float32)


OVERFLOW_ROWS = (7, 107, 207, 307)


def overflow_case(X: np.ndarray):
    """The finite float32 L2 rows with four rows that hold one element of 3e19: their squared difference exceeds float32."""
    X = X.copy()
    for k, i in enumerate(OVERFLOW_ROWS):
        X[i, (k * 5) % X.shape[1]] = np.float32(3e19)
    return X


def assert_finite(D: np.ndarray, what):
    assert np.isfinite(D).all() and np.abs(D).max() < 2.0 ** 120, what


# ---- the rows that read the two-element dot off the hardware -----------------------------------------------------------------------
def dot2_case(n: int = rc.N_ROWS):
    """(rows, queries) of a float16 IP index of dim 8 whose distances are 1 - (sum over elements 0, 1, 4, 5): elements 2, 3, 6 and
    7 are zero, so lane 0's second accumulator (under the two-element dot) and the lanes 1 .. 7 add +0.  With the dot the
    distance was 1 - dot(x[4:6], q[4:6], dot(x[0:2], q[0:2], +0)), and where the dot lies in [0.5, 2] the subtraction is exact
    and 1 - d gives the dot back without loss.  Random 11-bit mantissas over ten binades, so most exact sums need more than 24
    bits; rows 0 mod 2 leave elements 4 and 5 zero; rows 1 mod 5 hold a binary16 subnormal in element 1 and queries 30 .. 39 a
    value of 2^13 .. 2^15 there, so the subnormal's product decides the result (rows 6 mod 10: it is the only non-zero
    product).  The last ten rows and queries 28, 29 are integer valued with |v| <= 2048 and sums just below 2^24: the edge of
    DESIGN section 8's integer contract."""
    rng = np.random.default_rng(20251)
    X, Q = np.zeros((n, 8)), np.zeros((NQ, 8))
    X[:, :2] = _vals(rng, (n, 2), 11, rng.integers(-6, 4, (n, 2)))
    Q[:, :2] = _vals(rng, (NQ, 2), 11, rng.integers(-3, 7, (NQ, 2)))
    X[1::2, 4:6] = _vals(rng, (n // 2, 2), 11, rng.integers(-6, 4, (n // 2, 2)))
    Q[:, 4:6] = _vals(rng, (NQ, 2), 11, rng.integers(-3, 7, (NQ, 2)))
    Q[::3, 4:6] = 0.0
    sub = np.arange(1, n, 5)
    X[sub, 1] = rng.choice([-1.0, 1.0], len(sub)) * rng.integers(1, 1024, len(sub)) * 2.0 ** -24
    X[6::10, 0] = 0.0
    X[6::10, 4:6] = 0.0
    Q[30:, 1] = _vals(rng, (NQ - 30,), 11, rng.integers(13, 15, NQ - 30))
    X[n - 10:], Q[28:30] = 0.0, 0.0
    X[n - 10:, [0, 1, 4, 5]] = rng.integers(2038, 2049, (10, 4))
    Q[28:30, [0, 1, 4, 5]] = [[2048, 2047, 2046, 2045], [2047, 2048, 2041, 2047]]
    assert (Q[28:30] @ X[n - 10:].T).max() < 2 ** 24 - 1 and (Q[28:30] @ X[n - 10:].T).max() > 2 ** 24 - 2 ** 18
    return _f16(X), _f16(Q)


def dot2_readable(X, Q):
    """bool [nq][n]: pairs of dot2_case whose dot lies in [0.5, 2] under every candidate that keeps binary16 subnormals, so
    1 - d reads it back exactly."""
    ok = np.ones((len(Q), len(X)), bool)
    for mode in DOT_FORMS:
        s = np.float32(1.0) - distances("float16", "ip", X, Q, dot_mode=mode).view(np.float32)
        ok &= (s >= 0.5) & (s <= 2.0)
    return ok
