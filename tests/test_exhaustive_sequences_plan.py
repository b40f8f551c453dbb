"""The call sequences of tests/exhaustive_sequences.py replayed through the launch planner alone, on the CPU: the committed seed
and step count (40 steps per index) reach the code tests/test_gpu_exhaustive_sequences.py is meant to run.  These are conditions on the
generator, not measurements: a change of seed, weights or step count that loses one of them fails here, in seconds, and not as
a GPU test that quietly stopped covering a kernel."""
import collections

import numpy as np
import pytest

import exhaustive_sequences as seq
from test_gpu_exhaustive import _dist64

REACHABLE = {"uint8": (3, 4), "int8": (3, 4), "float16": (3, 5, 7), "float32": (3, 6, 8)}


@pytest.fixture(scope="module")
def replayed():
    """{element type: [per index: [(step, plan, padded, truncated, zero_ties)]]}; padded: a query has fewer candidates than K;
    truncated: a range step where a query has more in-range candidates than K; zero_ties: an l2 call that holds the zero query,
    with more all-zero candidate rows per row segment than K (tests/exhaustive_sequences.py: a bound that equals the K-th distance)."""
    out = collections.defaultdict(list)
    for ix in seq.indexes():
        X, Q, labels = seq.data(ix)
        D, rows, zero = _dist64(X, Q, ix.metric), [], ~X.any(1)
        for step in seq.sequence(ix):
            cands, p = seq.row_candidates(step, labels), seq.plan(ix, step)
            _, _, count, total = seq.expected(step, D, labels, cands)
            # (p.segments: a matrix engine's; 0 where the vector scan keeps the call)
            zero_ties = ix.metric == "l2" and step.nq > seq.ZERO_QUERY and p.segments != 0 and int(zero[cands[seq.ZERO_QUERY]].sum()) // p.segments > step.K
            rows.append((step, p, min(len(c) for c in cands) < step.K, step.radius is not None and bool((total > count.astype(np.uint64)).any()), zero_ties))
        out[ix.dtype].append(rows)
    return out


def test_the_generator_draws_what_it_says():
    assert seq.STEPS == 40 and len(seq.indexes()) == len(set(seq.indexes())) == 20
    for ix in seq.indexes():
        assert 1000 <= ix.n <= 2500 and ix.n % 64 not in (0, 1)
        steps = seq.sequence(ix)
        assert len(steps) == seq.STEPS and steps[0].radius is None
        for s, again in zip(steps, seq.sequence.__wrapped__(ix)):  # (drawn once more: the same steps)
            assert all(np.array_equal(a, b) for a, b in zip(s[:4] + s[5:] + tuple(s.filters or ()), again[:4] + again[5:] + tuple(again.filters or ())))
        for s in steps:
            assert 1 <= s.nq <= seq.NQ and 1 <= s.K <= seq.MAX_K and s.seg in seq.SEG_SET
            if s.kind == "grouped":
                assert 1 <= len(s.filters) <= 6 and len(s.qf) == s.nq and s.qf.min() >= -1 and len(set(range(len(s.filters))) - set(s.qf.tolist())) >= 1
    assert {s.radius_kind for ix in seq.indexes() for s in seq.sequence(ix)} == set(seq.RADII) | {None}


@pytest.mark.parametrize("dtype", list(REACHABLE))
def test_the_sequences_reach_the_code_they_are_meant_to_reach(replayed, dtype):
    flat = [row for rows in replayed[dtype] for row in rows]
    steps = [(s, p) for s, p, _, _, _ in flat]
    by_mode = collections.Counter(p.kernel_mode for _, p in steps)
    print(dtype, "steps by kernel mode", dict(by_mode))
    assert set(by_mode) == set(REACHABLE[dtype]) and min(by_mode.values()) >= 5, by_mode
    for mode in set(REACHABLE[dtype]) & {3, 4, 5, 6}:
        assert sum(p.kernel_mode == mode and s.radius is not None and not p.refused for s, p in steps) >= 5, (mode, "with a radius")
        assert sum(p.kernel_mode == mode and s.kind == "grouped" and not p.refused for s, p in steps) >= 5, (mode, "grouped")
    if dtype in ("float16", "float32"):
        other = lambda s: s.radius is not None or s.kind == "grouped"  # noqa: E731
        pairs = [(a, b) for rows in replayed[dtype] for a, b in zip(rows, rows[1:])]
        assert sum(a[1].waves != 0 and other(b[0]) for a, b in pairs) >= 3 and sum(other(a[0]) and b[1].waves != 0 for a, b in pairs) >= 3
        sizes = {len(s.filters[0]) for s, p in steps if p.waves}
        assert sizes >= {0, 1, 31, 32, 33}, sizes
        for s, p in steps:  # the block form is an ungrouped single-filter call without a radius, 64 threads a wavefront
            assert not p.waves or (s.kind == "one" and s.radius is None and s.nq > 32 and 2 <= p.waves <= 4)
    if dtype == "float16":  # (float32's margin has a constant term: its bound never equals an integer distance)
        assert sum(bool(p.waves) and ties for _, p, _, _, ties in flat) >= 1 and sum(p.kernel_mode == 5 and s.radius is None and ties for s, p, _, _, ties in flat) >= 3
    assert sum(padded for _, _, padded, _, _ in flat) >= 5 and sum(truncated for _, _, _, truncated, _ in flat) >= 5
    # a refused call (the vector scan's LDS beyond kScanMaxLds; with a radius, the counter's four bytes on a full LDS) stays in
    # the sequence and must raise; at these row lengths (a query and 1024 keys: 11 KB of 160) the planner refuses none
    assert sum(p.refused for _, p in steps) * 4 <= len(flat)
