"""The CPU model of the batched wiring rule (tests/batched_wiring_ref.cpp) must be right before it judges a kernel.

1. With one node per call the batched rule IS the reference's sequential insertion (every target has one requester), so
   chaining the model over N insertions must reproduce the oracle's single-threaded build byte for byte.
2. The inputs of tests/test_gpu_batched_wiring.py must reach the code paths they were chosen for: the model's path counters
   are asserted here, on the CPU, for every GPU case."""
import numpy as np
import pytest

import batched_wiring_cases as cases
import batched_wiring_ref as bwr


@pytest.mark.parametrize("hi", [4, 60], ids=["ties_everywhere", "few_ties"])
@pytest.mark.parametrize("M", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("metric", ["l2", "angular"])
@pytest.mark.parametrize("dt", ["float32", "uint8", "int8"])
def test_one_node_batches_reproduce_the_oracle_build(oracle_mod, dt, metric, M, hi):
    rng = np.random.default_rng(5)
    N, dim, efc = 600, 16, 24
    X = bwr.integer_data(rng, N, dim, dt, hi)
    o = oracle_mod.OracleIndex.create(metric, dim, N, M, dt)
    o.add(X, efc)
    want = np.asarray(o.blob())[: N * o.node_size].reshape(N, o.node_size)
    b = bwr.Batch(oracle_mod, metric, dt, dim, M, X, 1, efc)
    short = 0
    for _ in range(1, N):
        _, ctr, _ = b.insert(1)
        short += ctr["short_beam_nodes"]
    assert short >= max(M // 2, 1) - 1  # the first insertions see fewer nodes than they may keep
    bad = np.flatnonzero((want != b.nodes).any(axis=1))
    assert bad.size == 0, "first differing node %d of %d differing" % (bad[0], bad.size)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_gpu_case_inputs_reach_their_paths(oracle_mod, case):
    b, steps, total = cases.model(case, oracle_mod)
    cases.check_expectations(case, total)
    n = case.first + sum(case.counts)
    L = b.links(n)
    assert (L < n).all()
    assert (L[case.first:] < case.first + np.cumsum(case.counts)[-1]).all()
    own = np.arange(n, dtype=np.uint32)[:, None]
    srt = np.sort(np.where(L != own, L, np.uint32(0xFFFFFFFF)), axis=1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != 0xFFFFFFFF)).any()  # no neighbour twice in a row


def test_every_path_counter_is_reached_by_some_case(oracle_mod):
    seen = {k: 0 for k in bwr.COUNTERS}
    for case in cases.CASES:
        total = cases.model(case, oracle_mod)[2]
        for k in seen:
            seen[k] = max(seen[k], total[k])
    assert all(v > 0 for v in seen.values()), seen
