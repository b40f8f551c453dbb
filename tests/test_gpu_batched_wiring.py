"""The batched device builder (fnv_index_insert_batch with batches of many nodes: wire_select_kernel + wire_connect_kernel,
flatnav_amd/csrc/wire.hpp) against the CPU model of its rule (tests/batched_wiring_ref.cpp), byte for byte, through the C ABI.

Per case: a seed graph of `first` nodes from the oracle goes into a device index allocated at full capacity, one
insert_batch wires `count` more, and EVERY link row of EVERY node -- targets and new nodes -- must equal the model's, which is
fed the oracle's beams for the same batch.  The evaluation count must equal the oracle's, and a search over the result must
equal the oracle's search over the model's graph bit for bit.  The cases and the code paths each one reaches (hub targets
consumed in several rounds, runs that cross a 64-request block, shared free slots, prunes over more than 64 candidates,
equal keys, beams shorter than M / 2, every row width and row configuration) are listed in tests/batched_wiring_cases.py;
tests/test_batched_wiring_model.py proves on the CPU that they reach them.

Integer-valued data only: on real-valued floats the predicate d(k, c) < d(u, c) can flip on the last bit of a sum.  Float
distance arithmetic is pinned by the search tests, and nothing in the wiring logic depends on the element type beyond the
distance."""
import os

import numpy as np
import pytest

import batched_wiring_cases as cases
import batched_wiring_ref as bwr
from flatnav_amd import hip

pytestmark = pytest.mark.gpu


def _load(b, M):
    """A device index at full capacity holding every record of b's initial table, the seed graph live."""
    blob, node_size, data_size = b.device_blob()
    n = len(b.initial)
    dev = hip.DeviceIndex.alloc(M, n, b.dtype, b.metric, b.dim)
    dev.write_nodes(0, blob, node_size, data_size)
    dev.set_live_nodes(b.first)
    return dev


def _compare_rows(got, want, first, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        v = int(bad[0])
        raise AssertionError("%s: %d of %d rows differ (%d of them targets); first: node %d (%s)\n  device %s\n  model  %s" % (
            what, bad.size, len(want), int((bad < first).sum()), v, "target" if v < first else "new node", got[v].tolist(),
            want[v].tolist()))


def _run(b, steps, counts, efc, what):
    """The device through the same batches as the model went through; compared after every call."""
    dev = _load(b, b.M)
    cur = b.first
    for step, (count, (want, _, want_evals)) in enumerate(zip(counts, steps)):
        evals = dev.insert_batch(cur, count, efc)
        got = dev.read_links(0, cur + count)
        _compare_rows(got, want, cur, "%s, batch %d (%d nodes onto %d)" % (what, step, count, cur))
        assert evals == want_evals, "%s, batch %d: %d distance evaluations, the oracle's beam searches made %d" % (
            what, step, evals, want_evals)
        cur += count
    # the vectors and links the wiring left behind are the ones searched
    rng = np.random.default_rng(11)
    Q = b.X[rng.integers(0, len(b.X), 32)] + (rng.random((32, b.dim)) < 0.2)
    wd, wl = b.search(Q, 10, 64)
    gd, gl = dev.search(Q.astype(np.float16 if b.dtype == "float16" else b.X.dtype), 10, 64)
    assert np.array_equal(gl, wl) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what + ": search differs"
    return dev


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_batched_insertion_equals_the_cpu_model(oracle_mod, case):
    b, steps, total = cases.model(case, oracle_mod)
    cases.check_expectations(case, total)
    _run(b, steps, case.counts, case.efc, repr(case))


def test_rows_wider_than_a_wave_are_refused_and_nothing_changes(oracle_mod):
    rng = np.random.default_rng(65)
    M, first, count, dim = 65, 100, 20, 16
    b = bwr.Batch(oracle_mod, "l2", "float32", dim, M, bwr.integer_data(rng, first + count, dim, "float32", 60), first, 40)
    dev = _load(b, M)
    before = dev.read_links(0, first + count)
    assert np.array_equal(before, b.links(first + count))
    with pytest.raises(ValueError, match="device-side wiring supports max_edges_per_node <= 64"):
        dev.insert_batch(first, count, 40)
    assert np.array_equal(dev.read_links(0, first + count), before)
    # dev.n_nodes is the Python object's own copy; a second wrapper of the same handle asks the library for the live count
    assert hip.DeviceIndex(dev._h, owned=False).n_nodes == first


def test_batched_insertion_equals_the_cpu_model_on_random_shapes(oracle_mod):
    # Randomly drawn element type, metric, row width, link-row width, ef_construction, tie density, live graph and batch
    # size (FNV_FUZZ_TRIALS / FNV_FUZZ_SEED deepen the sweep).
    rng = np.random.default_rng(int(os.environ.get("FNV_FUZZ_SEED", "177")))
    for trial in range(int(os.environ.get("FNV_FUZZ_TRIALS", "12"))):
        dt = ["float32", "uint8", "int8", "float16"][trial % 4]
        metric = ["l2", "angular"][int(rng.integers(0, 2))]
        dim = int(rng.choice([4, 16, 33, 64, 100, 128, 200]))
        M = int(rng.choice([1, 2, 3, 4, 8, 16, 32, 48, 64]))
        efc = int(rng.choice([5, 20, 40, 100]))
        hi = int(rng.choice([2, 4, 16, 60]))  # sums <= 200 * 59^2 < 2^24
        first = int(rng.choice([1, 2, 5, 40, 300, 600]))
        count = int(rng.integers(1, 1500 - first + 1)) if trial % 3 else int(rng.choice([1, 63, 64, 65, 256]))
        keep = max(M // 2, 1)
        if 16 < min(first, efc) < keep:  # the model cannot tell the pop order of such a beam (batched_wiring_ref.cpp)
            first, efc = max(first, keep), max(efc, keep)
        what = "trial %d: %s %s d=%d M=%d efc=%d values 0..%d first=%d count=%d" % (trial, dt, metric, dim, M, efc, hi - 1, first, count)
        try:
            b = bwr.Batch(oracle_mod, metric, dt, dim, M, bwr.integer_data(rng, first + count, dim, dt, hi), first, efc)
            _run(b, [b.insert(count)], (count,), efc, what)
        except Exception as e:  # the seed build, the model and the device calls name no shape of their own
            if what in str(e):
                raise
            raise AssertionError("%s: %s: %s" % (what, type(e).__name__, e)) from e
