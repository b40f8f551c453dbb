"""The five batched search forms of both Python surfaces -- hip.DeviceIndex's host-buffer methods and the extension's index
methods -- share one argument check and one result packaging each.  Every form must still raise its own ValueError for a wrong
query width, K = 0 and (the exhaustive forms) K = 1025, before it looks at its filter arguments, and return its own stats keys."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, NQ, EF = 64, 8, 3, 16
BAD_FILTER = np.array([-1])  # a negative label: raises on its own, so a K error that wins was checked first
K_POSITIVE = "K must be positive"
K_EXHAUSTIVE = "K of an exhaustive search must be between 1 and 1024"
HOP_KEYS, SCAN_KEYS = {"count", "n_dist", "n_hops"}, {"count", "n_dist"}


@pytest.fixture(scope="module")
def setup():
    import flatnav_amd as flatnav
    from flatnav_amd import hip

    rng = np.random.default_rng(7)
    X, Q = rng.random((N, DIM), dtype=np.float32), rng.random((NQ, DIM), dtype=np.float32)
    index = flatnav.index.create("l2", DIM, N, 8)
    index.add(X, 32)
    dev = hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False)
    return index, dev, Q


def device_forms(dev):
    """name -> (call(queries, K, filter argument, stats), upper bound on K or None, stats keys)."""
    qf = np.zeros(NQ, np.int64)
    return {
        "search": (lambda q, K, f, stats: dev.search(q, K, EF, stats=stats), None, HOP_KEYS),
        "search_filtered": (lambda q, K, f, stats: dev.search_filtered(q, K, EF, f, stats=stats), None, HOP_KEYS),
        "search_exhaustive": (lambda q, K, f, stats: dev.search_exhaustive(q, K, f, stats=stats), 1024, SCAN_KEYS),
        "search_filtered_grouped": (lambda q, K, f, stats: dev.search_filtered_grouped(q, K, EF, [f], qf, stats=stats), None, HOP_KEYS),
        "search_exhaustive_grouped": (lambda q, K, f, stats: dev.search_exhaustive_grouped(q, K, [f], qf, stats=stats), 1024, SCAN_KEYS),
    }


def index_forms(index):
    qf = np.zeros(NQ, np.int64)
    return {
        "search": (lambda q, K, f: index.search(q, K, EF), None),
        "search_filtered": (lambda q, K, f: index.search_filtered(q, K, EF, f), None),
        "search_exhaustive": (lambda q, K, f: index.search_exhaustive(q, K, f), 1024),
        "search_filtered_grouped": (lambda q, K, f: index.search_filtered_grouped(q, K, EF, [f], qf), None),
        "search_exhaustive_grouped": (lambda q, K, f: index.search_exhaustive_grouped(q, K, [f], qf), 1024),
    }


FORMS = ["search", "search_filtered", "search_exhaustive", "search_filtered_grouped", "search_exhaustive_grouped"]


@pytest.mark.parametrize("form", FORMS)
def test_device_index_checks_and_stats(setup, form):
    _, dev, Q = setup
    call, k_max, keys = device_forms(dev)[form]
    everything = np.arange(N)
    with pytest.raises(ValueError, match="^Queries have incorrect dimensions.$"):
        call(Q[:, :DIM - 1], 5, BAD_FILTER, False)
    with pytest.raises(ValueError, match="^Queries have incorrect dimensions.$"):
        call(Q[0], 5, BAD_FILTER, False)
    with pytest.raises(ValueError, match="^%s$" % (K_EXHAUSTIVE if k_max else K_POSITIVE)):
        call(Q, 0, BAD_FILTER, False)
    if k_max:
        with pytest.raises(ValueError, match="^%s$" % K_EXHAUSTIVE):
            call(Q, k_max + 1, BAD_FILTER, False)
    if form != "search":
        with pytest.raises(ValueError, match="non-negative"):
            call(Q, 5, BAD_FILTER, False)
    plain = call(Q, 5, everything, False)
    assert len(plain) == 2
    d, l, stats = call(Q, 5, everything, True)
    assert set(stats) == keys
    assert d.shape == l.shape == (NQ, 5) and d.dtype == np.float32 and l.dtype == np.int32
    assert np.array_equal(d, plain[0]) and np.array_equal(l, plain[1])
    assert stats["count"].dtype == np.int32 and (stats["count"] == 5).all()
    assert all(stats[k].dtype == np.uint64 and stats[k].shape == (NQ,) and (stats[k] > 0).all() for k in keys - {"count"})


@pytest.mark.parametrize("form", FORMS)
def test_extension_index_checks(setup, form):
    index, dev, Q = setup
    call, k_max = index_forms(index)[form]
    with pytest.raises(ValueError, match="^Queries have incorrect dimensions.$"):
        call(Q[:, :DIM - 1], 5, BAD_FILTER)
    with pytest.raises(ValueError, match=r"^%s\.$" % (K_EXHAUSTIVE if k_max else K_POSITIVE)):
        call(Q, 0, BAD_FILTER)
    if k_max:
        with pytest.raises(ValueError, match=r"^%s\.$" % K_EXHAUSTIVE):
            call(Q, k_max + 1, BAD_FILTER)
    if form != "search":
        with pytest.raises(ValueError, match="non-negative"):
            call(Q, 5, BAD_FILTER)
    out = call(Q, 5, np.arange(N))
    assert isinstance(out, tuple) and len(out) == 2
    d, l = out
    assert d.shape == l.shape == (NQ, 5) and d.dtype == np.float32 and l.dtype == np.int32
    want = device_forms(dev)[form][0](Q, 5, np.arange(N), False)  # the two surfaces run the same launch
    assert np.array_equal(d.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(l, want[1])
