"""Range search (option "scan_radius") without a GPU: the key bound of flatnav_amd/csrc/scan_select.hpp against numpy
(tests/range_bound_harness.cpp, compiled with g++), the option's values, the header's text and the Python surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_bound_against_numpy(tmp_path):
    out = str(tmp_path / "librange_bound_harness.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", os.path.join(ROOT, "tests", "range_bound_harness.cpp"), "-o", out])
    L = C.CDLL(out)
    L.rbh_in_range.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.rbh_radius_valid.argtypes = [C.c_int64]
    # distances: negative (inner product), both zeros, attained values and their neighbours, the extremes, +-inf, two NaNs
    d = np.array([-np.inf, -3.5, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.nextafter(np.float32(1), np.float32(2)), 7.0, 3.4e38, np.inf,
                  np.nan, np.nan], np.float32)
    dbits = d.view(np.uint32).copy()
    dbits[-1] = 0xFFC00001  # (a NaN with its sign and a payload)
    # radii: below every distance but -inf, exactly attained ones, between two, negative, +-0, +inf
    r = np.array([-np.inf, -4.0, -3.5, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 7.0, 1e30, np.inf], np.float32)
    with np.errstate(invalid="ignore"):
        want = d[None, :] <= r[:, None]  # (a NaN compares false: within no radius)
    for node in (0, 5, 0xFFFFFFFE):  # the node id never decides
        got, nodes = np.zeros((len(r), len(d)), np.uint8), np.full(len(d), node, np.uint32)
        L.rbh_in_range(r.ctypes.data, len(r), dbits.ctypes.data, nodes.ctypes.data, len(d), got.ctypes.data)
        assert np.array_equal(got.astype(bool), want), node
    assert not want[:, -2:].any() and want[-1, :-2].all() and want[0].sum() == 1
    ok = lambda v: bool(L.rbh_radius_valid(v))  # noqa: E731  (off; 0, +-inf, -1.0 / the NaNs, beyond 32 bits)
    assert ok(-1) and ok(-(2 ** 40)) and ok(0) and ok(0x7F800000) and ok(0xFF800000) and ok(0xBF800000)
    assert not ok(0x7FC00000) and not ok(0xFFC00000) and not ok(0x7F800001) and not ok(2 ** 32) and not ok(2 ** 32 + 5)


def test_header_and_python_surface():
    header = open(os.path.join(ROOT, "include", "flatnav_hip.h")).read()
    knobs = header[header.index("Tuning / test knobs"):]
    assert '"scan_radius"' in knobs[:knobs.index("*/")]
    section = header[header.index("Range search (option"):header.index("int fnv_search_batch_exhaustive(")]
    assert header.index("Matrix engine (option") < header.index("Range search (option") and '"scan_radius"' in section and "out_ndist" in section
    import flatnav_amd

    classes = [c for c in vars(flatnav_amd._core.index).values() if isinstance(c, type) and hasattr(c, "search_exhaustive")]
    assert len(classes) == 8 and all(callable(getattr(c, "set_exhaustive_radius", None)) for c in classes)
    index = flatnav_amd.index.create("l2", 8, 10, 4)  # no device mirror exists yet, so nothing is uploaded
    for radius in ((), (None,), (2.5,), (float("inf"),)):
        index.set_exhaustive_radius(*radius)
    with pytest.raises(ValueError):
        index.set_exhaustive_radius(float("nan"))
