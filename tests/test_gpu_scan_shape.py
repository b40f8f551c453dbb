"""The exhaustive scan is launched in the shape the planner's CPU test pins (csrc/launch_plan.hpp scan_shape, swept by
tests/test_launch_plan.py): for plain, single-filter and grouped calls, what fnv_last_launch_geometry reports of the launch --
grid, LDS bytes and, grouped, queries per tile, id-queue entries and row segments -- equals what tests/launch_plan_harness.cpp
computes for the same (element type, dim, capacity, CU count, K, nq, "scan_segment_rows").

Two device-built 3000-row indexes, 64-d float32 and 128-d uint8.  (nq, K) = (1, 1), (33, 10), (200, 1024): one query, one more
than the widest tile of 32, and result lists so long that a block's LDS budget holds two queries of 64-d rows."""
import ctypes
import itertools

import numpy as np
import pytest

import test_launch_plan as tlp
from flatnav_amd import datasets as ds
from flatnav_amd import hip

pytestmark = pytest.mark.gpu
N, M, EFC, FILTERS = 3000, 16, 32, 3
DTYPES = {"float32": (tlp.F32, 64), "uint8": (tlp.U8, 128)}
_BUILT = {}


def _index(dtype):
    if dtype not in _BUILT:
        import flatnav_amd

        dim = DTYPES[dtype][1]
        X, Q = ds.sift_like(N, 200, dim=dim)
        index = flatnav_amd.index.create("l2", dim, N, M, getattr(flatnav_amd.data_type.DataType, dtype))
        index.set_num_threads(4)
        index.add(X.astype(dtype), EFC, labels=list(range(N)), device=True)
        _BUILT[dtype] = (index, hip.DeviceIndex(ctypes.c_void_p(index.device_handle()), owned=False), Q.astype(dtype))
    return _BUILT[dtype][1:]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_scan_launches_in_the_planned_shape(dtype):
    import torch

    dev, Q = _index(dtype)
    code, dim = DTYPES[dtype]
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(5)
    filters = [rng.choice(N, N // 2, replace=False), np.arange(100, 400), np.array([7])]
    seen_tiles = set()
    try:
        for kind, (nq, K), seg in itertools.product(("plain", "single", "grouped"), ((1, 1), (33, 10), (200, 1024)), (0, 256)):
            dev.set_option("scan_segment_rows", seg)
            if kind == "grouped":
                dev.search_exhaustive_grouped(Q[:nq], K, filters, rng.integers(-1, FILTERS, nq).astype(np.int32))
            else:
                dev.search_exhaustive(Q[:nq], K, allowed=filters[0] if kind == "single" else None)
            geom = dev.launch_geometry()
            rows = FILTERS + 2 if kind == "grouped" else 0  # (scan_select.hpp: a grouped launch keeps n_filters + 2 node bitmaps)
            want = tlp.scan_shapes([[code, dim, N, num_cus, seg, 0, 0, nq, K, N, rows]])
            tile, tiles, segments, lds = (int(want[c][0]) for c in ("tile", "tiles", "segments", "lds"))
            what = (dtype, kind, nq, K, seg, geom)
            assert geom["kernel"] == "exhaustive_scan", what
            assert geom["grid_blocks"] == tiles * segments and geom["lds_bytes"] == lds, (what, tile, tiles, segments, lds)
            if kind == "grouped":
                assert (geom["tile_queries"], geom["queue_ids"], geom["segments"]) == (tile, tlp.SCAN_QUEUE_IDS, segments), (what, tile, segments)
            else:
                assert "tile_queries" not in geom, what
            seen_tiles.add(tile)
    finally:
        dev.set_option("scan_segment_rows", 0)
    assert {1, 2, 32} <= seen_tiles, seen_tiles  # (K = 1024: two queries per tile on both indexes; nq = 33: the widest tile)
