"""ctypes binding of the C ABI in include/flatnav_hip.h (libflatnav_hip.so, gfx950).

This is the only way Python code reaches the device search path.  There is NO CPU fallback: if the
shared library is missing or no MI355X is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLATNAV_HIP_LIB") or os.path.join(HERE, "libflatnav_hip.so")

FNV_OK, FNV_ERR_INVALID, FNV_ERR_RUNTIME, FNV_ERR_NO_DEVICE, FNV_ERR_CAPACITY = 0, 1, 2, 3, 4
DTYPE_ORD = {"float32": 9, "uint8": 0, "int8": 4, "float16": 8}
ORD_DTYPE = {v: k for k, v in DTYPE_ORD.items()}
METRIC_ORD = {"l2": 0, "angular": 1, "ip": 1}

# every symbol include/flatnav_hip.h declares (tests check the library exports exactly these)
C_ABI_SYMBOLS = [
    "fnv_last_error", "fnv_version", "fnv_device_count", "fnv_index_upload", "fnv_index_alloc",
    "fnv_index_device_buffers", "fnv_index_info", "fnv_index_free", "fnv_set_option", "fnv_search_batch",
    "fnv_search_batch_device", "fnv_search_status", "fnv_last_kernel_ms", "fnv_last_launch_geometry",
    "fnv_index_set_live_nodes", "fnv_index_write_nodes", "fnv_index_write_links", "fnv_index_insert_batch",
    "fnv_index_read_links", "fnv_last_replayed_queries", "fnv_replicate", "fnv_replica_refresh",
    "fnv_search_batch_multi", "fnv_index_view", "fnv_tune", "fnv_last_launch_info", "fnv_gather_ceiling",
    "fnv_index_adopt", "fnv_lane_info", "fnv_last_handover_stats", "fnv_row_layout",
    "fnv_search_batch_filtered", "fnv_search_batch_filtered_device", "fnv_index_build_half_rows", "fnv_index_half_rows",
    "fnv_search_batch_exhaustive", "fnv_search_batch_exhaustive_device",
    "fnv_search_batch_filtered_grouped", "fnv_search_batch_filtered_grouped_device",
    "fnv_search_batch_exhaustive_grouped", "fnv_search_batch_exhaustive_grouped_device",
]

_lib = None


class DeviceUnavailable(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libflatnav_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DeviceUnavailable(
            "flatnav_amd: %s is missing -- build it with `python -m flatnav_amd.build` "
            "(there is no CPU fallback for the search path)" % LIB_PATH)
    from ._runtime import preload_hip_runtime

    preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.fnv_last_error.restype = C.c_char_p
    L.fnv_version.restype = C.c_char_p
    L.fnv_device_count.argtypes = [C.POINTER(C.c_int)]
    L.fnv_index_upload.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int,
                                   C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    L.fnv_index_alloc.argtypes = [C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_int,
                                  C.POINTER(C.c_void_p)]
    L.fnv_index_device_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.fnv_index_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "fnv_row_layout"):  # (round 6; older builds under the A/B tools lack it)
        L.fnv_row_layout.argtypes = [C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.fnv_index_free.argtypes = [C.c_void_p]
    L.fnv_index_set_live_nodes.argtypes = [C.c_void_p, C.c_uint64]
    L.fnv_index_write_nodes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]
    L.fnv_index_write_links.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.fnv_index_insert_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.fnv_index_read_links.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.fnv_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.fnv_search_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    L.fnv_search_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int] + [
        C.c_void_p] * 6
    if hasattr(L, "fnv_search_batch_filtered"):  # (older builds under the A/B tools lack the filtered entry points)
        L.fnv_search_batch_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_uint64] + [C.c_void_p] * 5
        L.fnv_search_batch_filtered_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                                       C.c_void_p, C.c_uint64] + [C.c_void_p] * 6
    if hasattr(L, "fnv_search_batch_exhaustive"):  # (older builds under the A/B tools lack the exhaustive search)
        L.fnv_search_batch_exhaustive.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                                  C.c_uint64] + [C.c_void_p] * 4
        L.fnv_search_batch_exhaustive_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                                         C.c_uint64] + [C.c_void_p] * 5
    if hasattr(L, "fnv_search_batch_filtered_grouped"):  # (older builds under the A/B tools lack the grouped filters)
        table = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]  # filters, n_filters, stride, n_bits, query_filter
        L.fnv_search_batch_filtered_grouped.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int] + table + [
            C.c_void_p] * 5
        L.fnv_search_batch_filtered_grouped_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                                               C.c_int] + table + [C.c_void_p] * 6
        L.fnv_search_batch_exhaustive_grouped.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int] + table + [C.c_void_p] * 4
        L.fnv_search_batch_exhaustive_grouped_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int] + table + [
            C.c_void_p] * 5
    L.fnv_search_status.argtypes = [C.c_void_p]
    L.fnv_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.fnv_last_replayed_queries.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.fnv_last_launch_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.fnv_index_view.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    if hasattr(L, "fnv_index_adopt"):  # (older builds of the library, A/B'ed by tools/dev/knob_sweep.py, lack it)
        L.fnv_index_adopt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_int,
                                      C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    L.fnv_replicate.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    L.fnv_replica_refresh.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.fnv_search_batch_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                         C.c_int] + [C.c_void_p] * 5
    L.fnv_tune.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fnv_last_launch_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.fnv_gather_ceiling.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    # (round-5 entry points: an OLDER build of the library, loaded by the developer A/B tools through FLATNAV_HIP_LIB, lacks them)
    for name in ("fnv_lane_info", "fnv_last_handover_stats"):
        if hasattr(L, name) or LIB_PATH == os.path.join(HERE, "libflatnav_hip.so"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "fnv_index_half_rows"):  # (older builds under the A/B tools lack the half-width mirror)
        L.fnv_index_build_half_rows.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.fnv_index_half_rows.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    _lib = L
    return L


def check(rc: int) -> None:
    """Map C-ABI status codes onto the exceptions the reference raises at the same points."""
    if rc == FNV_OK:
        return
    msg = lib().fnv_last_error().decode()
    if rc == FNV_ERR_INVALID:
        raise ValueError(msg)
    if rc == FNV_ERR_NO_DEVICE:
        raise DeviceUnavailable(msg)
    raise RuntimeError(msg)


def row_layout(dim: int, dtype: str, capacity: int):
    """(row_bytes, tail_bytes) of the vector table the library keeps for this geometry (fnv_row_layout; needs no GPU)."""
    rb, tb = C.c_uint32(0), C.c_uint32(0)
    check(lib().fnv_row_layout(dim, DTYPE_ORD[dtype], capacity, C.byref(rb), C.byref(tb)))
    return int(rb.value), int(tb.value)


def device_count() -> int:
    n = C.c_int(0)
    check(lib().fnv_device_count(C.byref(n)))
    return n.value


def _np_dtype(name: str):
    return {"float32": np.float32, "uint8": np.uint8, "int8": np.int8, "float16": np.float16}[name]


MAX_FILTER_BITS = 1 << 31  # labels are int32: a bitmap never needs more bits


def pack_allowed(allowed):
    """The C ABI's filter bitmap for `allowed` -> (uint8 array, n_bits).  `allowed`: a 1-D bool mask indexed by label (n_bits =
    its length), or a 1-D integer array of labels (order and duplicates do not matter; n_bits = largest label + 1).  Byte L >> 3,
    bit L & 7 (little-endian bit order) = label L allowed.  A negative label raises ValueError."""
    a = np.asarray(allowed)
    if a.ndim != 1:
        raise ValueError("allowed must be a 1-D bool mask or a 1-D array of labels")
    if a.dtype == np.bool_:
        n_bits = int(a.size)
        if n_bits > MAX_FILTER_BITS:
            raise ValueError("allowed mask longer than 2^31 labels")
        return np.ascontiguousarray(np.packbits(a, bitorder="little")), n_bits
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("allowed must be a bool mask or an integer array of labels, not %s" % a.dtype)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint8), 0
    a = a.astype(np.int64, copy=False)
    if int(a.min()) < 0:
        raise ValueError("allowed labels must be non-negative")
    n_bits = int(a.max()) + 1
    if n_bits > MAX_FILTER_BITS:
        raise ValueError("allowed label %d does not fit an int32 label" % (n_bits - 1))
    mask = np.zeros(n_bits, dtype=np.bool_)
    mask[a] = True
    return np.ascontiguousarray(np.packbits(mask, bitorder="little")), n_bits


def pack_filters(filters):
    """The C ABI's filter TABLE of a grouped search -> (uint8 array [F, stride], n_bits).  `filters`: a sequence of anything
    pack_allowed takes (they may differ in kind and length), or a 2-D bool mask [F, labels].  n_bits is the largest of the
    filters' own; a shorter filter's row is zero beyond its own bits (those labels are not allowed).  Row f is filter f."""
    if isinstance(filters, np.ndarray) and filters.ndim == 2:
        if filters.dtype != np.bool_:
            raise ValueError("a 2-D filter table must be a bool mask [filters, labels]")
        packed = [pack_allowed(row) for row in filters]
    else:
        packed = [pack_allowed(f) for f in filters]
    n_bits = max([n for _, n in packed], default=0)
    table = np.zeros((len(packed), (n_bits + 7) // 8), dtype=np.uint8)
    for f, (bits, _) in enumerate(packed):
        table[f, :bits.size] = bits
    return table, n_bits


def _query_filter(query_filter, nq: int, n_filters: int) -> np.ndarray:
    """query_filter of a grouped search as the C ABI takes it: int32 [nq], every value -1 (no filter) or a row of the table."""
    a = np.asarray(query_filter)
    if a.ndim != 1 or a.size != nq:
        raise ValueError("query_filter must hold one entry per query")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("query_filter must be an integer array, not %s" % a.dtype)
    a = a.astype(np.int64, copy=False)
    bad = np.flatnonzero((a < -1) | (a >= n_filters))
    if bad.size:
        raise ValueError("query_filter[%d] = %d is neither -1 nor a filter of the table (n_filters = %d)"
                         % (int(bad[0]), int(a[bad[0]]), n_filters))
    return np.ascontiguousarray(a, dtype=np.int32)


def search_multi(indexes, queries, K: int, ef_search: int, num_initializations: int = 100, stats: bool = False):
    """One batch over several handles of the same index (replicas on several GPUs): rows [g*ceil(Q/G), ...) go to
    indexes[g], all devices work concurrently -> (dist float32[Q,K], labels int32[Q,K][, stats])."""
    first = indexes[0]
    q = np.ascontiguousarray(queries, dtype=_np_dtype(first.dtype))
    if q.ndim != 2 or q.shape[1] != first.dim:
        raise ValueError("Queries have incorrect dimensions.")
    nq = q.shape[0]
    d = np.empty((nq, K), dtype=np.float32)
    l = np.empty((nq, K), dtype=np.int32)
    cnt = np.empty(nq, dtype=np.int32)
    nd = np.zeros(nq, dtype=np.uint64)
    nh = np.zeros(nq, dtype=np.uint64)
    arr = (C.c_void_p * len(indexes))(*[ix._h for ix in indexes])
    check(lib().fnv_search_batch_multi(arr, len(indexes), q.ctypes.data, nq, K, ef_search, num_initializations,
                                       d.ctypes.data, l.ctypes.data, cnt.ctypes.data, nd.ctypes.data, nh.ctypes.data))
    if stats:
        return d, l, {"count": cnt, "n_dist": nd, "n_hops": nh}
    return d, l


class _Outputs:
    """The arrays a host-buffer search fills, in the order the C ABI takes them: dist float32[Q,K], labels int32[Q,K], then the
    per-query stats count, n_dist and -- for the graph searches -- n_hops."""

    def __init__(self, nq: int, K: int, hops: bool):
        self.dist = np.empty((nq, K), dtype=np.float32)
        self.labels = np.empty((nq, K), dtype=np.int32)
        self.stats = {"count": np.empty(nq, dtype=np.int32), "n_dist": np.zeros(nq, dtype=np.uint64)}
        if hops:
            self.stats["n_hops"] = np.zeros(nq, dtype=np.uint64)
        self.ptrs = [a.ctypes.data for a in (self.dist, self.labels, *self.stats.values())]

    def result(self, stats: bool):
        return (self.dist, self.labels, self.stats) if stats else (self.dist, self.labels)


class DeviceIndex:
    """An index resident in one GPU's HBM (vectors / links / labels in SoA form)."""

    def __init__(self, handle: C.c_void_p, owned: bool = True):
        """owned=False: a view of a handle that belongs to someone else (e.g. flatnav.index.*.device_handle());
        close() / garbage collection then leave it alone."""
        self._h = handle
        self._owned = owned
        info = (C.c_uint64 * 8)()
        check(lib().fnv_index_info(self._h, info))
        self.dtype = ORD_DTYPE[int(info[0])]
        self.M = int(info[1])
        self.row_bytes = int(info[2]) & 0xFFFFFFFF  # stride of the (main) vector table
        self.tail_bytes = int(info[2]) >> 32        # split rows (csrc/distance.hpp): bytes per row in the side table that follows it
        self.n_nodes = int(info[3])
        self.dim = int(info[4])
        self.metric = "l2" if int(info[5]) == 0 else "angular"
        self.device = int(info[6])

    @classmethod
    def upload(cls, blob: np.ndarray, node_size: int, data_size: int, M: int, n_nodes: int, dtype: str,
               metric: str, dim: int, device: int = 0) -> "DeviceIndex":
        blob = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
        if blob.size < node_size * n_nodes:
            raise ValueError("blob smaller than n_nodes * node_size")
        h = C.c_void_p()
        check(lib().fnv_index_upload(blob.ctypes.data, node_size, data_size, M, n_nodes, DTYPE_ORD[dtype],
                                     METRIC_ORD[metric], dim, device, C.byref(h)))
        return cls(h)

    @classmethod
    def alloc(cls, M: int, n_nodes: int, dtype: str, metric: str, dim: int, device: int = 0) -> "DeviceIndex":
        h = C.c_void_p()
        check(lib().fnv_index_alloc(M, n_nodes, DTYPE_ORD[dtype], METRIC_ORD[metric], dim, device, C.byref(h)))
        return cls(h)

    @classmethod
    def adopt(cls, buffers, M: int, n_nodes: int, dtype: str, metric: str, dim: int, device: int = 0, keep_alive=None) -> "DeviceIndex":
        """A handle on device buffers somebody else owns: `buffers` = [(ptr, nbytes)] * 3 as device_buffers() reports them
        (vectors at the library's row stride, links, labels).  `keep_alive`: whatever must outlive the handle."""
        h = C.c_void_p()
        check(lib().fnv_index_adopt(buffers[0][0], buffers[1][0], buffers[2][0], M, n_nodes, DTYPE_ORD[dtype],
                                    METRIC_ORD[metric], dim, device, C.byref(h)))
        v = cls(h)
        v._parent = keep_alive
        return v

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                check(lib().fnv_index_free(self._h))  # fails (ValueError) while views of this handle are alive
            self._h = None
            self._parent = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_buffers(self):
        """[(ptr, nbytes)] * 3 for vectors, links, labels (for RCCL broadcast / peer copies)."""
        ptrs = (C.c_void_p * 3)()
        sizes = (C.c_uint64 * 3)()
        check(lib().fnv_index_device_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[i] or 0), int(sizes[i])) for i in range(3)]

    # ---- incremental construction -------------------------------------------------------------
    def set_live_nodes(self, n_live: int) -> None:
        check(lib().fnv_index_set_live_nodes(self._h, int(n_live)))
        self.n_nodes = int(n_live)

    def write_nodes(self, first_node: int, rows: np.ndarray, node_size: int, data_size: int) -> None:
        """rows: uint8 blob of whole AoS node records for nodes first_node, first_node+1, ..."""
        rows = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
        if rows.size % node_size:
            raise ValueError("rows must hold whole node records")
        check(lib().fnv_index_write_nodes(self._h, int(first_node), rows.size // node_size, rows.ctypes.data,
                                          node_size, data_size))

    def write_links(self, node_ids: np.ndarray, link_rows: np.ndarray) -> None:
        ids = np.ascontiguousarray(node_ids, dtype=np.uint32).reshape(-1)
        rows = np.ascontiguousarray(link_rows, dtype=np.uint32).reshape(ids.size, self.M)
        check(lib().fnv_index_write_links(self._h, ids.ctypes.data, rows.ctypes.data, ids.size))

    def insert_batch(self, first_node: int, count: int, ef_construction: int, num_initializations: int = 100) -> int:
        """Search + wire nodes [first_node, first_node+count) on the device; returns the distance evaluations."""
        ev = C.c_uint64(0)
        check(lib().fnv_index_insert_batch(self._h, int(first_node), int(count), int(ef_construction),
                                           int(num_initializations), C.byref(ev)))
        self.n_nodes = int(first_node) + int(count)
        return int(ev.value)

    def read_links(self, first_node: int, count: int) -> np.ndarray:
        out = np.empty((int(count), self.M), dtype=np.uint32)
        check(lib().fnv_index_read_links(self._h, int(first_node), int(count), out.ctypes.data))
        return out

    def view(self) -> "DeviceIndex":
        """A second handle on the same device buffers with its own workspace: two searches in flight on one index."""
        h = C.c_void_p()
        check(lib().fnv_index_view(self._h, C.byref(h)))
        v = DeviceIndex(h)
        v._parent = self  # the view aliases this handle's buffers: keep it alive (the library refuses to free it first)
        return v

    def replicate(self, devices) -> list:
        """Replicas of this index on the given device ordinals (peer copies over xGMI); each is an independent handle."""
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        out = (C.c_void_p * len(devices))()
        check(lib().fnv_replicate(self._h, len(devices), devs, out))
        return [DeviceIndex(C.c_void_p(out[i])) for i in range(len(devices))]

    def refresh_replicas(self, replicas) -> None:
        arr = (C.c_void_p * len(replicas))(*[r._h for r in replicas])
        check(lib().fnv_replica_refresh(self._h, len(replicas), arr))
        for r in replicas:
            r.n_nodes = self.n_nodes

    # ---- the half-width mirror of a float32 index (include/flatnav_hip.h) -------------------------
    def build_half_rows(self) -> bool:
        """(Re)convert rows [0, n_live) into the half-width mirror (fnv_index_build_half_rows): needed after vectors were
        written through device_buffers().  True when a live mirror resulted."""
        built = C.c_int(0)
        check(lib().fnv_index_build_half_rows(self._h, C.byref(built)))
        return bool(built.value)

    def half_rows(self) -> dict:
        """State of the mirror this handle's searches read (fnv_index_half_rows)."""
        r = (C.c_uint64 * 4)()
        check(lib().fnv_index_half_rows(self._h, r))
        return {"state": ["none", "live", "dropped", "ineligible"][int(r[0])], "rows": int(r[1]), "bytes": int(r[2]),
                "used_by_last_launch": bool(int(r[3]))}

    def set_option(self, name: str, value: int) -> None:
        check(lib().fnv_set_option(self._h, name.encode(), int(value)))

    def _batch(self, queries, K: int, k_max, hops: bool):
        """What the host-buffer searches share: the queries as a C-contiguous array of the element type, checked, nq, and the
        output arrays (_Outputs).  k_max: the upper bound of K (None: there is none); hops: the search counts hops."""
        q = np.ascontiguousarray(queries, dtype=_np_dtype(self.dtype))
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("Queries have incorrect dimensions.")
        if k_max is not None and not 1 <= K <= k_max:
            raise ValueError("K of an exhaustive search must be between 1 and %d" % k_max)
        if K <= 0:
            raise ValueError("K must be positive")
        return q, q.shape[0], _Outputs(q.shape[0], K, hops)

    def search(self, queries, K: int, ef_search: int, num_initializations: int = 100, stats: bool = False):
        """Host-buffer batched search -> (dist float32[Q,K], labels int32[Q,K][, stats])."""
        q, nq, out = self._batch(queries, K, None, True)
        check(lib().fnv_search_batch(self._h, q.ctypes.data, nq, K, ef_search, num_initializations, *out.ptrs))
        return out.result(stats)

    def search_filtered(self, queries, K: int, ef_search: int, allowed, num_initializations: int = 100, stats: bool = False):
        """Host-buffer batched search restricted to the nodes whose label is allowed (fnv_search_batch_filtered) ->
        (dist float32[Q,K], labels int32[Q,K][, stats]).  `allowed`: see pack_allowed.  Rows with fewer than K allowed
        results are padded with (+inf, -1) (stats["count"] says how many are real); that is not an error."""
        q, nq, out = self._batch(queries, K, None, True)
        bits, n_bits = pack_allowed(allowed)
        check(lib().fnv_search_batch_filtered(self._h, q.ctypes.data, nq, K, ef_search, num_initializations,
                                              bits.ctypes.data if n_bits else None, n_bits, *out.ptrs))
        return out.result(stats)

    def search_exhaustive(self, queries, K: int, allowed=None, stats: bool = False):
        """Exhaustive search (fnv_search_batch_exhaustive): the exact K nearest among the live nodes, or -- `allowed` given, see
        pack_allowed -- among those whose label is allowed -> (dist float32[Q,K], labels int32[Q,K][, stats]).  Sorted by
        (distance, node id), NaN distances last.  Rows with fewer than K candidates are padded with (+inf, -1);
        stats = {"count": real entries per row, "n_dist": rows evaluated per query = the number of candidates}."""
        q, nq, out = self._batch(queries, K, 1024, False)
        bits, n_bits = pack_allowed(allowed) if allowed is not None else (None, 0)
        check(lib().fnv_search_batch_exhaustive(self._h, q.ctypes.data, nq, K, 0 if allowed is None else 1,
                                                bits.ctypes.data if n_bits else None, n_bits, *out.ptrs))
        return out.result(stats)

    def search_filtered_grouped(self, queries, K: int, ef_search: int, filters, query_filter, num_initializations: int = 100,
                                stats: bool = False):
        """search_filtered with one allowed set PER QUERY, in one launch (fnv_search_batch_filtered_grouped) ->
        (dist float32[Q,K], labels int32[Q,K][, stats]).  `filters`: see pack_filters; query_filter[q] = the filter query q
        uses, or -1 for none.  Row q is what search_filtered returns for that query with that filter (search for -1)."""
        q, nq, out = self._batch(queries, K, None, True)
        table, n_bits = pack_filters(filters)
        qf = _query_filter(query_filter, nq, table.shape[0])
        check(lib().fnv_search_batch_filtered_grouped(self._h, q.ctypes.data, nq, K, ef_search, num_initializations,
                                                      table.ctypes.data if table.size else None, table.shape[0],
                                                      table.shape[1], n_bits, qf.ctypes.data, *out.ptrs))
        return out.result(stats)

    def search_exhaustive_grouped(self, queries, K: int, filters, query_filter, stats: bool = False):
        """search_exhaustive with one allowed set PER QUERY, in one launch (fnv_search_batch_exhaustive_grouped) ->
        (dist float32[Q,K], labels int32[Q,K][, stats]).  `filters`: see pack_filters; query_filter[q] = the filter query q
        uses, or -1 for every live node.  Row q is what search_exhaustive returns for that query with that filter."""
        q, nq, out = self._batch(queries, K, 1024, False)
        table, n_bits = pack_filters(filters)
        qf = _query_filter(query_filter, nq, table.shape[0])
        check(lib().fnv_search_batch_exhaustive_grouped(self._h, q.ctypes.data, nq, K, table.ctypes.data if table.size else None,
                                                        table.shape[0], table.shape[1], n_bits, qf.ctypes.data, *out.ptrs))
        return out.result(stats)

    def search_into(self, queries: np.ndarray, K: int, ef_search: int, dist: np.ndarray, labels: np.ndarray,
                    num_initializations: int = 100) -> None:
        """Host-buffer batched search into arrays the CALLER owns (no allocation, no conversion): queries [Q, dim] of the index's
        element type, dist float32 [Q, K], labels int32 [Q, K], all C-contiguous.  When all three are pinned host memory
        (e.g. numpy views of torch tensors from pin_memory()) the call is zero-copy at any batch size."""
        if (queries.dtype != _np_dtype(self.dtype) or queries.ndim != 2 or queries.shape[1] != self.dim or not queries.flags.c_contiguous):
            raise ValueError("Queries have incorrect dimensions.")
        nq = queries.shape[0]
        if dist.shape != (nq, K) or labels.shape != (nq, K) or dist.dtype != np.float32 or labels.dtype != np.int32 \
                or not dist.flags.c_contiguous or not labels.flags.c_contiguous:
            raise ValueError("output arrays must be C-contiguous float32 / int32 [Q, K]")
        check(lib().fnv_search_batch(self._h, queries.ctypes.data, nq, K, ef_search, num_initializations, dist.ctypes.data,
                                     labels.ctypes.data, None, None, None))

    def search_device(self, q_ptr: int, nq: int, K: int, ef_search: int, num_initializations: int, dist_ptr: int,
                      label_ptr: int, count_ptr: int = 0, ndist_ptr: int = 0, nhops_ptr: int = 0,
                      stream: int = 0) -> None:
        """Device-buffer batched search, enqueued on `stream` (raw hipStream_t handle, 0 = null stream)."""
        check(lib().fnv_search_batch_device(self._h, q_ptr, nq, K, ef_search, num_initializations, dist_ptr,
                                            label_ptr, count_ptr or None, ndist_ptr or None, nhops_ptr or None,
                                            stream or None))

    def search_device_filtered(self, q_ptr: int, nq: int, K: int, ef_search: int, num_initializations: int, bits_ptr: int,
                               n_bits: int, dist_ptr: int, label_ptr: int, count_ptr: int = 0, ndist_ptr: int = 0,
                               nhops_ptr: int = 0, stream=None) -> None:
        """Device-buffer filtered search (fnv_search_batch_filtered_device): every pointer, the label bitmap `bits_ptr` of
        `n_bits` bits included, is device memory; enqueued on `stream` (raw hipStream_t handle, None / 0 = null stream).
        A candidate-heap overflow is reported by status()."""
        check(lib().fnv_search_batch_filtered_device(self._h, q_ptr, nq, K, ef_search, num_initializations, bits_ptr or None,
                                                     int(n_bits), dist_ptr, label_ptr, count_ptr or None, ndist_ptr or None,
                                                     nhops_ptr or None, stream or None))

    def search_device_exhaustive(self, q_ptr: int, nq: int, K: int, dist_ptr: int, label_ptr: int, count_ptr: int = 0,
                                 ndist_ptr: int = 0, bits_ptr: int = 0, n_bits: int = 0, use_filter: bool = False,
                                 stream=None) -> None:
        """Device-buffer exhaustive search (fnv_search_batch_exhaustive_device): every pointer is device memory; with
        `use_filter` the label bitmap `bits_ptr` of `n_bits` bits restricts the candidates (n_bits = 0: the empty filter).
        Enqueued on `stream` (raw hipStream_t handle, None / 0 = null stream) without synchronising."""
        check(lib().fnv_search_batch_exhaustive_device(self._h, q_ptr, nq, K, 1 if use_filter else 0, bits_ptr or None,
                                                       int(n_bits), dist_ptr, label_ptr, count_ptr or None, ndist_ptr or None,
                                                       stream or None))

    def search_device_filtered_grouped(self, q_ptr: int, nq: int, K: int, ef_search: int, num_initializations: int,
                                       filters_ptr: int, n_filters: int, stride_bytes: int, n_bits: int, query_filter_ptr: int,
                                       dist_ptr: int, label_ptr: int, count_ptr: int = 0, ndist_ptr: int = 0, nhops_ptr: int = 0,
                                       stream=None) -> None:
        """Device-buffer grouped filtered search (fnv_search_batch_filtered_grouped_device): every pointer -- the filter table
        (`n_filters` bitmaps of `n_bits` bits, `stride_bytes` apart) and the int32 `query_filter_ptr` [nq] included -- is device
        memory; enqueued on `stream` without synchronising.  A query_filter value that is neither -1 nor a filter of the table
        gives that query the empty filter."""
        check(lib().fnv_search_batch_filtered_grouped_device(self._h, q_ptr, nq, K, ef_search, num_initializations,
                                                             filters_ptr or None, int(n_filters), int(stride_bytes), int(n_bits),
                                                             query_filter_ptr or None, dist_ptr, label_ptr, count_ptr or None,
                                                             ndist_ptr or None, nhops_ptr or None, stream or None))

    def search_device_exhaustive_grouped(self, q_ptr: int, nq: int, K: int, filters_ptr: int, n_filters: int, stride_bytes: int,
                                         n_bits: int, query_filter_ptr: int, dist_ptr: int, label_ptr: int, count_ptr: int = 0,
                                         ndist_ptr: int = 0, stream=None) -> None:
        """Device-buffer grouped exhaustive search (fnv_search_batch_exhaustive_grouped_device); arguments as
        search_device_filtered_grouped."""
        check(lib().fnv_search_batch_exhaustive_grouped_device(self._h, q_ptr, nq, K, filters_ptr or None, int(n_filters),
                                                               int(stride_bytes), int(n_bits), query_filter_ptr or None, dist_ptr,
                                                               label_ptr, count_ptr or None, ndist_ptr or None, stream or None))

    def tune(self, queries, K: int, ef_search: int, num_initializations: int = 100, nq: int = 0) -> None:
        """Settle the adaptive kernel choice for (K, ef_search, this batch size) in one call (fnv_tune): afterwards no
        launch of that shape is an exploratory one.  `queries`: host array [Q, dim], or a device pointer (int) + nq."""
        if isinstance(queries, int):
            check(lib().fnv_tune(self._h, queries, int(nq), 1, K, ef_search, num_initializations))
            return
        q = np.ascontiguousarray(queries, dtype=_np_dtype(self.dtype))
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("Queries have incorrect dimensions.")
        check(lib().fnv_tune(self._h, q.ctypes.data, q.shape[0], 0, K, ef_search, num_initializations))

    def launch_info(self) -> dict:
        """Variant of the most recent launch, whether it was an exploratory sample of the adaptive choice, and the host
        timestamps (ns, steady clock) of the most recent host-buffer search."""
        r = (C.c_uint64 * 4)()
        check(lib().fnv_last_launch_info(self._h, r))
        names = ["two_heaps", "merged_beam", "merged_beam_tail50", "merged_beam_tail75", "merged_beam_tail100",
                 "merged_beam_tail25", "merged_beam_tail_shadows"]
        return {"variant": names[int(r[0])], "variant_id": int(r[0]), "exploratory": bool(int(r[1]) & 1),
                "shadow": bool(int(r[1]) & 2),
                "enqueued_ns": int(r[2]), "completed_ns": int(r[3])}

    def gather_ceiling(self, waves_per_cu: int = 0) -> float:
        """GB/s of row bytes a pure random-row gather of this index's vector table reaches (fnv_gather_ceiling)."""
        v = C.c_double(0)
        check(lib().fnv_gather_ceiling(self._h, int(waves_per_cu), C.byref(v)))
        return float(v.value)

    def status(self) -> None:
        check(lib().fnv_search_status(self._h))

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0)
        check(lib().fnv_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def replayed_queries(self) -> dict:
        """Queries of the last search that the exact kernel replayed after the merged-beam kernel handed them over, by reason."""
        r = (C.c_uint64 * 5)()
        check(lib().fnv_last_replayed_queries(self._h, r))
        return dict(zip(["total", "eviction_tie", "selection_tie", "result_tie", "nan_inf"], [int(x) for x in r]))

    def handover_stats(self) -> dict:
        """Hand-overs of the last search (fnv_last_handover_stats): queries resumed from their log, hops taken from the logs,
        hops those queries' merged-beam passes had made, queries searched again from scratch."""
        r = (C.c_uint64 * 4)()
        if not hasattr(lib(), "fnv_last_handover_stats"):  # (an older build under the A/B tools)
            return dict(zip(["resumed", "hops_from_log", "hops_of_resumed", "from_scratch"], [0, 0, 0, self.replayed_queries()["total"]]))
        check(lib().fnv_last_handover_stats(self._h, r))
        return dict(zip(["resumed", "hops_from_log", "hops_of_resumed", "from_scratch"], [int(x) for x in r]))

    def launch_geometry(self) -> dict:
        g = (C.c_uint64 * 8)()
        check(lib().fnv_last_launch_geometry(self._h, g))
        keys = ["grid_blocks", "block_threads", "lds_bytes", "blocks_per_cu", "visited_slots", "cand_slots"]
        out = {k: int(g[i]) for i, k in enumerate(keys)}
        out["kernel"] = ["two_heaps", "merged_beam_registers", "merged_beam_lds", "exhaustive_scan"][int(g[6])]
        out["tail_exact"] = int(g[7])
        if int(g[6]) == 3 and int(g[4]):  # the grouped scan reports its tiling in the slots the graph search's layout uses
            out["tile_queries"], out["queue_ids"], out["segments"] = int(g[3]), int(g[4]), int(g[5])
        return out


def _lane_info(dev) -> list:
    r = (C.c_uint64 * 16)()
    check(lib().fnv_lane_info(dev._h, r))
    return [int(x) for x in r]


def lane_workspaces(dev) -> list:
    """Bytes of launch workspace (HBM) held by the handle [0] and by each of its hidden lanes [1..7] (fnv_lane_info)."""
    return _lane_info(dev)[0::2]


def lane_exploratory_launches(dev) -> list:
    """Exploratory launches of the adaptive kernel choice on the handle [0] and on each hidden lane [1..7] (always 0 there)."""
    return _lane_info(dev)[1::2]
