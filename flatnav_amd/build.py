"""Builds the in-tree gfx950 shared library (C ABI of include/flatnav_hip.h) with hipcc.

hipcc cross-compiles for gfx950 without a GPU, so this runs in the dev container as well as on the MI355X box.
The kernels are templates over <element type, metric, row configuration>; their instantiations are compiled as 104
objects (kernel_inst.hip: 13 kernel families x 4 element types x 2 metrics) in parallel, eighteen more for float32 queries on
half-width mirror rows (HALF_ROWS_FAMILIES x 2 metrics), plus the host units behind csrc/runtime.hpp (HOST_UNITS: host code,
C ABI, the non-template kernels), one object each in the same pool, and linked into libflatnav_hip.so.  Objects are cached in csrc/_obj and rebuilt
when a source they include is newer.  The .so stays in-tree (git-ignored, but shipped by gpurun)."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libflatnav_hip.so")
HEADERS = [os.path.join(CSRC, f) for f in ("search_types.h", "search_params.h", "kernel_table.h", "heaps.hpp", "distance.hpp",
                                           "visited.hpp", "kernels.hpp", "wire.hpp", "merged_beam.hpp", "runtime.hpp",
                                           "launch_plan.hpp", "measurements.hpp", "half_rows.hpp", "scan.hpp", "scan_select.hpp")] + [
    os.path.join(ROOT, "include", "flatnav", "util", "StlExact.h"), os.path.join(ROOT, "include", "flatnav_hip.h")]
# The host units behind runtime.hpp, which brings launch_plan.hpp with measurements.hpp (kernel units include none) and, through kernel_table.h,
# the device headers that say what a launch passes.  Each unit with the kernel headers it includes on top of those (launch.hip:
# scan.hpp for its non-template kernels; the others in developer builds, where it instantiates the search kernels itself).
HOST_HEADERS = ("runtime.hpp", "launch_plan.hpp", "measurements.hpp")
KERNEL_HEADERS = ("scan.hpp", "kernels.hpp", "merged_beam.hpp", "visited.hpp")
HOST_UNITS = {"index.hip": (), "launch.hip": KERNEL_HEADERS, "host_search.hip": (), "multi.hip": (), "tune.hip": (),
              "device_build.hip": ()}
INST = os.path.join(CSRC, "kernel_inst.hip")
TYPES = [("float", "f32"), ("uint8_t", "u8"), ("int8_t", "i8"), ("_Float16", "f16")]
METRICS = [(0, "l2"), (1, "ip")]
# (ordinal, name) as in kernel_table.h's FNV_FOR_EACH_FAMILY; a family missing here fails at link time
FAMILIES = [(0, "exact"), (3, "wire"), (4, "merged"), (5, "merged1"), (6, "merged0"), (7, "merged2"),
            (8, "merged_d"), (9, "merged1_d"), (10, "merged0_d"), (11, "merged2_d"),  # 8-11: the DIRECT forms (small launches)
            (12, "exact_f"),  # the filtered two-heap kernel
            (13, "scan"),  # the exhaustive search's scan (csrc/scan.hpp)
            (14, "scan_g")]  # ... with one filter per query (fnv_search_batch_exhaustive_grouped)
# the row format f32h (csrc/half_rows.hpp; kernel_table.h's FNV_FOR_EACH_HALF_ROWS_FAMILY): the families that read mirror rows
HALF_ROWS_TYPE = ("fnv_dev::f32h", "f32h")
HALF_ROWS_FAMILIES = [f for f in FAMILIES if f[0] == 0 or 4 <= f[0] <= 11]  # exact, merged beam and its DIRECT forms


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _units(defines):
    """(object path, source, extra -D flags) for every translation unit."""
    units = [(os.path.join(OBJ, name[:-4] + ".o"), os.path.join(CSRC, name), []) for name in HOST_UNITS]
    if "FNV_DEV_FAST_BUILD" in defines:  # developer build: the host units only, one instantiation per kernel (launch.hip)
        return [(o, s, f + ["-D" + d for d in defines]) for o, s, f in units]
    for (ctype, tag), families, extra in [(t, FAMILIES, []) for t in TYPES] + [(HALF_ROWS_TYPE, HALF_ROWS_FAMILIES,
                                                                                 ["-DFNV_INST_HALF_ROWS"])]:
        for metric, mtag in METRICS:
            for fam, fname in families:
                units.append((os.path.join(OBJ, "inst_%s_%s_%s.o" % (fname, tag, mtag)), INST,
                              ["-DFNV_INST_T=" + ctype, "-DFNV_INST_TAG=" + tag, "-DFNV_INST_METRIC=%d" % metric,
                               "-DFNV_INST_MTAG=" + mtag, "-DFNV_INST_FAMILY=%d" % fam, "-DFNV_INST_FNAME=" + fname] + extra))
    return [(o, s, f + ["-D" + d for d in defines]) for o, s, f in units]


def _stale(obj, src):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    name = os.path.basename(src)
    if name in HOST_UNITS:
        deps = [h for h in HEADERS if os.path.basename(h) not in KERNEL_HEADERS or os.path.basename(h) in HOST_UNITS[name]]
    else:  # runtime.hpp, launch_plan.hpp and measurements.hpp (the launch planner) are included by the host units only
        deps = [h for h in HEADERS if os.path.basename(h) not in HOST_HEADERS]
    return any(os.path.getmtime(d) > t for d in [src] + deps)


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in [os.path.join(CSRC, name) for name in HOST_UNITS] + [INST] + HEADERS)


def build(force: bool = False, verbose: bool = False, defines=(), out: str | None = None, jobs: int | None = None) -> str:
    out = out or LIB
    custom = bool(defines) or out != LIB  # profiling / experiment builds get their own object directory
    if not force and not custom and not needs_build():
        return LIB
    if custom:  # its own object directory: readable prefix + a hash of the whole define set and the output (no collisions)
        import hashlib

        tag = "_".join(sorted(d.replace("=", "-") for d in defines))
        objdir = OBJ + "_" + tag[:60] + "_" + hashlib.sha1((tag + "|" + out).encode()).hexdigest()[:10]
    else:
        objdir = OBJ
    os.makedirs(objdir, exist_ok=True)
    base = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-inline-asm",
            "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include")]
    if verbose:
        base.insert(1, "-Rpass-analysis=kernel-resource-usage")
    units = [(os.path.join(objdir, os.path.basename(o)), s, f) for o, s, f in _units(defines)]
    todo = [(o, s, f) for o, s, f in units if force or custom or _stale(o, s)]

    def compile_one(unit):
        o, s, f = unit
        cmd = base + f + ["-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)

    jobs = jobs or max(1, min(8, os.cpu_count() or 1))
    with ThreadPoolExecutor(jobs) as pool:
        list(pool.map(compile_one, todo))
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden"] +
                          [o for o, _, _ in units] + ["-o", out])
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose="-v" in sys.argv)
    print(LIB)
