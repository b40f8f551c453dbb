"""The build's translation units and its staleness rule (flatnav_amd/build.py), checked without a compiler: the host units
behind csrc/runtime.hpp are rebuilt one by one, a change to runtime.hpp rebuilds them all and no kernel object, a change to a
device header rebuilds every kernel object."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["index.hip", "launch.hip", "host_search.hip", "multi.hip", "tune.hip", "device_build.hip"]


def _is_host(src):
    return os.path.basename(src) != "kernel_inst.hip"


def test_every_host_source_exists_and_object_names_are_unique():
    from flatnav_amd import build

    units = build._units(())
    host = [s for _, s, _ in units if _is_host(s)]
    assert sorted(os.path.basename(s) for s in host) == sorted(HOST)
    assert all(os.path.isfile(s) for s in host)
    assert all(not f for _, s, f in units if _is_host(s))  # a host unit takes no -D of its own
    objs = [o for o, _, _ in units]
    assert len(set(objs)) == len(objs) > len(HOST)  # (the host units, then the kernel-instantiation units)
    assert len({os.path.basename(o) for o in objs}) == len(objs)  # (custom builds re-root them into one directory)


def test_the_developer_build_compiles_the_host_units_only():
    from flatnav_amd import build

    units = build._units(("FNV_PHASE_TIMING", "FNV_DEV_FAST_BUILD"))
    assert sorted(os.path.basename(s) for _, s, _ in units) == sorted(HOST)
    assert all(f == ["-DFNV_PHASE_TIMING", "-DFNV_DEV_FAST_BUILD"] for _, _, f in units)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """build.py over a copy of the sources whose modification times the test sets: every source at T, every object at T + 10."""
    tmp_path = tmp_path_factory.mktemp("build_units")
    for rel in ("flatnav_amd/csrc", "include"):
        shutil.copytree(os.path.join(ROOT, rel), tmp_path / rel, ignore=shutil.ignore_patterns("_obj*", "*.o"))
    shutil.copy(os.path.join(ROOT, "flatnav_amd", "build.py"), tmp_path / "flatnav_amd" / "build.py")
    spec = importlib.util.spec_from_file_location("build_units_copy", str(tmp_path / "flatnav_amd" / "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.CSRC == str(tmp_path / "flatnav_amd" / "csrc")
    T = 1_700_000_000
    for top in (tmp_path / "flatnav_amd" / "csrc", tmp_path / "include"):
        for d, _, files in os.walk(top):
            for f in files:
                os.utime(os.path.join(d, f), (T, T))
    os.makedirs(build.OBJ)
    units = build._units(())
    for o, _, _ in units:
        open(o, "w").close()
        os.utime(o, (T + 10, T + 10))

    def stale_after_touching(name):
        path = os.path.join(build.CSRC, name)
        os.utime(path, (T + 20, T + 20))
        try:
            return {os.path.basename(o) for o, s, _ in units if build._stale(o, s)}
        finally:
            os.utime(path, (T, T))

    host_objs = {os.path.basename(o) for o, s, _ in units if _is_host(s)}
    kernel_objs = {os.path.basename(o) for o, s, _ in units if not _is_host(s)}
    assert stale_after_touching("kernel_table.h") == host_objs | kernel_objs  # (and nothing is stale before a touch:)
    assert not any(build._stale(o, s) for o, s, _ in units)
    return stale_after_touching, host_objs, kernel_objs


@pytest.mark.parametrize("name", HOST)
def test_touching_one_host_unit_makes_exactly_its_object_stale(tree, name):
    stale_after_touching, _, _ = tree
    assert stale_after_touching(name) == {name[:-4] + ".o"}


def test_touching_runtime_hpp_makes_every_host_object_stale_and_no_kernel_object(tree):
    stale_after_touching, host_objs, kernel_objs = tree
    assert len(host_objs) == len(HOST) and len(kernel_objs) >= 100
    assert stale_after_touching("runtime.hpp") == host_objs
    assert stale_after_touching("launch_plan.hpp") == host_objs


def test_touching_a_device_header_makes_every_kernel_object_stale(tree):
    stale_after_touching, host_objs, kernel_objs = tree
    assert stale_after_touching("distance.hpp") >= kernel_objs
    assert stale_after_touching("distance.hpp") >= host_objs  # (every host unit includes it through kernel_table.h)
    # the kernel headers only launch.hip includes (scan.hpp: its non-template kernels) leave the other host units alone
    assert stale_after_touching("scan.hpp") == kernel_objs | {"launch.o"}
    assert stale_after_touching("merged_beam.hpp") == kernel_objs | {"launch.o"}
