"""The device mirror's protocol (include/flatnav/index/DeviceMirror.h, driven through flatnav::Index) on the CPU:
tests/cpp/test_device_mirror.cpp is linked with plain g++ against tests/cpp/fake_hip_abi.cpp, a recording stand-in for the C ABI,
and its log -- which calls follow which host mutation, with which node ranges, link rows and payload bytes -- is compared line
by line with tests/golden/device_mirror_calls.txt.  That file was recorded from the header as it stood BEFORE the mirror was
moved out of Index.h and is not regenerated from later code: a change to it is a change of protocol and has to be argued as one.

So that the stored file is not the only judge, the rules the mirror promises are also checked on the parsed log: what an
increment ships, how a failed write is recovered from, when a batch is spread over replicas, and the counter arithmetic.

The second case runs the same program under AddressSanitizer + UndefinedBehaviorSanitizer with nothing suppressed (a stand-alone
program with its own main: nothing is preloaded, nothing touches a GPU)."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "test_device_mirror.cpp"), os.path.join(ROOT, "tests", "cpp", "fake_hip_abi.cpp")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "device_mirror_calls.txt")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
NDIST_PER_QUERY = 5  # what the stand-in reports for every query
GRAPH_SEARCHES = {"search", "search_filtered", "search_filtered_grouped", "multi"}
SCAN_SEARCHES = {"search_exhaustive", "search_exhaustive_grouped"}


def build_and_run(tmp, name, extra=()):
    exe = os.path.join(tmp, name)
    subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", "-pthread", *extra, "-I" + os.path.join(ROOT, "include"), *SOURCES, "-o", exe],
                   check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS", "FLATNAV_DEVICES")}
    return subprocess.run([exe, tmp], capture_output=True, text=True, timeout=300, env=env)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = build_and_run(str(tmp_path_factory.mktemp("device_mirror")), "test_device_mirror")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return out


class Call:
    """One line of the stand-in: name, '#n' handle (None for multi), key=value fields, whether it was made to fail."""

    def __init__(self, line):
        self.line = line
        self.failed = line.endswith(" -> FAIL")
        words = line.replace(" -> FAIL", "").split()
        self.name = words[0]
        self.handle = next((w for w in words[1:] if w.startswith("#")), None)
        self.args = dict(w.split("=", 1) for w in words[1:] if "=" in w)

    def num(self, key):
        return int(self.args[key])


def parse(log):
    """-> {scenario number: [step]}, step = {"what": the driver's '> ...' line, "calls": [Call], "notes": [indented lines]}."""
    scenarios, steps = {}, []  # (steps before the first scenario line belong to the fixture's construction)
    for line in log.splitlines():
        if line.startswith("-- scenario "):
            steps = scenarios.setdefault(int(line.split()[2].rstrip(":")), [])
        elif line.startswith("> "):
            steps.append({"what": line[2:], "calls": [], "notes": []})
        elif line.startswith("  "):
            steps[-1]["notes"].append(line.strip())
        else:
            steps[-1]["calls"].append(Call(line))
    return scenarios


@pytest.fixture(scope="module")
def scenarios(run):
    return parse(run.stdout)


def test_call_log_is_the_one_recorded_before_the_refactor(run):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = run.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}: got {g!r}, recorded {w!r}"
    assert len(got) == len(want)
    assert sorted(parse(run.stdout)) == list(range(1, 14))


def test_an_increment_ships_the_new_nodes_and_the_dirty_rows_below_the_watermark(scenarios):
    steps = scenarios[2]
    assert steps[0]["what"].startswith("host add: 10 nodes")
    names = [c.name for c in steps[1]["calls"]]
    assert names == ["write_nodes", "write_links", "set_live", "search"]
    # everywhere but in the device-assisted builder (which writes the rows of its own new nodes): per handle, the watermark is
    # what the last set_live / upload said; an increment appends from there and rewrites only rows below it, in ascending order
    live = {}
    for number, steps in scenarios.items():
        for step in steps:
            calls = step["calls"]
            for i, c in enumerate(calls):
                if c.name == "upload" or (c.name == "set_live" and not c.failed):
                    live[c.handle] = c.num("n")
                if c.name == "write_links":
                    assert c.num("ascending") == 1 and c.num("count") > 0, c.line
                    if number != 12:
                        assert c.num("max_id") < live[c.handle], c.line
                        after = next((x for x in calls[i + 1:] if x.name == "set_live"), None)
                        assert c.failed or c.num("count") <= after.num("n") // 4, c.line  # (more dirty rows: the whole store goes)
                if c.name == "write_nodes" and c.num("first") != 0 and number != 12:
                    assert c.num("first") == live[c.handle], c.line


def test_after_a_failed_write_the_next_sync_frees_the_handle_and_ships_the_whole_store(scenarios):
    seen = set()
    for number in (5, 12):
        steps = scenarios[number]
        for i, step in enumerate(steps):
            failed = [c for c in step["calls"] if c.failed]
            if not failed:
                continue
            assert len(failed) == 1 and failed[0] is [c for c in step["calls"] if c.name != "set_option"][-1]  # nothing after it
            assert any(n.startswith("threw runtime_error: injected failure in " + failed[0].name) for n in step["notes"])
            seen.add(failed[0].name)
            nxt = next(s for s in steps[i + 1:] if s["calls"])["calls"]
            assert nxt[0].name == "free" and nxt[0].handle == failed[0].handle
            assert nxt[1].name in ("alloc", "upload") and nxt[1].handle != failed[0].handle
            if nxt[1].name == "alloc":
                assert nxt[2].name == "write_nodes" and nxt[2].num("first") == 0 and nxt[3].name == "set_live"
                assert nxt[2].num("count") == nxt[3].num("n")
    assert seen == {"write_nodes", "write_links", "set_live", "insert_batch"}


def test_batches_are_spread_only_from_64_queries_per_device(scenarios, run):
    spread = 0
    for number, steps in scenarios.items():
        for step in steps:
            m = re.match(r"searchBatch nq=(\d+)", step["what"])
            for c in step["calls"]:
                if c.name == "replicate":
                    assert m and int(m.group(1)) >= 64 * (c.num("n") + 1), c.line
                if c.name == "multi":
                    n = int(c.line.split()[1])
                    assert int(m.group(1)) >= 64 * n and len(c.args["handles"].split(",")) == n, c.line
                    spread += 1
    assert spread >= 6
    eight = scenarios[8]
    by_nq = {s["what"]: [c.name for c in s["calls"]] for s in eight[:4]}
    assert by_nq["searchBatch nq=100"][-1] == "search" and "replicate" not in by_nq["searchBatch nq=100"]
    assert by_nq["searchBatch nq=191"] == ["search"] and by_nq["searchBatch nq=192"] == ["replicate", "multi"]
    # a refresh that fails: those replicas are freed and made anew; a replication the caller asked for that fails: throws
    refresh = next(s for s in eight if any(c.name == "refresh" and c.failed for c in s["calls"]))
    tail = refresh["calls"][[c.name for c in refresh["calls"]].index("refresh"):]
    assert [c.name for c in tail] == ["refresh", "free", "free", "replicate", "multi"]
    assert ",".join(c.handle for c in tail[1:3]) == tail[0].args["replicas"]
    failed = next(s for s in eight if any(c.name == "replicate" and c.failed for c in s["calls"]))
    assert failed["calls"][-1].name == "replicate" and failed["notes"][0].startswith("threw runtime_error")
    # ... and one nobody asked for (FLATNAV_DEVICES=all): one warning, the primary alone from then on
    nine = [s for s in scenarios[9] if s["what"].startswith("searchBatch")]
    assert [c.name for c in nine[0]["calls"]][-2:] == ["replicate", "search"] and nine[0]["notes"] == ["returned"]
    assert [c.name for c in nine[1]["calls"]] == ["search"]
    assert len(re.findall(r"^flatnav: replicating the index over 3 visible GPUs failed", run.stderr, re.M)) == 1


def test_distance_computations_are_the_entry_cost_plus_what_the_device_counted(scenarios):
    checked = set()
    for step in scenarios[11]:
        searches = [c for c in step["calls"] if c.name in GRAPH_SEARCHES | SCAN_SEARCHES]
        assert all(c.num("ndist") == 1 for c in searches)
        total = next((int(n.split("=")[1]) for n in step["notes"] if n.startswith("distanceComputations=")), None)
        if total is None:
            assert not searches
            continue
        if not searches or searches[0].failed:
            assert total == 0
            continue
        (c,) = searches
        init_cost = c.num("n_init") if c.name in GRAPH_SEARCHES else 0
        assert total == init_cost * c.num("nq") + NDIST_PER_QUERY * c.num("nq"), step["what"]
        checked.add(c.name)
    assert checked == (GRAPH_SEARCHES | SCAN_SEARCHES) - {"multi"}
    # without collect_stats nobody asks the device for counts (and the frame has nothing to size)
    for number in (1, 2, 3, 4, 5, 8, 10, 13):
        for step in scenarios[number]:
            assert all(c.num("ndist") == 0 for c in step["calls"] if c.name in GRAPH_SEARCHES | SCAN_SEARCHES)


def test_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path, run):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run(["g++", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + linked.stderr.strip().splitlines()[-1])
    out = build_and_run(str(tmp_path), "test_device_mirror_san", SANITIZE)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.stdout == run.stdout
