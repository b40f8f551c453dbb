"""A real fnv_tune, replayed: the measurements it logs (FLATNAV_TUNE_LOG, every compared value as a hex float) are fed, in
the order they were taken, to the CPU harness of the same tournament (tests/test_adaptive_choice.py).  The harness must ask
for exactly those measurements, land on the layout the next search launches with, and settle times under which the adaptive
choice picks the variant that search runs.  Nothing here depends on what a launch's time was."""
import re

import numpy as np
import pytest

from flatnav_amd import datasets as ds
from test_adaptive_choice import LOG_DUEL, TIME, tournament

pytestmark = pytest.mark.gpu
K, EF = 10, 64
LAYOUT = re.compile(r"fnv_tune B=(\d+) layout (\d+) \(heap in LDS (-?\d+), table (\d+)\): merged \S+ ms, 75% tail exact \S+ ms "
                    r"-> (\d+) slots, (\d+) per CU \[(\S+) (\S+), (\d+) heap entries\]$")
DUEL = re.compile(r"fnv_tune B=(\d+) duel \((\d) rounds?\): layout (\d+) \S+ ms against layout (\d+) \S+ ms -> (challenger|holder) \[(\S+) (\S+)\]$")
VARIANT = re.compile(r"fnv_tune B=(\d+) variant (\d+): \S+ ms \[(\S+)\]$")
SETTLING = re.compile(r"fnv_tune B=(\d+) settling: \S+ ms \(at \S+ s\)$")


@pytest.fixture(scope="module")
def hipmod():
    from flatnav_amd import hip

    assert hip.device_count() >= 1, "no MI355X visible"
    return hip


@pytest.fixture(scope="module")
def index(oracle_mod):
    X, Q = ds.sift_like(8000, 6000)
    ix = oracle_mod.OracleIndex.create("l2", 128, 8000, 16)
    ix.add(X, 64)
    return ix, Q


def f32(text):
    return np.float32(float.fromhex(text))


def tune_and_log(dev, Q, monkeypatch, capfd):
    monkeypatch.setenv("FLATNAV_TUNE_LOG", "1")
    capfd.readouterr()
    dev.tune(Q, K, EF)
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("fnv_tune ")]
    print("\n".join(lines))
    assert all(LAYOUT.match(l) or DUEL.match(l) or VARIANT.match(l) or SETTLING.match(l) for l in lines), lines
    return lines


@pytest.mark.parametrize("nq,tune_layout", [(6000, 1), (2048, 1), (6000, 0)],
                         ids=["more_than_one_round", "one_round", "the_rules_layout_only"])
def test_a_tune_replayed_on_the_cpu_lands_where_the_gpu_did(hipmod, index, monkeypatch, capfd, nq, tune_layout):
    ix, Q = index
    Q = Q[:nq]
    dev = hipmod.DeviceIndex.upload(ix.blob(), ix.node_size, ix.data_size, ix.M, ix.cur_nodes, ix.dtype, ix.metric, ix.dim)
    if not tune_layout:
        dev.set_option("tune_layout", 0)
    lines = tune_and_log(dev, Q, monkeypatch, capfd)
    layouts = [LAYOUT.match(l) for l in lines if LAYOUT.match(l)]
    variants = [VARIANT.match(l) for l in lines if VARIANT.match(l)]
    assert layouts and variants and all(int(m.group(1)) == max(EF, K) for m in layouts + variants)
    n_cands = max(int(m.group(2)) for m in layouts) + 1
    assert (n_cands == 1) == (not tune_layout)

    # the script: every logged measurement, in the order it was taken (a layout line is one or two of them: the merged-beam
    # kernel alone and, in a launch of more than one round, its 75 % tail); a candidate with no line at all failed its first
    script, multi, geometry = [], [0] * n_cands, {}
    for m in layouts:
        li, t1, t4 = int(m.group(2)), f32(m.group(7)), f32(m.group(8))
        script.append((li, 1, 0, t1))
        if t4 != np.float32(-1):
            script.append((li, 3, 0, t4))
            multi[li] = 1
        geometry[li] = dict(visited_slots=int(m.group(5)), blocks_per_cu=int(m.group(6)), cand_slots=int(m.group(9)))
    logged = [(li, v) for li, v, _, _ in script]
    script += [(li, 1, 1, np.float32(0)) for li in range(n_cands) if li not in geometry]
    assert len(set(multi[li] for li in geometry)) == 1 and multi[0] == (1 if nq == 6000 else 0), multi

    def replay(answers):
        li, v, rc, ms = zip(*answers)
        return tournament(n_cands, multi, True, True, li, v, rc, ms)

    winner = replay(script)[1]["layout"]  # (step 1 alone: the variant pass then finds no answers)
    script += [(winner, int(m.group(2)), 0, f32(m.group(3))) for m in variants]
    logged += [(winner, int(m.group(2))) for m in variants]
    trace, result = replay(script)
    asked = [(r[1], r[2]) for r in trace if r[0] == TIME and r[5] == 0]
    assert not result["exhausted"] and result["rc"] == 0 and result["layout"] == winner
    assert asked == logged, "the harness asks for exactly the logged measurements, in order"
    assert all(r[3] == 4 for r in trace if r[0] == TIME)
    duels = [DUEL.match(l) for l in lines if DUEL.match(l)]
    assert [(int(m.group(3)), int(m.group(4)), int(m.group(2)) * (1 if m.group(5) == "challenger" else -1)) for m in duels] == \
        [r[1:4] for r in trace if r[0] == LOG_DUEL]
    assert [int(m.group(2)) for m in variants] == ([0, 1, 2, 3, 4, 5] if multi[winner] else [0, 1])

    # the next search: the layout and the variant the replay landed on, and no exploration
    dev.search(Q, K, EF)
    info, geom = dev.launch_info(), dev.launch_geometry()
    print(info["variant"], geom, "replayed:", winner, geometry[winner], result["final_variant"])
    assert not info["exploratory"]
    assert info["variant_id"] == result["final_variant"]
    if info["variant_id"] != 0:  # (the layout is the merged-beam kernel's: the two-heap kernel reports its own)
        assert {k: geom[k] for k in geometry[winner]} == geometry[winner]
    else:
        assert geom["kernel"] == "two_heaps"


def test_a_pinned_variant_leaves_nothing_to_measure(hipmod, index, monkeypatch, capfd):
    ix, Q = index
    dev = hipmod.DeviceIndex.upload(ix.blob(), ix.node_size, ix.data_size, ix.M, ix.cur_nodes, ix.dtype, ix.metric, ix.dim)
    dev.set_option("sorted_variant", 1)
    assert tune_and_log(dev, Q, monkeypatch, capfd) == []  # the early return: no measurement, not even the settling launches
    dev.search(Q, K, EF)
    assert not dev.launch_info()["exploratory"] and dev.launch_info()["variant_id"] == 1
