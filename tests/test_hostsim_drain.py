"""kbg_node_drain on the CPU: the unchanged session code on hostsim's simulated
HIP stream (kube-arbitrator_amd/tools/libkbg_hostsim.so) with the host
restatement of the new launcher (tools/hostsim_kernels.cpp), under both
schedules (eager, lazy: tests/test_hostsim_parity.py).

Kernel level: every case of tests/drain_cases.py through the probe of that
library against tests/drain_ref.py, and the launches the probe refuses.
Session level (tests/drain_session.py): the KAT fixtures of the other queries,
seeds of the random, contended
and host-port generators, without and with a cordon, seeds of the pod-affinity
generator held to the invariants, to kbg_task_reasons through Pending twins and
to the oracle's allocate of one Pending twin at a time, the refusals, a resident
session over a churn chain and one structural batch, the hand-derived tests/golden/kat_drain.json (host ports,
pod affinity as of now, a nil Node), the hand-worked walks of
the hand-built cluster (a cordon, a BestEffort pod, a gang that breaks and one
that does not, two pods sharing a host port), the Pending-twin check against kbg_task_reasons and the one-target
check against kbg_task_headroom, and, independent of the Python restatement,
the oracle's own allocate of the moved pods on the seeded clusters and the
hand-built one. The expected rows come from the fixture and
the oracle's output, never from the library's getters. Each schedule runs in
two children (tests/drain_worker.py) whose only kbg library is the hostsim one.
No test here is marked gpu."""
import json
import os
import subprocess
import sys

import pytest

import drain_cases as dc
import drain_worker as dw
from helpers import build_hostsim

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
KERNEL_IDS = ["case/" + n for n in dc.NAMES] + ["reject/" + x[0] for x in dc.illegal_launches()]
NEEDED = {"two_shapes", "two_on_one_node", "pipeline", "unplaced_then_placed", "best_effort", "cordon_changed_a_place",
          "jobs_short", "jobs_not_short"}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {"kernels": ..., "sessions": ...}}: all children started at once."""
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("drain")
    procs = []
    for sched in SCHEDULES:
        env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
        for what in ("kernels", "sessions"):
            out = str(d / f"{sched}.{what}.json")
            procs.append((sched, what, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "drain_worker.py"), what, out], env=env)))
    res = {s: {} for s in SCHEDULES}
    failed = []
    for sched, what, out, p in procs:
        if p.wait() != 0:
            failed.append((sched, what, p.returncode))
            continue
        with open(out) as f:
            res[sched][what] = json.load(f)
    assert not failed, f"hostsim children ended with {failed}"
    return res


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", KERNEL_IDS)
def test_hostsim_launcher_matches_the_reference(results, case, sched):
    errs = results[sched]["kernels"][case]
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", dw.SESSION_CASES)
def test_session_rows_match_the_reference(results, case, sched):
    rec = results[sched]["sessions"][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", dw.ALLOCATE_CASES + dw.AFTER_CASES)
def test_places_are_the_oracles_allocate(results, case, sched):
    """The moved pods as Pending pods of one new PodGroup, the drained node and
    the cordon unschedulable: kbref's decisions are the places, on both paths.
    allocate-after-*: the session has run allocate, and the moved pods are the
    node's at open and then those the oracle's own allocate decided onto it,
    in the order of its log."""
    rec = results[sched]["sessions"][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])


@pytest.mark.parametrize("sched", SCHEDULES)
def test_allocate_cases_say_something(results, sched):
    """At most a third of the seeded clusters were left out of the check
    against the oracle's allocate (no walk compared: no predicates plugin, pod
    affinity, only walks with a BestEffort pod, an oracle ref_panic)."""
    res = results[sched]["sessions"]
    seeded = [c for c in dw.ALLOCATE_CASES if c not in ("allocate-hand", "allocate-dev")]
    left = [c for c in seeded if not res[c]["compared"]]
    assert 3 * len(left) <= len(seeded), f"{left} were left out"
    assert sum(res[c]["compared"] or 0 for c in dw.ALLOCATE_CASES) >= 20
    assert res["allocate-hand"]["compared"] and res["allocate-dev"]["compared"]
    after = [c for c in dw.AFTER_CASES if not res[c]["compared"]]
    assert 3 * len(after) <= len(dw.AFTER_CASES), f"{after} were left out"
    assert sum(res[c]["compared"] or 0 for c in dw.AFTER_CASES) >= 20


@pytest.mark.parametrize("sched", SCHEDULES)
def test_device_shaped_path_launches(results, sched):
    """hostsim counts the launches under `drain`, after `node_why`: sessions
    without host ports, pod affinity, a nil Node or a colliding pod key
    launch, the others never do (the host path answers)."""
    res = results[sched]["sessions"]
    assert res["names"].index("drain") == res["names"].index("node_why") + 1
    launches = {c: res[c]["launches"] for c in dw.SESSION_CASES}
    assert all(v is not None for v in launches.values()), "no counter named drain"
    for case in ["kat_task_why", "drain-dev", "drain-hand", "headroom", "resident", "structural"] + \
            [f"contended{s}" for s in dw.SEEDS["contended"]]:
        assert launches[case] > 0, case
    assert launches["kat_drain-hand"] == 0  # a nil Node, pod affinity: the host path
    assert launches["dup-hand"] == 0  # a colliding pod key: the host path
    # pod affinity, and the host-port generator's clusters (pods with a port run on every node): the host path
    for case in [f"{kind}{s}" for kind in ("affinity", "ports") for s in dw.SEEDS[kind]] + \
            ["twin-affinity", "oracle-twin-affinity"]:
        assert launches[case] == 0, case


@pytest.mark.parametrize("sched", SCHEDULES)
def test_session_cases_say_something(results, sched):
    """The expected rows of the prefix cases show, from the fixture and the
    oracle's output alone, every feature of NEEDED, and at most a quarter of a
    generator's seeds without pod affinity were left to the invariants."""
    res = results[sched]["sessions"]
    seen = set()
    for c in dw.SESSION_CASES:
        seen |= set(res[c]["seen"] or [])
    assert seen >= NEEDED, f"not shown: {sorted(NEEDED - seen)}"
    for kind, seeds in dw.SEEDS.items():
        skipped = [s for s in seeds if res[f"{kind}{s}"]["skipped"]]
        if kind != "affinity":  # (the Python reference has no pod-affinity stage: invariants, twins and the KAT)
            assert 4 * len(skipped) <= len(seeds), f"{kind}: seeds {skipped} of {seeds} were skipped"
