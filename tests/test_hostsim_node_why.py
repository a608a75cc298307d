"""kbg_node_reasons on the CPU: the unchanged session code on hostsim's
simulated HIP stream (kube-arbitrator_amd/tools/libkbg_hostsim.so) with the
host restatement of the new launchers (tools/hostsim_kernels.cpp), under both
schedules (eager, lazy: tests/test_hostsim_parity.py).

Kernel level: every case of tests/node_why_cases.py through the probe of that
library against tests/node_why_ref.py, and the launches the probe refuses.
Session level (tests/node_why_session.py): the KATs, seeds of the random,
contended, host-port and pod-affinity generators over three action prefixes,
three resident sessions, the refusals and the hand-derived rows of
tests/golden/kat_node_why.json. The expected rows come from the fixture and
the oracle's output, never from the library's getters; every asked point is
also held to kbg_task_reasons' rows of the same session, to the host path and
to the named-node call. hostsim's launch counter says which path answered.
Each schedule runs in two children (tests/node_why_worker.py) whose only kbg
library is the hostsim one. No test here is marked gpu."""
import json
import os
import subprocess
import sys

import pytest

import node_why_cases as nc
import node_why_worker as nw
from helpers import build_hostsim, ensure_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
KERNEL_IDS = ["case/" + n for n in nc.NAMES] + ["reject/" + x[0] for x in nc.illegal_launches()]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {"kernels": ..., "sessions": ...}}: all children started at once."""
    lib = build_hostsim()
    ensure_oracle()  # (built once here: the children would race to build it)
    d = tmp_path_factory.mktemp("node_why")
    procs = []
    for sched in SCHEDULES:
        env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
        for what in ("kernels", "sessions"):
            out = str(d / f"{sched}.{what}.json")
            procs.append((sched, what, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "node_why_worker.py"), what, out], env=env)))
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
@pytest.mark.parametrize("case", nw.SESSION_CASES)
def test_session_rows_match_the_reference(results, case, sched):
    rec = results[sched]["sessions"][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])


@pytest.mark.parametrize("sched", SCHEDULES)
def test_session_cases_say_something(results, sched):
    """The expected rows of the session cases hold every cause the Python
    reference can name (pod cap, selector, host ports, unschedulable, taints,
    fits Idle, short), some asked row has pods of an overused queue under
    cause 6 or 7 (open_idle or open_releasing below its count), and at most a
    third of a generator's seeds were left to the invariants because their
    cycle discards a statement."""
    count = [0] * 10
    for case in nw.SESSION_CASES:
        seen = results[sched]["sessions"][case]["seen"]
        if seen:
            count = [a + b for a, b in zip(count, seen)]
    assert all(count[k] > 0 for k in (0, 1, 2, 3, 4, 6, 8)), count
    assert any(results[sched]["sessions"][case]["differs"] for case in nw.SESSION_CASES)
    for kind, seeds in nw.SEEDS.items():
        skipped = [s for s in seeds if results[sched]["sessions"][f"{kind}{s}"]["skipped"]]
        assert 3 * len(skipped) <= len(seeds), f"{kind}: seeds {skipped} of {seeds} were skipped"


@pytest.mark.parametrize("sched", SCHEDULES)
def test_launch_counter_names_the_path(results, sched):
    """A session without host ports, pod affinity or a nil Node launches once
    per call (its shapes fit one chunk), for all nodes and for one; with
    KBG_HOST_NODE_WHY=1, and on the host-only KAT, nothing is launched."""
    assert results[sched]["sessions"]["launches"] == {"device, all nodes": 1, "device, one node": 1, "forced host": 0,
                                                      "host only": 0}
