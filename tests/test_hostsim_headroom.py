"""kbg_task_headroom on the CPU: the unchanged session code on hostsim's
simulated HIP stream (kube-arbitrator_amd/tools/libkbg_hostsim.so) with the
host restatement of the new launchers (tools/hostsim_kernels.cpp), under both
schedules (eager, lazy: tests/test_hostsim_parity.py).

Kernel level: every case of tests/headroom_cases.py through the probe of that
library against tests/headroom_ref.py, and the launches the probe refuses.
Session level (tests/headroom_session.py): the KATs, seeds of the random,
contended, host-port and pod-affinity generators over three action prefixes,
the refusals, the hand-derived rows of tests/golden/kat_headroom.json and
kat_headroom_dev.json, and three small clusters on which the oracle's own
allocate places identical copies until none fits. The expected rows come from
the fixture and the oracle's output, never from the library's getters.
Each schedule runs in two children (tests/headroom_worker.py) whose only kbg
library is the hostsim one. No test here is marked gpu."""
import json
import os
import subprocess
import sys

import pytest

import headroom_cases as hc
import headroom_ref as hr
import headroom_worker as hw
from helpers import build_hostsim

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
KERNEL_IDS = ["case/" + n for n in hc.NAMES] + ["reject/" + x[0] for x in hc.illegal_launches()]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {"kernels": ..., "sessions": ...}}: all children started at once."""
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("headroom")
    procs = []
    for sched in SCHEDULES:
        env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
        for what in ("kernels", "sessions"):
            out = str(d / f"{sched}.{what}.json")
            procs.append((sched, what, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "headroom_worker.py"), what, out], env=env)))
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
@pytest.mark.parametrize("case", hw.SESSION_CASES)
def test_session_rows_match_the_reference(results, case, sched):
    rec = results[sched]["sessions"][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])


@pytest.mark.parametrize("sched", SCHEDULES)
def test_device_shaped_path_launches(results, sched):
    """hostsim counts the launches under `task_headroom`: sessions without host
    ports, pod affinity or a nil Node launch, the others never do (the host
    path answers the whole table)."""
    launches = {c: results[sched]["sessions"][c]["launches"] for c in hw.SESSION_CASES}
    assert all(v is not None for v in launches.values()), "no counter named task_headroom"
    for case in ["kat_headroom_dev-hand", "kat_task_why"] + [f"allocate-{a}" for a in hw.ALLOCATE]:
        assert launches[case] > 0, case
    for case in ["kat_headroom-hand"] + [f"affinity{s}" for s in hw.SEEDS["affinity"]]:
        assert launches[case] == 0, case


@pytest.mark.parametrize("sched", SCHEDULES)
def test_session_cases_say_something(results, sched):
    """The expected rows of the session cases hold nodes that take copies,
    more than one a node, and nodes past the stages that take none, and at
    most a quarter of a generator's seeds were left to the invariants because
    their cycle discards a statement."""
    seen = [0] * len(hr.KEYS)
    for case in hw.SESSION_CASES:
        s = results[sched]["sessions"][case]["seen"]
        if s:
            seen = [max(a, b) for a, b in zip(seen, s)]
    got = dict(zip(hr.KEYS, seen))
    assert got["copies_idle"] > got["nodes_idle"] > 0 and got["max_node_copies"] > 1, got
    assert got["nodes_pass"] > got["nodes_idle"], got
    for kind, seeds in hw.SEEDS.items():
        skipped = [s for s in seeds if results[sched]["sessions"][f"{kind}{s}"]["skipped"]]
        assert 4 * len(skipped) <= len(seeds), f"{kind}: seeds {skipped} of {seeds} were skipped"
