"""kbg_victim_reasons on the CPU: the unchanged session code on hostsim's
simulated HIP stream (kube-arbitrator_amd/tools/libkbg_hostsim.so) with the
host restatement of the two new launchers (tools/hostsim_kernels.cpp), under
both schedules (eager, lazy: tests/test_hostsim_parity.py).

Kernel level: every case of tests/victim_why_cases.py through the probe of
that library against tests/victim_why_ref.py. Session level
(tests/victim_why_session.py): kat_reclaim and kat_preempt, seeds of the
contended generators tests/test_parity_gpu.py uses, a resident session
updated between cycles, a node of 1025 Running candidates, each fixture's twin
that takes the host path (one more pod with a host port nothing conflicts
with), the refusals, and seeds whose cycle discards a statement after
evicting, where the device-shaped path is held to host_why on the same
session (KBG_HOST_VICTIM_WHY). The expected rows come from the fixture, the Python
cache mirror and the oracle's output of the same actions, never from the
library's getters; the cycle with the calls in between must end as the
oracle's. Each schedule runs in two children (tests/victim_why_worker.py)
whose only kbg library is the hostsim one. No test here is marked gpu."""
import json
import os
import subprocess
import sys

import pytest

import victim_why_cases as wc
import victim_why_worker as ww
from helpers import build_hostsim

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
KERNEL_IDS = ["case/" + n for n in wc.NAMES] + ["reject/" + x[0] for x in ww.illegal_launches()]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {"kernels": ..., "sessions": ...}}: all children started at once."""
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("victim_why")
    procs = []
    for sched in SCHEDULES:
        env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
        for what in ("kernels", "sessions"):
            out = str(d / f"{sched}.{what}.json")
            procs.append((sched, what, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "victim_why_worker.py"), what, out], env=env)))
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
def test_hostsim_launchers_match_the_reference(results, case, sched):
    errs = results[sched]["kernels"][case]
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", ww.SESSION_CASES)
def test_session_rows_match_the_reference(results, case, sched):
    rec = results[sched]["sessions"][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])


@pytest.mark.parametrize("sched", SCHEDULES)
def test_session_cases_say_something(results, sched):
    """The reference rows of the session cases hold pod-cap and selector
    nodes, nodes without preemptees, without victims (each fn empty somewhere)
    and with victims: a green comparison of empty rows would prove little."""
    count, fn = [0] * 11, [0, 0, 0]
    for case in ww.SESSION_CASES:
        seen = results[sched]["sessions"][case]["seen"]
        if seen and not case.startswith("discard"):  # (those sum the library's rows, not the reference's)
            count = [a + b for a, b in zip(count, seen["count"])]
            fn = [a + b for a, b in zip(fn, seen["fn_empty"])]
    assert all(count[k] for k in (0, 1, 6, 7, 9)) and all(fn), (count, fn)
    huge = results[sched]["sessions"]["huge"]["seen"]
    assert huge and sum(huge["count"]) > 0
