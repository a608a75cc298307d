"""kbg_job_fit on the CPU: the unchanged session code on hostsim's simulated
HIP stream (kube-arbitrator_amd/tools/libkbg_hostsim.so) with the host
restatement of the new launcher (tools/hostsim_kernels.cpp), under both
schedules (eager, lazy: tests/test_hostsim_parity.py).

Kernel level: every case of tests/job_fit_cases.py through the probe of that
library against tests/job_fit_ref.py, and the launches the probe refuses.
Session level (tests/job_fit_session.py): the KATs, seeds of the random,
contended, host-port and pod-affinity generators over three action prefixes,
the refusals, a resident session over a churn chain and one structural batch,
the hand-derived walks of tests/golden/kat_job_fit.json and of the hand-built
gang cluster, and the oracle's own allocate of single jobs on that cluster and
on seeded clusters. The expected rows come from the fixture and the oracle's
output, never from the library's getters. Each schedule runs in two children
(tests/job_fit_worker.py) whose only kbg library is the hostsim one. No test
here is marked gpu."""
import json
import os
import subprocess
import sys

import pytest

import job_fit_cases as jc
import job_fit_session as js
import job_fit_worker as jw
from helpers import build_hostsim

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
KERNEL_IDS = ["case/" + n for n in jc.NAMES] + ["reject/" + x[0] for x in jc.illegal_launches()]
ALLOCATE_IDS = ["allocate-hand", "allocate-dev"] + [f"allocate-seed{s}" for s in js.ALLOCATE_SEEDS]
NEEDED = {"two_shapes", "two_on_one_node", "pipeline", "unplaced_then_placed", "ready_within", "not_ready_within",
          "port_pair_on_two_nodes"}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {"kernels": ..., "sessions": ...}}: all children started at once."""
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("job_fit")
    procs = []
    for sched in SCHEDULES:
        env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
        for what in ("kernels", "sessions"):
            out = str(d / f"{sched}.{what}.json")
            procs.append((sched, what, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "job_fit_worker.py"), what, out], env=env)))
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
@pytest.mark.parametrize("case", jw.SESSION_CASES)
def test_session_rows_match_the_reference(results, case, sched):
    rec = results[sched]["sessions"][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", ALLOCATE_IDS)
def test_places_are_the_oracles_allocate(results, case, sched):
    rec = results[sched]["sessions"][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])


@pytest.mark.parametrize("sched", SCHEDULES)
def test_device_shaped_path_launches(results, sched):
    """hostsim counts the launches under `job_fit`, the last counter, after
    `victim_why`: sessions without host ports, pod affinity, a nil Node or a
    colliding pod key launch, the others never do (the host path answers)."""
    res = results[sched]["sessions"]
    assert res["names"][-2:] == ["victim_why", "job_fit"]
    launches = {c: res[c]["launches"] for c in list(jw.SESSION_CASES) + ALLOCATE_IDS}
    assert all(v is not None for v in launches.values()), "no counter named job_fit"
    for case in ["kat_task_why", "gang-dev", "allocate-dev", "resident", "structural"] + [f"contended{s}" for s in jw.SEEDS["contended"]]:
        assert launches[case] > 0, case
    for case in ["kat_job_fit-hand", "gang-hand"] + [f"affinity{s}" for s in jw.SEEDS["affinity"]]:
        assert launches[case] == 0, case


@pytest.mark.parametrize("sched", SCHEDULES)
def test_allocate_cases_say_something(results, sched):
    """From the reference rows alone (the oracle's decisions): the kept set
    shows every feature of NEEDED, and at most a third of the seeds were left
    out (the oracle ends in ref_panic, or pod affinity)."""
    res = results[sched]["sessions"]
    left = [c for c in ALLOCATE_IDS if res[c].get("left_out")]
    assert 3 * len(left) <= len(ALLOCATE_IDS), f"{left} were left out"
    seen = set()
    for c in ALLOCATE_IDS:
        seen |= set(res[c]["seen"] or [])
    assert seen >= NEEDED, f"not shown: {sorted(NEEDED - seen)}"
    assert sum(res[c].get("jobs", 0) for c in ALLOCATE_IDS) >= 20


@pytest.mark.parametrize("sched", SCHEDULES)
def test_session_cases_say_something(results, sched):
    """The expected rows of the prefix cases show walks over two shapes, two
    steps on a node and both outcomes of a gang, and at most a quarter of a
    generator's seeds without pod affinity were left to the invariants."""
    res = results[sched]["sessions"]
    seen = set()
    for c in jw.SESSION_CASES:
        seen |= set(res[c]["seen"] or [])
    assert seen >= {"two_shapes", "two_on_one_node", "ready_within", "not_ready_within"}, seen
    for kind, seeds in jw.SEEDS.items():
        if kind != "affinity":
            skipped = [s for s in seeds if res[f"{kind}{s}"]["skipped"]]
            assert 4 * len(skipped) <= len(seeds), f"{kind}: seeds {skipped} of {seeds} were skipped"
