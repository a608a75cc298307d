"""Queue and job names that return to a resident session, on the production
session code over hostsim's simulated HIP stream (CPU only, both schedules;
tests/test_hostsim_parity.py describes them): kbg_session_update's precheck,
the names the session keeps through restructure(), kbg_session_reset and its
cycles, and the wrapper's own record kept by Session._accept. The bodies are
tests/revival_session.py, run in child Pythons whose KBG_LIB_PATH names the
hostsim library (tests/hostsim_worker.py, mode "revival"): the hand-made
cases, the whole generated seed list, the raw-ABI cases over two updates and
the refused batch that must leave nothing recorded. No test here is marked gpu."""
import json
import os
import subprocess
import sys

import pytest

from helpers import build_hostsim
from revival_cases import CASES, EXPECT, SEEDS
from revival_session import SPECIALS

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")


def _opts(seed):
    return {"batch_tasks": 1 + seed % 7, "full_scan": seed % 2}


RUNS = [dict(id=f"case-{c}", kind="case", arg=c) for c in sorted(CASES)] + \
       [dict(id=f"seed{s}", kind="seed", arg=s, opts=_opts(s)) for s in SEEDS] + \
       [dict(id=s, kind="special", arg=s) for s in sorted(SPECIALS)]
BY_ID = {c["id"]: c for c in RUNS}
CHILDREN = max(1, min(4, (os.cpu_count() or 2) // 2))  # per schedule


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("revival")
    procs = []
    for sched in SCHEDULES:
        for k in range(CHILDREN):
            cases, out = str(d / f"{sched}{k}.cases.json"), str(d / f"{sched}{k}.out.json")
            with open(cases, "w") as f:
                json.dump(RUNS[k::CHILDREN], f)
            env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
            env.pop("KBG_FORCE_GENERAL_SCAN", None)
            procs.append((sched, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "hostsim_worker.py"), "revival", cases, out], env=env)))
    res = {s: {} for s in SCHEDULES}
    failed = []
    for sched, out, p in procs:
        if p.wait() != 0:
            failed.append((sched, p.returncode))
            continue
        with open(out) as f:
            res[sched].update(json.load(f))
    assert not failed, f"hostsim children ended with {failed}"
    return res


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("run", [c["id"] for c in RUNS])
def test_revival_on_the_simulated_stream(results, run, sched):
    rec = results[sched][run]
    assert "error" not in rec, rec["error"]
    c = BY_ID[run]
    if c["kind"] == "case":  # the session went the way the case's verdict is written out
        assert rec["refused"] == ([] if EXPECT[c["arg"]] is None else [EXPECT[c["arg"]][0]])
