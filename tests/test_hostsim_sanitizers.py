"""The session code under ThreadSanitizer and AddressSanitizer + UBSan, on
hostsim's simulated HIP stream: tools/hostsim_main (a stand-alone program; the
sanitizer runtime is linked into it — nothing is preloaded and no sanitizer
build is loaded into Python) replays saved snapshots of sessions whose
allocate is contended — the Predictor thread runs beside the committer, lists
are cut, staging is reused — and of contended sessions under their own reclaim
/ preempt action lists (kbg_victims.ipp: the inline and the staged prep, the
kept stop maps, host_stop on huge nodes, discarded statements, class masks
following pod affinity and host ports), under both schedules and three batch
sizes. Each sanitizer build must end with status 0, print no report, and write
the bytes the plain build writes (decision log with its actions, eviction log
and node state of the cycle and of its repeat after kbg_session_reset).

CPU only and opt-in: skipped unless KBG_HOSTSIM_SANITIZE=1 (the sanitizer
builds of the host sources take a few minutes to compile). Never marked gpu."""
import json
import os
import subprocess
import sys

import pytest

from helpers import ROOT, build_hostsim

pytestmark = pytest.mark.skipif(os.environ.get("KBG_HOSTSIM_SANITIZE") != "1",
                                reason="set KBG_HOSTSIM_SANITIZE=1 to build and run the sanitizer programs")

HERE = os.path.dirname(os.path.abspath(__file__))
TOOLS = os.path.join(ROOT, "kube-arbitrator_amd", "tools")
FUZZ = dict(only_allocate_backfill=True)
SNAPSHOTS = [
    dict(id="saturated", gen="saturated", kw=dict(nodes=64, jobs=40, tasks_per_job=12)),
    dict(id="random27", gen="random", arg=27, **FUZZ),
    dict(id="random33", gen="random", arg=33, **FUZZ),
    dict(id="random38", gen="random", arg=38, **FUZZ),
    dict(id="affinity27", gen="affinity", arg=27, **FUZZ),
    dict(id="staging-race", gen="golden", arg="fx_staging_race.json", **FUZZ),
    dict(id="deep8193", gen="deep", arg=8193),
    # reclaim / preempt with the fixtures' own action lists (tests/test_hostsim_parity.py's victim cases)
    dict(id="contended115", gen="contended", arg=115),
    dict(id="contended-large56", gen="contended", arg=5056, kw=dict(nodes=40, jobs=30, tasks=10, queues=3)),
    dict(id="victim-affinity100", gen="contended", arg=7100, kw=dict(nodes=12, jobs=14, tasks=8, aff=0.5)),
    dict(id="victim-ports62", gen="contended", arg=8062, kw=dict(nodes=12, jobs=14, tasks=8, ports=0.4)),
    dict(id="victim-huge5", gen="contended", arg=9505, kw=dict(big=True, huge=True, nodes=2, jobs=240, tasks=30)),
    dict(id="staged-rows", gen="staged_rows"),  # (batch1 / batch3: the staged prep in several chunks)
]
REPORT = ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "UndefinedBehaviorSanitizer", "runtime error:")


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """{id: (snapshot path, actions)}: saved by a child Python through the plain hostsim library."""
    lib = build_hostsim()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kube-arbitrator_amd"), "-j", str(min(8, os.cpu_count() or 2)),
                    "hostsim-tsan", "hostsim-asan"], check=True)
    d = tmp_path_factory.mktemp("hostsim-snapshots")
    cases = str(d / "cases.json")
    with open(cases, "w") as f:
        json.dump(SNAPSHOTS, f)
    subprocess.run([sys.executable, os.path.join(HERE, "hostsim_worker.py"), "snapshots", cases, str(d)], check=True,
                   env=dict(os.environ, KBG_LIB_PATH=lib))
    with open(d / "manifest.json") as f:
        return {m["id"]: (m["path"], m["actions"]) for m in json.load(f)}, d


def replay(program, snapshot, actions, sched, batch, out):
    cmd = [os.path.join(TOOLS, program), snapshot, out, "--schedule", sched, "--actions", ",".join(actions),
           "--repeat", "2"]
    if batch:
        cmd += ["--batch-tasks", str(batch)]
    env = {k: v for k, v in os.environ.items() if k != "KBG_HOSTSIM_SCHEDULE"}  # (--schedule sets it)
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    with open(out, "rb") as f:
        return p, f.read()


@pytest.mark.parametrize("batch", [1, 3, 0], ids=["batch1", "batch3", "default"])
@pytest.mark.parametrize("sched", ["eager", "lazy"])
@pytest.mark.parametrize("snap", [s["id"] for s in SNAPSHOTS])
def test_sanitizer_builds_are_clean(saved, snap, sched, batch):
    table, d = saved
    path, actions = table[snap]
    plain, want = replay("hostsim_main", path, actions, sched, batch, str(d / "plain.bin"))
    assert plain.returncode == 0, plain.stderr
    assert len(want) > 16  # (statuses, a decision count and the nodes' states at least)
    for program in ("hostsim_main_tsan", "hostsim_main_asan"):
        p, got = replay(program, path, actions, sched, batch, str(d / (program + ".bin")))
        assert not any(r in p.stderr for r in REPORT), f"{program}:\n{p.stderr[-6000:]}"
        assert p.returncode == 0, f"{program} ended with {p.returncode}:\n{p.stderr[-3000:]}"
        assert got == want, f"{program} wrote other bytes than the plain build"
