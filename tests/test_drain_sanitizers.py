"""kbg_node_drain under ThreadSanitizer and AddressSanitizer + UBSan, on
hostsim's simulated HIP stream: tools/hostsim_main --drain (a stand-alone
program; the sanitizer runtime is linked into it, nothing is preloaded and no
sanitizer build is loaded into Python) asks the call before the first action
and after each one, for every node without a cordon and for a named subset
under one, on sessions the kernel answers (the call's own predicate classes
compiled, uploaded, used and freed per call) and on sessions the host walk
answers (host ports on a moved pod, pod affinity), under both schedules. Each sanitizer build must end
with status 0, print no report, say what the calls found, and write the bytes
the plain build writes WITHOUT the flag: the call changes nothing.

CPU only and opt-in: skipped unless KBG_HOSTSIM_SANITIZE=1 (the sanitizer
builds of the host sources take a few minutes to compile). Never marked gpu."""
import json
import os
import subprocess
import sys

import pytest

from helpers import ROOT, build_hostsim
from test_hostsim_sanitizers import REPORT, TOOLS

pytestmark = pytest.mark.skipif(os.environ.get("KBG_HOSTSIM_SANITIZE") != "1",
                                reason="set KBG_HOSTSIM_SANITIZE=1 to build and run the sanitizer programs")

HERE = os.path.dirname(os.path.abspath(__file__))
SNAPSHOTS = [
    dict(id="random8", gen="random", arg=8),
    dict(id="contended6", gen="contended", arg=6),
    dict(id="contended-wide56", gen="contended", arg=5056, kw=dict(nodes=150, jobs=20, tasks=8, queues=3)),
    dict(id="victim-affinity100", gen="contended", arg=7100, kw=dict(nodes=12, jobs=14, tasks=8, aff=0.5)),
    dict(id="ports13", gen="contended", arg=13, kw=dict(ports=0.3)),
]


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    lib = build_hostsim()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kube-arbitrator_amd"), "-j", str(min(8, os.cpu_count() or 2)),
                    "hostsim-tsan", "hostsim-asan"], check=True)
    d = tmp_path_factory.mktemp("drain-snapshots")
    cases = str(d / "cases.json")
    with open(cases, "w") as f:
        json.dump(SNAPSHOTS, f)
    subprocess.run([sys.executable, os.path.join(HERE, "hostsim_worker.py"), "snapshots", cases, str(d)], check=True,
                   env=dict(os.environ, KBG_LIB_PATH=lib))
    with open(d / "manifest.json") as f:
        return {m["id"]: (m["path"], m["actions"]) for m in json.load(f)}, d


def replay(program, snapshot, actions, sched, out, ask):
    cmd = [os.path.join(TOOLS, program), snapshot, out, "--schedule", sched, "--actions", ",".join(actions),
           "--repeat", "2"] + (["--drain"] if ask else [])
    env = {k: v for k, v in os.environ.items() if k != "KBG_HOSTSIM_SCHEDULE"}  # (--schedule sets it)
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    with open(out, "rb") as f:
        return p, f.read()


@pytest.mark.parametrize("sched", ["eager", "lazy"])
@pytest.mark.parametrize("snap", [s["id"] for s in SNAPSHOTS])
def test_sanitizer_builds_are_clean(saved, snap, sched):
    table, d = saved
    path, actions = table[snap]
    plain, want = replay("hostsim_main", path, actions, sched, str(d / "plain.bin"), False)
    assert plain.returncode == 0, plain.stderr
    assert len(want) > 16
    for program in ("hostsim_main", "hostsim_main_tsan", "hostsim_main_asan"):
        p, got = replay(program, path, actions, sched, str(d / (program + ".bin")), True)
        assert not any(r in p.stderr for r in REPORT), f"{program}:\n{p.stderr[-6000:]}"
        assert p.returncode == 0, f"{program} ended with {p.returncode}:\n{p.stderr[-3000:]}"
        said = [ln for ln in p.stderr.splitlines() if "node drain after" in ln]
        # two repeats of a cycle and its rerun after a reset: at open and after every action that did not end the list
        assert 8 <= len(said) <= 4 * (len(actions) + 1) and len(said) % 4 == 0, p.stderr[-3000:]
        assert not any("status" in ln for ln in said), p.stderr[-3000:]
        assert any(" 0 pods walked" not in ln for ln in said), p.stderr[-3000:]
        assert got == want, f"{program} --drain wrote other bytes than the plain build without the flag"
