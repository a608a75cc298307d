"""The allocate committer with its dead masks under
ThreadSanitizer and AddressSanitizer + UBSan: tools/hostsim_main_tsan and
tools/hostsim_main_asan (stand-alone programs with the sanitizer runtime
linked in; nothing is preloaded) replay a saved snapshot of the first
saturated session of tests/dead_masks_cases.py — allocate, both schedules,
grouped and --full-scan, batch_tasks=64 — with the masks and with
KBG_DEAD_MASKS=0. Each run must end with status 0, print no report and write
the bytes the plain build writes; with and without the masks the bytes are the
same.

CPU only and opt-in like tests/test_hostsim_sanitizers.py: skipped unless
KBG_HOSTSIM_SANITIZE=1. Never marked gpu."""
import json
import os
import subprocess
import sys

import pytest

import dead_masks_cases as dm
from helpers import ROOT, build_hostsim

pytestmark = pytest.mark.skipif(os.environ.get("KBG_HOSTSIM_SANITIZE") != "1",
                                reason="set KBG_HOSTSIM_SANITIZE=1 to build and run the sanitizer programs")

HERE = os.path.dirname(os.path.abspath(__file__))
TOOLS = os.path.join(ROOT, "kube-arbitrator_amd", "tools")
REPORT = ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "UndefinedBehaviorSanitizer", "runtime error:")


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    lib = build_hostsim()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kube-arbitrator_amd"), "-j", str(min(8, os.cpu_count() or 2)),
                    "hostsim-tsan", "hostsim-asan"], check=True)
    d = tmp_path_factory.mktemp("dead-mask-snapshots")
    cases = str(d / "cases.json")
    with open(cases, "w") as f:
        json.dump(dm.SATURATED[:1], f)
    subprocess.run([sys.executable, os.path.join(HERE, "hostsim_worker.py"), "snapshots", cases, str(d)], check=True,
                   env=dict(os.environ, KBG_LIB_PATH=lib))
    with open(d / "manifest.json") as f:
        return json.load(f)[0]["path"], d


def replay(program, snapshot, sched, full, masks, out):
    cmd = [os.path.join(TOOLS, program), snapshot, out, "--schedule", sched, "--actions", "allocate", "--repeat", "2",
           "--batch-tasks", "64"] + (["--full-scan"] if full else [])
    env = {k: v for k, v in os.environ.items() if k not in ("KBG_HOSTSIM_SCHEDULE", "KBG_DEAD_MASKS")}
    if not masks:
        env["KBG_DEAD_MASKS"] = "0"
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    with open(out, "rb") as f:
        return p, f.read()


@pytest.mark.parametrize("full", [0, 1], ids=["grouped", "full-scan"])
@pytest.mark.parametrize("sched", ["eager", "lazy"])
def test_sanitizer_builds_are_clean(saved, sched, full):
    path, d = saved
    plain, want = replay("hostsim_main", path, sched, full, True, str(d / "plain.bin"))
    assert plain.returncode == 0, plain.stderr
    assert len(want) > 16
    off, want_off = replay("hostsim_main", path, sched, full, False, str(d / "plain_off.bin"))
    assert off.returncode == 0 and want_off == want
    for program in ("hostsim_main_tsan", "hostsim_main_asan"):
        for masks in (True, False):
            p, got = replay(program, path, sched, full, masks, str(d / (program + ".bin")))
            assert not any(r in p.stderr for r in REPORT), f"{program}:\n{p.stderr[-6000:]}"
            assert p.returncode == 0, f"{program} ended with {p.returncode}:\n{p.stderr[-3000:]}"
            assert got == want, f"{program} wrote other bytes than the plain build"
