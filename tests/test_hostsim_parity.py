"""The production session code between the kernels — allocate_cycle
(Predictor thread, committer, Logger / Replayer, epochs), device_launch /
device_wait / device_drop, push_deltas / push_mask_deltas with stage_acquire /
stage_release, the refresh scans polled with hipEventQuery, kbg_session_reset
and kbg_session_update — against the kbref oracle, on the CPU: the unchanged
host sources run on hostsim's simulated HIP stream
(kube-arbitrator_amd/tools/hostsim_hip.cpp) with host launchers
(tools/hostsim_kernels.cpp, held to the kernels' reference by
tests/test_hostsim_kernels.py), under both of its schedules:

  eager — every stream operation runs when it is enqueued;
  lazy  — every operation runs at the last moment HIP allows (an event wait
          runs the stream up to that event's record and no further), so pinned
          staging rewritten before its reader was waited for is read in its
          rewritten state, deterministically.

Each case runs in a child Python whose KBG_LIB_PATH names the hostsim library
(tests/hostsim_worker.py; the cases are dealt over a few children per
schedule); the outputs are compared here with the oracle's (compare_outputs).
Preempt / reclaim are out of scope (the victim launchers are not simulated):
fuzz fixtures that list them run their allocate / backfill actions only, here
and in the oracle. No test here is marked gpu."""
import functools
import glob
import json
import os
import subprocess
import sys

import pytest

import reasons_cases
from helpers import GOLDEN, build_hostsim, churn_chain, compare_outputs, load_golden, run_oracle
from hostsim_worker import make_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
FUZZ = dict(only_allocate_backfill=True)


def fuzz_opts(seed):
    return {"batch_tasks": 1 + seed % 9, "candidates": 1 + seed % 5, "full_scan": seed % 2}


def _kats():
    """The hand-derived KAT sessions whose actions are allocate / backfill."""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "kat_*.json"))):
        with open(p) as f:
            fx = json.load(f)
        if fx.get("kind", "session") == "session" and set(fx.get("actions") or ["allocate"]) <= {"allocate", "backfill"}:
            out.append(os.path.basename(p))
    return out


def _staging_option_sets():
    """The distinct option sets of test_parity_gpu.py test_staging_reuse_under_overlap's 120 iterations."""
    seen = []
    for it in range(120):
        o = {"batch_tasks": 3, "candidates": 4, "full_scan": 1} if it % 2 else \
            {"batch_tasks": 1 + it % 9, "candidates": 1 + it % 5, "full_scan": int(it % 4 == 0)}
        if o not in seen:
            seen.append(o)
    return seen


def _cases():
    c = []
    c += [dict(id=f"ref-{n}", gen="golden", arg=f"ref_allocate_case{n}.json", binds=True) for n in (1, 2)]
    c += [dict(id=k[:-5], gen="golden", arg=k, kat=True) for k in _kats()]
    c += [dict(id=f"config{n}", gen="config", arg=n) for n in (1, 2)]
    c += [dict(id=f"config{n}-gen", gen="config", arg=n, general=1) for n in (1, 2)]
    for o in ({"batch_tasks": 1, "candidates": 1}, {"batch_tasks": 7, "candidates": 2},
              {"batch_tasks": 64, "candidates": 4}, {"batch_tasks": 4096, "candidates": 256},
              {"batch_tasks": 1, "candidates": 1, "full_scan": 1}, {"batch_tasks": 7, "candidates": 2, "full_scan": 1},
              {"batch_tasks": 64, "candidates": 4, "full_scan": 1},
              {"batch_tasks": 2048, "candidates": 32, "full_scan": 1}):  # test_batching_is_exact
        c.append(dict(id="batching-" + "-".join(str(v) for v in o.values()), gen="config", arg=1, opts=o))
    c += [dict(id=f"random{s}", gen="random", arg=s, opts=fuzz_opts(s), **FUZZ) for s in range(100)]
    c += [dict(id=f"random{s}-gen", gen="random", arg=s, opts=fuzz_opts(s), general=1, **FUZZ) for s in range(0, 100, 2)]
    c += [dict(id=f"heaprule{s}", gen="random", arg=1000 + s, kw=dict(max_nodes=6, max_jobs=14, max_tasks=5),
               heap_rule=1, **FUZZ) for s in range(8)]
    c += [dict(id=f"affinity{s}", gen="affinity", arg=s, opts=fuzz_opts(s), **FUZZ) for s in range(100)]
    c += [dict(id=f"backfill{s}", gen="random", arg=2000 + s,
               kw=dict(max_nodes=10, max_jobs=12, max_tasks=12, be_frac=0.6),
               actions=["allocate", "backfill"] if s % 4 else ["backfill"],
               opts={"batch_tasks": 1 + s % 7, "candidates": 1 + s % 3, "full_scan": s % 2}) for s in range(60)]
    c += [dict(id=f"dupkey{s}", gen="dupkey", arg=s, opts=fuzz_opts(s), **FUZZ) for s in range(60)]
    for key, n, rel in (("8193", 8193, False), ("8300", 8300, False), ("8300-releasing", 8300, True)):
        c += [dict(id=f"deep{key}-fs{fs}", gen="deep", arg=n, kw=dict(releasing=rel), opts={"full_scan": fs}, deep=key)
              for fs in (0, 1)]
    c += [dict(id=f"zero-nodes-fs{fs}", gen="config", arg=1, no_nodes=1, opts={"full_scan": fs}, empty=True)
          for fs in (0, 1)]
    c += [dict(id=f"zero-nodes-backfill-fs{fs}", gen="config", arg=1, no_nodes=1, actions=["allocate", "backfill"],
               opts={"full_scan": fs}, empty=True) for fs in (0, 1)]
    c += [dict(id=f"chain-random{s}", gen="chain", base="random", arg=7000 + s, seed=s, rounds=3, opts=fuzz_opts(s),
               **FUZZ) for s in (0, 1, 2, 83)]
    c.append(dict(id="chain-config1", gen="chain", base="config", arg=1, seed=1, rounds=3))
    c += [dict(id="staging-race-" + "-".join(str(v) for v in o.values()), gen="golden", arg="fx_staging_race.json",
               opts=o, **FUZZ) for o in _staging_option_sets()]  # (its allocate, backfill: where the hazard was)
    # sessions opened with kbg_options.reasons (tests/test_reasons_gpu.py's bodies, checked in the child)
    c += [dict(id=f"reasons-{n}", gen="reasons", kind="hand", arg=n) for n in sorted(reasons_cases.CASES)]
    c += [dict(id=f"reasons-{k}{s}", gen="reasons", kind=k, arg=s) for k, s in reasons_cases.DEVICE_SEEDS]
    return c


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
CHILDREN = max(1, min(4, (os.cpu_count() or 2) // 2))  # per schedule


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {case id: the child's record}}: every child of both
    schedules is started at once and waited for here."""
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("hostsim")
    procs = []
    for sched in SCHEDULES:
        for k in range(CHILDREN):
            cases, out = str(d / f"{sched}{k}.cases.json"), str(d / f"{sched}{k}.out.json")
            with open(cases, "w") as f:
                json.dump(CASES[k::CHILDREN], f)
            env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
            env.pop("KBG_FORCE_GENERAL_SCAN", None)
            procs.append((sched, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "hostsim_worker.py"), "parity", cases, out], env=env)))
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


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    """The oracle's output of a case (for a chain: of every round), shared by the schedules."""
    c = BY_ID[case_id]
    if c["gen"] == "reasons":
        return None
    if c["gen"] == "chain":
        fx0 = make_fixture(dict(c, gen=c["base"]))
        return tuple(out for _, _, _, out in churn_chain(fx0, c["seed"], c["rounds"], lambda fx, ch: run_oracle(fx)))
    return run_oracle(make_fixture(c))


def test_library_links_no_gpu_runtime():
    """libkbg_hostsim.so runs the session code without libamdhip64 and librccl."""
    out = subprocess.run(["ldd", build_hostsim()], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" not in out and "librccl" not in out, out
    assert "libstdc++" in out  # (ldd did list the dependencies)


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", [c["id"] for c in CASES])
def test_session_matches_oracle(results, case, sched):
    c, rec = BY_ID[case], results[sched][case]
    assert "error" not in rec, rec["error"]
    if c["gen"] == "reasons":  # (every comparison ran in the child)
        return
    ref = oracle(case)
    if c["gen"] == "chain":
        assert len(rec["chain"]) == len(ref)
        for got_r, ref_r in zip(rec["chain"], ref):
            compare_outputs(ref_r, got_r)
        return
    got = rec["out"]
    compare_outputs(ref, got)
    if "int_scan" in rec and ref["status"] == "ok" and (c.get("general") or c.get("deep")):
        assert rec["int_scan"] == (0 if c.get("general") else 1)
    if c.get("binds"):
        assert got["status"] == "ok" and got["binds"] == load_golden(c["arg"])["expected"]["binds"]
    if c.get("kat"):
        exp = load_golden(c["arg"]).get("expected", {})
        if "decisions" in exp and got["status"] == "ok":
            assert [(d["task"], d["node"], d["kind"]) for d in got["decisions"]] == \
                [tuple(x) for x in exp["decisions"]]
    if c.get("deep"):
        assert ref["status"] == "ok" and len(ref["decisions"]) > 250  # cut and split lists were consumed
    if c.get("empty"):
        assert got["decisions"] == []
