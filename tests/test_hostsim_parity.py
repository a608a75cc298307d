"""The production session code between the kernels — allocate_cycle
(Predictor thread, committer, Logger / Replayer, epochs), device_launch /
device_wait / device_drop, push_deltas / push_mask_deltas with stage_acquire /
stage_release, the refresh scans polled with hipEventQuery, kbg_session_reset
and kbg_session_update, and the preempt / reclaim path of kbg_victims.ipp
(victim_push's inline and staged prep, vt_setup, the stop maps VictimCache
keeps across tries, host_stop, statements and their discard) — against the
kbref oracle, on the CPU: the unchanged
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
schedule); the outputs are compared here with the oracle's (compare_outputs:
decisions, pipelines, evictions, shares, node state). The older fuzz cases
keep running the allocate / backfill actions of their fixtures only
(only_allocate_backfill), here and in the oracle; the victim cases below them
run their fixtures' own action lists, reclaim and preempt included.
test_victim_cases_reach_the_code asserts from hostsim's launch counters and
kbg_stats that those cases left the inline prep. Sharded victim scans (the
allreduce of device words) are not simulated. No test here is marked gpu."""
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
from test_parity_gpu import DUP_DISCARD_SEEDS

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
FUZZ = dict(only_allocate_backfill=True)


def fuzz_opts(seed):
    return {"batch_tasks": 1 + seed % 9, "candidates": 1 + seed % 5, "full_scan": seed % 2}


VICTIM_ACTIONS = ["reclaim", "allocate", "backfill", "preempt"]


def _kats(victim=False):
    """The hand-derived KAT sessions whose actions are allocate / backfill, or
    (victim) those whose actions include reclaim or preempt."""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "kat_*.json"))):
        with open(p) as f:
            fx = json.load(f)
        plain = set(fx.get("actions") or ["allocate"]) <= {"allocate", "backfill"}
        if fx.get("kind", "session") == "session" and plain != victim:
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


def _victim_cases():
    """Sessions with their reclaim / preempt actions intact (`victim` names the
    family): the KATs that list them, the reference / config / zero-node
    sessions under all four actions, seeds spread over the ranges of
    tests/test_parity_gpu.py's contended generators, and resident sessions
    updated between contended cycles."""
    c = []
    c += [dict(id=k[:-5], gen="golden", arg=k, kat=True, victim="kat") for k in _kats(victim=True)]
    c += [dict(id=f"ref-{n}-victim", gen="golden", arg=f"ref_allocate_case{n}.json", actions=VICTIM_ACTIONS,
               victim="plain") for n in (1, 2)]
    c += [dict(id=f"config{n}-victim", gen="config", arg=n, actions=VICTIM_ACTIONS, victim="plain") for n in (1, 2)]
    c += [dict(id=f"zero-nodes-victim-fs{fs}", gen="config", arg=1, no_nodes=1, actions=VICTIM_ACTIONS,
               opts={"full_scan": fs}, empty=True, victim="plain") for fs in (0, 1)]
    # test_contended_reclaim_preempt_parity (seeds 0..149)
    c += [dict(id=f"contended{s}", gen="contended", arg=s, opts=fuzz_opts(s), victim="contended")
          for s in range(1, 150, 3)]
    # test_contended_large_parity (0..59): 40 nodes, 30 jobs, many tries per preemptor shape
    c += [dict(id=f"contended-large{s}", gen="contended", arg=5000 + s, kw=dict(nodes=40, jobs=30, tasks=10, queues=3),
               opts=fuzz_opts(s), victim="large") for s in range(2, 60, 3)]
    # test_victim_affinity_parity (0..119), test_victim_host_ports_parity (0..99)
    c += [dict(id=f"victim-affinity{s}", gen="contended", arg=7000 + s, kw=dict(nodes=12, jobs=14, tasks=8, aff=0.5),
               opts=fuzz_opts(s), victim="affinity") for s in range(1, 120, 3)]
    c += [dict(id=f"victim-ports{s}", gen="contended", arg=8000 + s, kw=dict(nodes=12, jobs=14, tasks=8, ports=0.4),
               opts=fuzz_opts(s), victim="ports") for s in range(2, 100, 3)]
    # test_dupkey_statement_discard_parity: every seed whose oracle run discards such a statement
    c += [dict(id=f"dupkey-discard{s}", gen="contended_dupkey", arg=s, opts=fuzz_opts(s), dup_discards=True,
               victim="dupkey-discard") for s in DUP_DISCARD_SEEDS]
    # test_dupkey_fuzz_parity (0..199) with the fixtures' own action lists
    c += [dict(id=f"dupkey-victim{s}", gen="dupkey", arg=s, opts=fuzz_opts(s), victim="dupkey")
          for s in range(3, 200, 7)]
    # test_victim_big_node_parity (0..11), test_victim_huge_node_parity (0..9), test_config5_scaled_parity
    c += [dict(id=f"victim-big{s}", gen="contended", arg=9000 + s, kw=dict(big=True, nodes=2, jobs=50, tasks=24),
               opts=fuzz_opts(s), victim="big") for s in (4, 9)]
    c += [dict(id=f"victim-huge{s}", gen="contended", arg=9500 + s,
               kw=dict(big=True, huge=True, nodes=2, jobs=240, tasks=30), opts=fuzz_opts(s), victim="huge")
          for s in (1, 5, 8)]
    c.append(dict(id="config5-300", gen="contended_config", kw=dict(nodes=300, jobs=120, pending_jobs=8),
                  evicts=True, victim="config5"))
    # the staged prep in several chunks of batch_tasks rows: the tries of one preemptor shape are answered
    # from the kept stop maps, so the next shape's victim_push holds every node they touched. Under the
    # default batch (config5-300) the rows go up in one chunk. staged-rows is hand-built so that a chunk
    # lost to a rewritten staging buffer changes the next scan's answer (hostsim_worker.staged_rows_fixture)
    c.append(dict(id="config5-300-batch4", gen="contended_config", kw=dict(nodes=300, jobs=120, pending_jobs=8),
                  opts={"batch_tasks": 4}, evicts=True, victim="config5"))
    c.append(dict(id="config5-100-batch1-fs", gen="contended_config", kw=dict(nodes=100, jobs=40, pending_jobs=4),
                  opts={"batch_tasks": 1, "candidates": 2, "full_scan": 1}, evicts=True, victim="config5"))
    c += [dict(id="staged-rows-" + "-".join(str(v) for v in o.values()), gen="staged_rows", opts=o, evicts=True,
               victim="staged") for o in ({"batch_tasks": 4}, {"batch_tasks": 3, "candidates": 2, "full_scan": 1})]
    # resident sessions over churn rounds on contended bases: the victim tables are rebuilt after
    # every kbg_session_update (vt_stale) and the kept stop maps dropped
    c += [dict(id=f"chain-contended{s}", gen="chain", base="contended", arg=s, kw=kw, actions=VICTIM_ACTIONS, seed=s,
               rounds=3, opts=fuzz_opts(s), victim="chain")
          for s, kw in ((4, {}), (5013, dict(nodes=40, jobs=30, tasks=10, queues=3)),
                        (7031, dict(nodes=12, jobs=14, tasks=8, aff=0.5)),
                        (8047, dict(nodes=12, jobs=14, tasks=8, ports=0.4)))]
    return c


CASES = _cases() + _victim_cases()
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
    if c.get("dup_discards"):
        assert ref["stats"]["dup_discards"] > 0
    if c.get("evicts"):
        assert ref["status"] == "ok" and ref["evictions"], ref.get("error")
    if c.get("victim") == "huge":  # host_stop took the nodes past kMaxNodeCandidates
        assert got["status"] != "unsupported", got.get("error")
    if c.get("victim") == "staged":  # (what the fixture is built for)
        assert rec["launches"].get("victim_prep_next_chunk", 0) > 0 and rec["stats"]["victim_scans"] == 2


# What a session must have done for a reach condition to count, from the
# child's record of it: hostsim's launch counters (tools/hostsim_kernels.cpp,
# `n`) and the victim counters of kbg_stats (`st`). Behind each, the cases
# that reach it as the generators stand.
REACH = {
    # launch_victim_prep_inline with nn > 0, with ns > 0: most contended sessions (contended*,
    # victim-affinity*, victim-ports*, chain-contended*: a try evicted a few tasks on one node)
    "inline prep carrying node rows": lambda n, st: n.get("victim_prep_inline_nodes", 0) > 0,
    "inline prep carrying state deltas": lambda n, st: n.get("victim_prep_inline_state", 0) > 0,
    # launch_victim_prep: config5-300 (hundreds of tries on kept maps, then every touched row in one
    # chunk), config2-victim (allocate changed more than 48 table entries before preempt), victim-huge5
    "staged prep": lambda n, st: n.get("victim_prep", 0) > 0,
    # ... twice within one victim_push: config5-300-batch4, config5-100-batch1-fs, staged-rows-*
    "staged prep in more than one chunk": lambda n, st: n.get("victim_prep_next_chunk", 0) > 0,
    # launch_victim_big with row_out: victim-big4, victim-big9 (nodes of 130-250 Running pods)
    "big-node launch with row_out": lambda n, st: n.get("victim_big_row_out", 0) > 0,
    # victim_tries > victim_scans: config5-*, staged-rows-*, victim-huge*, contended-large*
    "a try answered from kept stop maps": lambda n, st: st.get("victim_tries", 0) > st.get("victim_scans", 0),
    # victim_host_evals > 0: victim-huge* (nodes never scanned on the device), config5-*, staged-rows-*
    # (nodes touched since the scan)
    "host_stop evaluations": lambda n, st: st.get("victim_host_evals", 0) > 0,
}


@pytest.mark.parametrize("sched", SCHEDULES)
def test_victim_cases_reach_the_code(results, sched):
    """A green run that never left the inline prep proves little: over the
    victim cases, per schedule, every path of victim_push and try_task ran in
    at least one session that ended without an error (each is compared with
    the oracle by test_session_matches_oracle)."""
    ran = {c["id"]: results[sched][c["id"]] for c in CASES if c.get("victim")}
    ran = {i: r for i, r in ran.items() if "error" not in r}
    missing = [what for what, reached in REACH.items()
               if not any(reached(r.get("launches", {}), r.get("stats", {})) for r in ran.values())]
    assert not missing, missing
    # a huge-node session that ended without KBG_E_UNSUPPORTED, its huge nodes evaluated by host_stop
    huge = [r for i, r in ran.items() if BY_ID[i]["victim"] == "huge"]
    assert huge and all(r["out"]["status"] in ("ok", "ref_panic") for r in huge)
    assert any(r["stats"]["victim_host_evals"] > 0 for r in huge)
