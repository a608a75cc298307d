"""The in-order commit's dead masks (kbg_svc_link.ipp dead_update,
Resolver::resolve_mask) on hostsim, CPU only: every case of
tests/dead_masks_cases.py runs in a child Python on
kube-arbitrator_amd/tools/libkbg_hostsim.so, in production and full-scan mode
with batch_tasks=64, under both schedules, once with the masks and once with
KBG_DEAD_MASKS=0. Status, decision log, binds and every job, queue and node
state must be equal with and without, and equal to the kbref oracle's. On the
saturated sessions the masks must at least halve the re-checks, so the
comparison cannot pass with the masks inert; the hand-made session must have
met the edges it was made for. No test here is marked gpu."""
import functools
import json
import os
import subprocess
import sys

import pytest

import dead_masks_cases as dm
from helpers import build_hostsim, compare_outputs, run_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
BY_ID = {c["id"]: c for c in dm.HOST_CASES}
CHILDREN = max(1, min(4, (os.cpu_count() or 2) // 2))  # per schedule


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {case id: {"on": record, "off": record}}}"""
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("dead-masks")
    procs = []
    for sched in SCHEDULES:
        for k in range(CHILDREN):
            cases, out = str(d / f"{sched}{k}.cases.json"), str(d / f"{sched}{k}.out.json")
            with open(cases, "w") as f:
                json.dump(dm.HOST_CASES[k::CHILDREN], f)
            env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
            for k2 in ("KBG_FORCE_GENERAL_SCAN", "KBG_DEAD_MASKS"):
                env.pop(k2, None)
            procs.append((sched, out, subprocess.Popen(
                [sys.executable, os.path.join(HERE, "dead_masks_cases.py"), cases, out], env=env)))
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
    return run_oracle(dm.make_fixture(BY_ID[case_id]))


def check_edges(out):
    """The hand-made session met its edges (dead_masks_cases.edges_fixture)."""
    assert out["status"] == "ok"
    nodes = out["nodes"]
    for dim, tol in enumerate((10.0, 10.0 * 1024 * 1024, 10.0)):  # a request placed on Idle short by less than the tolerance
        assert any(-tol < n["idle"][dim] < 0 for n in nodes), dim
    by_job = {}
    for d in out["decisions"]:
        by_job.setdefault(d["job"], []).append(d)
    assert any(d["kind"] == "pipeline" for d in by_job["ns/pipe"])  # Idle short, Releasing fits
    assert len(by_job["ns/zero-mem"]) == 20 and len(by_job["ns/zero-cpu"]) == 16  # a zero request in a dimension
    assert [d.get("action") for d in by_job["ns/best-effort"]] == ["backfill"] * 6
    capped = [nodes[1], nodes[21], nodes[len(nodes) - 2]]
    assert all(n["ntasks"] == 2 for n in capped), capped
    # ... full by pod count alone: room is left for a task of `small`, which ran out of nodes
    assert any(n["idle"][0] >= 250 and n["idle"][1] >= 256 * 2 ** 20 for n in capped), capped
    assert 0 < len(by_job["ns/small"]) < 160
    assert nodes[-1]["ntasks"] > 1  # the node at the word edge took tasks


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", [c["id"] for c in dm.HOST_CASES])
def test_masks_change_no_output(results, case, sched):
    rec = results[sched][case]
    on, off = rec["on"], rec["off"]
    assert "error" not in on and "error" not in off, (on.get("error"), off.get("error"))
    assert on["out"] == off["out"]  # status, decisions, binds, evictions, job / queue / node states
    compare_outputs(oracle(case), on["out"])
    if case.startswith("edges"):
        check_edges(on["out"])
    if case.startswith("affinity"):  # (the allocate under pod affinity evaluated a session's worth of tasks)
        assert on["out"]["status"] == "ok" and on["stats"]["task_evaluations"] >= 20


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", [c["id"] for c in dm.with_modes(dm.SATURATED)])
def test_masks_halve_the_rechecks(results, case, sched):
    """Measured at the default schedule: 3164 -> 555 (production) and 3723 ->
    426 (full-scan) on the first session, 2025 -> 327 and 1579 -> 242 on the
    second; batch boundaries depend on thread timing, hence the margin."""
    on, off = results[sched][case]["on"]["stats"], results[sched][case]["off"]["stats"]
    print(case, sched, "re-checks", off["resolve_rechecks"], "->", on["resolve_rechecks"])
    assert off["resolve_rechecks"] > 0, (on, off)  # (how many depends on how often a scan overlapped a commit)
    assert on["resolve_rechecks"] <= 0.5 * off["resolve_rechecks"], (on, off)
    assert on["task_evaluations"] == off["task_evaluations"], (on, off)
