"""The seven query calls on sessions after update events, on the CPU: the
unchanged session code on hostsim's simulated HIP stream
(kube-arbitrator_amd/tools/libkbg_hostsim.so), under both schedules (eager,
lazy: tests/test_hostsim_parity.py). Every case of
tests/query_update_cases.py runs tests/query_update_session.py's check_rounds
in a child (tests/query_update_worker.py) whose only kbg library is the
hostsim one: a session is asked, updated and asked again, every point asks
all seven calls of the one session in an order that rotates with the point, and
is compared with a fresh session on the replayed cache and with the references
of tests/query_update_ref.py on the fixture after the events and the oracle's
output. hostsim's launch counters, read around the updated session's own
calls, say which path answered. No test here is marked gpu; no case may be
skipped."""
import json
import os
import subprocess
import sys

import pytest

import query_update_cases as qc
from helpers import build_hostsim

HERE = os.path.dirname(os.path.abspath(__file__))
SCHEDULES = ("eager", "lazy")
CASES = sorted(qc.all_cases())


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{schedule: {case: record}}: both children started at once."""
    lib = build_hostsim()
    d = tmp_path_factory.mktemp("query_update")
    procs = []
    for sched in SCHEDULES:
        env = dict(os.environ, KBG_LIB_PATH=lib, KBG_HOSTSIM_SCHEDULE=sched)
        out = str(d / f"{sched}.json")
        procs.append((sched, out, subprocess.Popen([sys.executable, os.path.join(HERE, "query_update_worker.py"), out],
                                                   env=env)))
    res, failed = {}, []
    for sched, out, p in procs:
        if p.wait() != 0:
            failed.append((sched, p.returncode))
            continue
        with open(out) as f:
            res[sched] = json.load(f)
    assert not failed, f"hostsim children ended with {failed}"
    return res


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", CASES)
def test_queries_after_update(results, case, sched):
    rec = results[sched][case]
    assert not rec["errors"], "\n".join(rec["errors"][:20])
    assert rec["skipped"] is None, f"a committed case was skipped: {rec['skipped']}"
    assert rec["ref"], "no fixture says the cache after the events: the references were not compared"
    print(f"{case}: {rec['rows']} rows against the fresh session, {rec['rows_ref']} against the references")
    assert rec["rows"] > 0 and rec["rows_ref"] > 0, rec
    assert min(rec["answered"]) > 0, f"a point without a Pending task: {rec['answered']}"
    # kbg_job_fit, kbg_node_reasons and kbg_node_drain were each held to their references; the walks' reference
    # has no pod-affinity stage, so on such fixtures kbg_node_reasons alone is
    for what in ("node",) if any(rec["pod_affinity"]) else ("fit", "node", "drain"):
        assert rec["rows_ref_by"].get(what, 0) > 0, (what, rec["rows_ref_by"])
    # (that the update is visible to the calls is tests/test_query_update_ref.py's, from the references)


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", CASES)
def test_device_shaped_path_answers_after_the_update(results, case, sched):
    """Without host ports, pod affinity or a nil Node the updated session's
    calls launch the task-reasons, headroom, victim-reasons, job-fit,
    node-reasons and drain kernels, and every update that rebuilt the session
    builds the stage planes again before its first answer. The drain kernel
    takes a walk only where it holds a pod without a host port (the others go
    to the host walk), so a case counts for it only if some walk after an
    update held such a pod."""
    rec = results[sched][case]
    for r, n in enumerate(rec["rebuilds"]):
        if n:
            assert rec["stage_mask"][r] > 0, f"round {r} rebuilt the session and no stage plane was built: {rec}"
    if not any(rec["host_only"]):
        for name in ("task_why", "task_headroom", "victim_why", "job_fit", "node_why"):
            assert rec["launches"].get(name, 0) > 0, (name, rec["launches"])
        if any(rec["drain_plain_walk"]):
            assert rec["launches"].get("drain", 0) > 0, rec["launches"]
        assert sum(rec["stage_mask"]) > 0 or not any(rec["rebuilds"])


@pytest.mark.parametrize("sched", SCHEDULES)
def test_new_class_makes_the_planes_larger(results, sched):
    """Pending pods with a spec only Running pods had: the update recompiles
    the static predicate with one more class, and the stage planes, whose size
    follows the classes, are built again before the first answer."""
    rec = results[sched]["structural/pod_group_add_new_class"]
    before, after = rec["n_classes"]
    assert after > before, rec["n_classes"]
    assert rec["stage_mask"][0] > 0 and not rec["host_only"][0], rec
    for case, other in results[sched].items():
        if case.startswith(("in_place/", "recompile/")):
            assert len(set(other["n_classes"])) == 1, (case, other["n_classes"])


@pytest.mark.parametrize("sched", SCHEDULES)
def test_entry_point_of_one_update(results, sched):
    """check_queries_after_update, the one-update form of check_rounds, on a relabel."""
    assert results[sched]["entry/relabel_hand"] == [], results[sched]["entry/relabel_hand"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_families_take_the_paths_they_are_named_for(results, sched):
    """Structural and recompile cases rebuild the session, in-place cases do
    not; some in-place batch leaves the old task numbers in place (compared by
    uid only); the staged case's warm-up cycle evicted; every family has a
    case the kernels answered."""
    recs = results[sched]
    cases = qc.all_cases()
    assert set(recs) == set(cases) | {"entry/relabel_hand"}
    for case, (fam, _) in cases.items():
        if fam in ("structural", "recompile"):
            assert all(recs[case]["rebuilds"]), (case, recs[case]["rebuilds"])
        if fam == "in_place" and case.split("/")[1] in qc.ue.IN_PLACE + ("regrow_keys",):
            assert not any(recs[case]["rebuilds"]), (case, recs[case]["rebuilds"])
    assert any(any(recs[c]["by_uid_only"]) for c, (fam, _) in cases.items() if fam == "in_place")
    assert recs["in_place/staged_after_preempt"]["evicted0"] > 0
    for fam in ("structural", "in_place", "recompile", "chain"):
        assert any(not any(recs[c]["host_only"]) for c, (f, _) in cases.items() if f == fam), fam


# Whether a family's updates rebuild the session: every structural and recompile batch does
# (test_families_take_the_paths_they_are_named_for), no JOB_UPDATE / QUEUE_SET or pod-churn batch does, and a
# chain goes through both kinds on one session.
REBUILDS = {"structural": (True,), "recompile": (True,), "in_place": (False,), "chain": (True, False)}


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("family", sorted(REBUILDS))
def test_new_kernels_answer_after_both_kinds_of_update(results, family, sched):
    """From the records: in every family, for each kind of update it holds
    (one that rebuilt the session, one that did not), some case has a round of
    that kind after which the job-fit, node-reasons and drain kernels each
    launched for the updated session's own calls (the drain kernel's round
    must have walked a pod without a host port)."""
    cases = qc.all_cases()
    for rebuilt in REBUILDS[family]:
        seen = set()
        for case, (fam, _) in cases.items():
            rec = results[sched][case]
            if fam != family or rec["skipped"]:
                continue
            for r, n in enumerate(rec["rebuilds"]):
                if bool(n) != rebuilt or rec["host_only"][r]:
                    continue
                got = rec["round_launches"][r]
                seen |= {name for name in ("job_fit", "node_why") if got.get(name, 0) > 0}
                if rec["drain_plain_walk"][r] and got.get("drain", 0) > 0:
                    seen.add("drain")
        assert seen == {"job_fit", "node_why", "drain"}, (family, rebuilt, seen)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_every_call_is_the_first_asked_after_some_update(results, sched):
    """The cases of a family start the rotation of the seven calls at
    different calls (tests/query_update_worker.py): each of the seven is, on
    some case, the first call a session answers after an update, and each of
    those that read the stage planes is the first on a round that rebuilt
    them and whose calls the kernels answered."""
    import query_update_session as qs
    recs = {c: r for c, r in results[sched].items() if c in qc.all_cases()}
    assert {call for r in recs.values() for call in r["first_asked"]} == set(qs.ORDER)
    on_planes = {call for r in recs.values() for k, call in enumerate(r["first_asked"])
                 if r["rebuilds"][k] and not r["host_only"][k]}
    assert {"task", "room", "fit", "node", "drain"} <= on_planes, on_planes
