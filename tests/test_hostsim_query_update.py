"""The four query calls on sessions after update events, on the CPU: the
unchanged session code on hostsim's simulated HIP stream
(kube-arbitrator_amd/tools/libkbg_hostsim.so), under both schedules (eager,
lazy: tests/test_hostsim_parity.py). Every case of
tests/query_update_cases.py runs tests/query_update_session.py's check_rounds
in a child (tests/query_update_worker.py) whose only kbg library is the
hostsim one: a session is asked, updated and asked again, and every point is
compared with a fresh session on the replayed cache and with the references
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
    # (that the update is visible to the calls is tests/test_query_update_ref.py's, from the references)


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", CASES)
def test_device_shaped_path_answers_after_the_update(results, case, sched):
    """Without host ports, pod affinity or a nil Node the updated session's
    calls launch the task-reasons, headroom and victim-reasons kernels, and
    every update that rebuilt the session builds the stage planes again
    before its first answer."""
    rec = results[sched][case]
    for r, n in enumerate(rec["rebuilds"]):
        if n:
            assert rec["stage_mask"][r] > 0, f"round {r} rebuilt the session and no stage plane was built: {rec}"
    if not any(rec["host_only"]):
        for name in ("task_why", "task_headroom", "victim_why"):
            assert rec["launches"].get(name, 0) > 0, (name, rec["launches"])
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
