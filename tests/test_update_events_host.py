"""PodGroup, PDB, Queue and namespace update events of kbg_session_update on
the CPU (no device): KBG_EV_JOB_UPDATE, KBG_EV_QUEUE_SET, KBG_EV_QUEUE_UPDATE
(include/kbgpu.h; event_handlers.go:344-494,635-755). The batch the wrapper
marshals (framework.Session.marshal) is prechecked and applied by the
library's own host code through the tool library (kbg_tool_structural, which
rebuilds the snapshot after any batch, in-place ones too), and the updated
snapshot must equal the snapshot of the Python cache mirror replayed through
the same handlers, in the wrapper's order. Nothing here skips: every case and
every listed seed must be accepted and compared. The GPU side
(tests/test_update_events_gpu.py) checks the cycles after such updates."""
import ctypes

import pytest

from helpers import build_tools, run_oracle
from test_update_structural_host import TOOLS, _view, canon
from update_events import CASES, IN_PLACE, SEEDS, fixture_after, fuzz_changes, fuzz_fixture, replay


@pytest.fixture(scope="module")
def tools():
    build_tools()
    L = ctypes.CDLL(TOOLS)
    L.kbg_tool_structural.restype = ctypes.c_int32
    return L


def run_tool(tools, v, evs, n_ev, lens):
    """kbg_tool_structural on view v's snapshot: (status, snapshot blob or None, the four maps)."""
    from kbgpu import _abi
    from kbgpu.snapshot import SnapshotBlob
    lens = (ctypes.c_int32 * 4)(*lens)
    maps = [(ctypes.c_int32 * max(1, lens[k]))() for k in range(4)]
    ptrs = (ctypes.POINTER(ctypes.c_int32) * 4)(*[ctypes.cast(m, ctypes.POINTER(ctypes.c_int32)) for m in maps])
    n_out = ctypes.c_int64(0)
    cap = 1 << 22
    out = (ctypes.c_uint8 * cap)()
    rc = tools.kbg_tool_structural(ctypes.byref(v.flat.snap), ctypes.byref(_abi.kbg_options()), evs, n_ev,
                                   out, ctypes.c_int64(cap), ctypes.byref(n_out), ptrs, lens)
    if rc != 0:
        return rc, None, None
    return 0, SnapshotBlob.decode(bytes(out[:n_out.value])), [list(maps[k][:lens[k]]) for k in range(4)]


def apply_round(tools, fx0, v, done, changes):
    """One update of view `v` (the session after the rounds in `done`): the
    library's updated snapshot against the replayed cache in the wrapper's
    order. Returns (the view of the session after it, the plan, the maps)."""
    from kbgpu import _abi
    plan = v.marshal(changes)  # a ValueError here fails the test: the cases and seeds are accepted ones
    lens = (len(v.flat.task_objs) + len(plan.objs) + 1, len(v.flat.node_names) + len(plan.new_nodes),
            len(v.jobs) + len(plan.new_jobs), len(v.queues) + len(plan.new_queues))
    rc, blob, maps = run_tool(tools, v, plan.evs, plan.n_ev, lens)
    assert rc == 0, _abi.STATUS_NAMES.get(rc, rc)
    got = canon(blob.snap)
    v._accept(plan, maps=maps)
    order = {"jobs": [j.uid for j in v.jobs], "nodes": [n for n in v.flat.node_names if n],
             "queues": [q.uid for q in v.queues]}
    ref = _view(replay(fx0, done + [changes]), dict(fx0, sessionOrder=order))
    want = canon(ref.flat.snap)
    if not blob.snap.n_node_pods:  # the library drops every copy when one is unknown
        for k in ("nodes", "pod_only_nodes"):
            want[k] = [r[:12] + (None,) + r[13:] for r in want[k]]
    assert got["queues"] == want["queues"]
    assert [j[0] for j in got["jobs"]] == [j[0] for j in want["jobs"]]
    for a, b in zip(got["jobs"], want["jobs"]):
        assert a == b, a[0]
    for k in ("nodes", "pod_only_nodes", "others"):
        assert got[k] == want[k], k
    # the wrapper's lists follow the library's: tasks in its order, jobs and queues with the events' fields
    assert [t.uid for t in v.flat.task_objs] == [t[0] for j in got["jobs"] for t in j[5]]
    assert [(j.uid, j.queue, j.min_available, j.creation_timestamp) for j in v.jobs] == \
           [(j[0], j[1], j[2], j[4]) for j in got["jobs"]]
    assert [(q.uid, q.weight) for q in v.queues] == got["queues"]
    for a, b in zip(v.jobs, ref.jobs):  # and what the events did to each job's PodGroup and PDB
        assert (a.pod_group is None, a.pdb is None) == (b.pod_group is None, b.pdb is None), a.uid
    blob.close()
    return ref, plan, maps


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_events_host_case(tools, case):
    from kbgpu import _abi
    from kbgpu.cache import FakeBinder, cache_from_fixture
    fx0, rounds = CASES[case]()
    v = _view(cache_from_fixture(fx0, FakeBinder()), fx0)
    queues0 = [q.uid for q in v.queues]
    jobs0 = {j.uid: j.queue for j in v.jobs}
    done = []
    for r, changes in enumerate(rounds):
        v, plan, maps = apply_round(tools, fx0, v, done, changes)
        done.append(changes)
        kinds = [plan.evs[k].kind for k in range(plan.n_ev)]
        if case in IN_PLACE:  # only JOB_UPDATE / QUEUE_SET: every index keeps its place
            assert kinds and set(kinds) <= {_abi.EV_JOB_UPDATE, _abi.EV_QUEUE_SET}
            for m in maps:
                assert m == list(range(len(m)))
        if r == 0 and case in ("queue_update", "queue_update_then_adds", "queue_update_chain"):
            # the queue is last among the old ones' survivors (new queues follow in event order), its jobs
            # are kept, and both its old index and the temporary one map to its final place: with them the
            # map is onto the new queue indices
            rq = maps[3]
            old, tmp = queues0.index("qa"), len(queues0)
            assert kinds[0] == _abi.EV_QUEUE_UPDATE
            assert rq[old] == rq[tmp] == len(queues0) - 1
            assert [q.uid for q in v.queues][:len(queues0)] == [q for q in queues0 if q != "qa"] + ["qa"]
            assert sorted(set(rq)) == list(range(len(v.queues)))
            assert len(rq) == len(v.queues) + 1  # one queue holds two old indices, every other exactly one
            assert {j.uid: j.queue for j in v.jobs if j.uid in jobs0} == jobs0
    if case == "pdb_delete_with_pod_group" or case == "pod_group_delete_pdb_left":
        assert plan.n_ev == 0  # the job stays in ssn.Jobs (cache.go:570): nothing to send
        assert "qa/pga" in [j.uid for j in v.jobs]
    if case == "pdb_delete_alone":
        assert [plan.evs[0].kind] == [_abi.EV_JOB_DELETE] and "ctl-a" not in [j.uid for j in v.jobs]
    if case == "pdb_add_new_job":
        assert plan.evs[0].kind == _abi.EV_JOB_ADD and v.jobs[-1].uid == "ctl-x" and len(v.jobs[-1].tasks) == 1
    if case == "namespaces":
        assert kinds == [_abi.EV_QUEUE_ADD, _abi.EV_QUEUE_SET, _abi.EV_QUEUE_UPDATE]
        assert [(q.uid, q.weight) for q in v.queues] == [("qb", 1), ("qc", 1), ("qa", 1)]
    if case == "namespace_delete":
        assert kinds == [_abi.EV_QUEUE_UPDATE, _abi.EV_QUEUE_DELETE]
        assert [q.uid for q in v.queues] == ["qb"] and [j.uid for j in v.jobs] == ["qb/pgb"]


def _raw(*events):
    from kbgpu import _abi
    evs = (_abi.kbg_event * len(events))()
    for i, fields in enumerate(events):
        for k, val in fields.items():
            setattr(evs[i], k, val)
    return evs


@pytest.mark.parametrize("bad", ["job_range", "job_negative", "queue_set_range", "queue_update_range",
                                 "job_update_queue_range", "job_deleted", "job_of_deleted_queue", "queue_set_deleted",
                                 "queue_update_deleted", "queue_update_twice_old_index", "job_update_deleted_queue",
                                 "job_update_updated_queue"])
def test_update_events_host_precheck(tools, bad):
    """Every refusal of the three kinds is KBG_E_INVALID, before anything is
    applied: an index out of range, a job or queue deleted earlier in the
    batch, a JOB_UPDATE whose queue is dead or out of range."""
    from kbgpu import _abi
    from kbgpu.cache import FakeBinder, cache_from_fixture
    fx0, _ = CASES["queue_update"]()  # 2 queues (qa, qb), 2 jobs (qa/pga in qa, qb/pgb in qb)
    v = _view(cache_from_fixture(fx0, FakeBinder()), fx0)
    J, Q = len(v.jobs), len(v.queues)
    ju, qs, qu = _abi.EV_JOB_UPDATE, _abi.EV_QUEUE_SET, _abi.EV_QUEUE_UPDATE
    batch = {
        "job_range": [dict(kind=ju, job=J, queue=0)],
        "job_negative": [dict(kind=ju, job=-1, queue=0)],
        "queue_set_range": [dict(kind=qs, queue=Q, weight=1)],
        "queue_update_range": [dict(kind=qu, queue=-1, weight=1)],
        "job_update_queue_range": [dict(kind=ju, job=0, queue=Q)],
        "job_deleted": [dict(kind=_abi.EV_JOB_DELETE, job=0), dict(kind=ju, job=0, queue=0)],
        "job_of_deleted_queue": [dict(kind=_abi.EV_QUEUE_DELETE, queue=1), dict(kind=ju, job=1, queue=0)],
        "queue_set_deleted": [dict(kind=_abi.EV_QUEUE_DELETE, queue=0), dict(kind=qs, queue=0, weight=2)],
        "queue_update_deleted": [dict(kind=_abi.EV_QUEUE_DELETE, queue=0), dict(kind=qu, queue=0, weight=2)],
        "queue_update_twice_old_index": [dict(kind=qu, queue=0, weight=2), dict(kind=qu, queue=0, weight=3)],
        "job_update_deleted_queue": [dict(kind=_abi.EV_QUEUE_DELETE, queue=1), dict(kind=ju, job=0, queue=1)],
        "job_update_updated_queue": [dict(kind=qu, queue=1, weight=2), dict(kind=ju, job=0, queue=1)],
    }[bad]
    lens = (len(v.flat.task_objs) + 1, len(v.flat.node_names), J, Q + 2)
    rc, _, _ = run_tool(tools, v, _raw(*batch), len(batch), lens)
    assert rc == _abi.KBG_E_INVALID
    # the same batch naming the queue by the index it took is accepted
    if bad == "job_update_updated_queue":
        batch[1]["queue"] = Q
        rc, blob, maps = run_tool(tools, v, _raw(*batch), len(batch), lens)
        assert rc == 0 and maps[3] == [0, 1, 1]
        got = canon(blob.snap)
        assert got["queues"] == [("qa", 1), ("qb", 2)] and [j[1] for j in got["jobs"]] == ["qb", "qb"]
        blob.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_update_events_host_fuzz(tools, seed):
    from kbgpu.cache import FakeBinder, cache_from_fixture
    fx0 = fuzz_fixture(seed)
    v = _view(cache_from_fixture(fx0, FakeBinder()), fx0)
    from kbgpu import _abi
    changes = fuzz_changes(fx0, seed, v)
    _, plan, _ = apply_round(tools, fx0, v, [], changes)
    kinds = {plan.evs[k].kind for k in range(plan.n_ev)}
    assert kinds & {_abi.EV_JOB_UPDATE, _abi.EV_QUEUE_SET, _abi.EV_QUEUE_UPDATE}
    if seed % 2:  # an in-place batch beside pod churn: no structural kind
        assert not kinds & _abi.STRUCTURAL_EVENTS


def test_update_events_seeds_open_under_the_oracle():
    """The listed seeds' S0, and S1 where a fixture can say it, open under the
    oracle (status ok: no RefPanic), and most of them can say S1."""
    from kbgpu.cache import FakeBinder, cache_from_fixture
    said = 0
    for seed in SEEDS:
        fx0 = fuzz_fixture(seed)
        assert run_oracle(fx0)["status"] == "ok", seed
        v = _view(cache_from_fixture(fx0, FakeBinder()), fx0)
        fx1 = fixture_after(fx0, [fuzz_changes(fx0, seed, v)])
        if fx1 is not None:
            said += 1
            assert run_oracle(fx1)["status"] == "ok", seed
    assert len(SEEDS) == 40 and said >= 20
