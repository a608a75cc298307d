"""Queue and job names that return, on the CPU through the tool library
(kbg_tool_structural: the library's own precheck and apply, no device).
Every round of tests/revival_cases.py either must be accepted — then the
updated snapshot equals the replayed cache's, maps included, exactly as
test_update_events_host.apply_round compares it — or must be refused: the
wrapper's marshal raises the re-open ValueError naming the queue or JobID,
and the same events sent past the wrapper get KBG_E_UNSUPPORTED from the
library when the name left in that batch (the tool is stateless: names that
left in an earlier update are covered on sessions, tests/test_revival_hostsim.py
and test_revival_gpu.py). Nothing here skips."""
import ctypes

import pytest

from helpers import build_tools
from revival_cases import CASES, EXPECT, QUEUE_KINDS, SEEDS, fuzz_fixture, fuzz_rounds, refused_name, verdicts
from test_update_events_host import _raw, apply_round, run_tool
from test_update_structural_host import TOOLS, _view, canon
from update_events import _two_queues, replay


@pytest.fixture(scope="module")
def tools():
    build_tools()
    L = ctypes.CDLL(TOOLS)
    L.kbg_tool_structural.restype = ctypes.c_int32
    return L


def _fresh(fx0, done):
    return _view(replay(fx0, done), fx0)


def raw_revival(v, changes, refusal):
    """The batch up to the refused event as the wrapper marshals it, then that
    event as a caller without the wrapper would send it: (events, n)."""
    from kbgpu import _abi
    plan = v.marshal(changes[:refusal.event])
    evs = (_abi.kbg_event * (plan.n_ev + 1))()
    for i in range(plan.n_ev):
        evs[i] = plan.evs[i]
    e = evs[plan.n_ev]
    if refusal.kind in QUEUE_KINDS:
        e.kind, e.name, e.weight = _abi.EV_QUEUE_ADD, refusal.queue.encode(), 1
    else:
        e.kind, e.name = _abi.EV_JOB_ADD, refusal.job.encode()
        e.queue = min(plan.qidx.values())  # a live queue: the refusal is about the JobID
        e.min_available = 1
    return evs, plan.n_ev + 1, plan


def walk(tools, fx0, rounds):
    """Every round against its verdict; returns the verdicts."""
    from kbgpu import _abi
    want = verdicts(fx0, rounds)
    v = w = _fresh(fx0, [])  # v: a fresh view per round; w: one wrapper carried through the rounds
    done = []
    for r, refusal in enumerate(want):
        changes = rounds[r]
        if refusal is None:
            plan_w = w.marshal(changes) if w is not v else None
            nxt, plan, maps = apply_round(tools, fx0, v, done, changes)  # accepts into v (round 0: that is w)
            if plan_w is not None:
                w._accept(plan_w, maps=maps)
            assert [j.uid for j in w.jobs] == [j.uid for j in nxt.jobs]
            assert [(q.uid, q.weight) for q in w.queues] == [(q.uid, q.weight) for q in nxt.queues]
            assert [t.uid for t in w.flat.task_objs] == [t.uid for t in nxt.flat.task_objs]
            v = nxt
            done.append(changes)
            continue
        name = refused_name(refusal)
        for view in {id(v): v, id(w): w}.values():  # from the cache of this round, and from what the wrapper kept
            with pytest.raises(ValueError) as err:
                view.marshal(changes)
            assert repr(name) in str(err.value) and "re-open" in str(err.value), str(err.value)
        if refusal.seen and refusal.job in v.job_index:  # the name left in this batch: the library sees it
            evs, n, plan = raw_revival(v, changes, refusal)
            lens = (len(v.flat.task_objs) + len(plan.objs) + 1, len(v.flat.node_names) + len(plan.new_nodes),
                    len(v.jobs) + len(plan.new_jobs) + 1, len(v.queues) + len(plan.new_queues) + 1)
            rc, _, _ = run_tool(tools, v, evs, n, lens)
            assert rc == _abi.KBG_E_UNSUPPORTED, _abi.STATUS_NAMES.get(rc, rc)
    return want


@pytest.mark.parametrize("case", sorted(CASES))
def test_revival_host_case(tools, case):
    fx0, rounds = CASES[case]()
    want = walk(tools, fx0, rounds)
    if EXPECT[case] is None:
        assert want == [None] * len(rounds)
    else:
        assert (want[-1].round, refused_name(want[-1])) == EXPECT[case] and len(want) == len(rounds)


@pytest.mark.parametrize("seed", SEEDS)
def test_revival_host_fuzz(tools, seed):
    fx0 = fuzz_fixture(seed)
    walk(tools, fx0, fuzz_rounds(fx0, seed))


def _tool(tools, v, events):
    lens = (len(v.flat.task_objs) + 1, len(v.flat.node_names), len(v.jobs) + 2, len(v.queues) + 2)
    return run_tool(tools, v, _raw(*events), len(events), lens)


def test_revival_host_raw_queue(tools):
    """QUEUE_DELETE then QUEUE_ADD of the same name in one kbg_session_update,
    past the wrapper: the replayed cache holds qa/pga and its four Pending
    pods again (deleteQueue removed only sc.Queues["qa"]), so a library that
    takes the batch must show them; it does not adopt them, so it refuses."""
    from kbgpu import _abi
    fx0 = _two_queues()
    v = _fresh(fx0, [])
    q = [x.uid for x in v.queues].index("qa")
    rc, blob, _ = _tool(tools, v, [dict(kind=_abi.EV_QUEUE_DELETE, queue=q),
                                   dict(kind=_abi.EV_QUEUE_ADD, name=b"qa", weight=1)])
    cache = replay(fx0, [[("queue_delete", {"name": "qa"}), ("queue_add", {"name": "qa", "weight": 1})]])
    if rc == 0:  # taken: then it must be the replayed cache's session
        assert sorted(j[0] for j in canon(blob.snap)["jobs"]) == sorted(j.uid for j in cache.snapshot().jobs)
    assert rc == _abi.KBG_E_UNSUPPORTED
    # a queue without jobs is free to return, under another weight too
    fx1 = dict(fx0, pods=fx0["pods"][:4], podGroups=fx0["podGroups"][:1])
    v1 = _fresh(fx1, [])
    q = [x.uid for x in v1.queues].index("qb")
    rc, blob, maps = _tool(tools, v1, [dict(kind=_abi.EV_QUEUE_DELETE, queue=q),
                                       dict(kind=_abi.EV_QUEUE_ADD, name=b"qb", weight=3)])
    assert rc == 0 and canon(blob.snap)["queues"] == [("qa", 1), ("qb", 3)] and maps[3] == [0, -1, 1]
    blob.close()


def test_revival_host_raw_job(tools):
    """JOB_DELETE then JOB_ADD of the same JobID in one kbg_session_update,
    past the wrapper: deletePodGroup kept the JobInfo and its tasks, so the
    replayed cache's job holds its four pods."""
    from kbgpu import _abi
    fx0 = _two_queues()
    v = _fresh(fx0, [])
    j = [x.uid for x in v.jobs].index("qa/pga")
    q = [x.uid for x in v.queues].index("qa")
    rc, blob, _ = _tool(tools, v, [dict(kind=_abi.EV_JOB_DELETE, job=j),
                                   dict(kind=_abi.EV_JOB_ADD, name=b"qa/pga", queue=q, min_available=1)])
    pg = fx0["podGroups"][0]
    cache = replay(fx0, [[("pod_group_delete", pg), ("pod_group_add", pg)]])
    if rc == 0:  # taken: then the job must hold the replayed cache's tasks
        got = {row[0]: len(row[5]) for row in canon(blob.snap)["jobs"]}
        assert got["qa/pga"] == len(cache.jobs["qa/pga"].tasks) == 4
    assert rc == _abi.KBG_E_UNSUPPORTED
    # a job without pods is free to return
    fx1 = dict(fx0, pods=fx0["pods"][4:])
    v1 = _fresh(fx1, [])
    j = [x.uid for x in v1.jobs].index("qa/pga")
    q = [x.uid for x in v1.queues].index("qa")
    rc, blob, maps = _tool(tools, v1, [dict(kind=_abi.EV_JOB_DELETE, job=j),
                                       dict(kind=_abi.EV_JOB_ADD, name=b"qa/pga", queue=q, min_available=1)])
    assert rc == 0 and sorted((row[0], len(row[5])) for row in canon(blob.snap)["jobs"]) == [("qa/pga", 0), ("qb/pgb", 4)]
    blob.close()
    # ... but not once the batch gave it one
    p = fx0["pods"][0]
    pod_add = v1.marshal([("pod_add", p)]).evs[0]
    evs = _raw(dict(kind=_abi.EV_JOB_DELETE, job=j), dict(kind=_abi.EV_JOB_ADD, name=b"qa/pga", queue=q, min_available=1))
    batch = (_abi.kbg_event * 3)(pod_add, evs[0], evs[1])
    lens = (len(v1.flat.task_objs) + 2, len(v1.flat.node_names), len(v1.jobs) + 2, len(v1.queues) + 2)
    assert run_tool(tools, v1, batch, 3, lens)[0] == _abi.KBG_E_UNSUPPORTED


def test_revival_host_previously_accepted_seeds_stay_accepted(tools):
    """The refusals must not reach further than the names that return: every
    seed of the structural and update fuzz that the wrapper and the library
    took before is taken still (the counts are the parent commit's: 80 + 20
    seeds of test_structural_host_*, 40 of test_update_events_host_fuzz)."""
    from kbgpu import synth
    from test_update_structural_host import _structural, check
    from update_events import SEEDS as UPDATE_SEEDS, fuzz_changes, fuzz_fixture as update_fixture
    taken = 0
    for seed in UPDATE_SEEDS:
        fx0 = update_fixture(seed)
        v = _fresh(fx0, [])
        changes = fuzz_changes(fx0, seed, v)
        assert verdicts(fx0, [changes]) == [None], seed  # no name returns: must be accepted
        apply_round(tools, fx0, v, [], changes)
        taken += 1
    assert taken == 40
    taken = 0
    for seed in range(100):
        if seed < 80:
            fx0 = synth.random_fixture(11000 + seed) if seed % 3 else \
                synth.contended_fixture(11000 + seed, nodes=12, jobs=8, tasks=6)
        else:
            fx0 = synth.contended_fixture(11300 + seed - 80, nodes=10, jobs=10, tasks=6, ports=0.5)
        try:  # (check skips what it skipped before: a reference panic, a session that does not open, a re-open case)
            assert check(tools, fx0, _structural(fx0, seed if seed < 80 else seed - 80)) == 0
        except pytest.skip.Exception:
            continue
        taken += 1
    assert taken == 90
