"""Queue and job names that return, on sessions: what tests/test_revival_gpu.py
runs on the device and tests/hostsim_worker.py (mode "revival", for
tests/test_revival_hostsim.py) on the simulated stream. Every round of
tests/revival_cases.py that must be accepted is applied with ssn.update and
the cycle after it equals a fresh session's on the replayed cache (and the
oracle's where a fixture can say the cache); the round that must be refused is
refused by the wrapper and, sent past it, by the library — with the session
left exactly as it was, and still taking a valid batch afterwards."""
import ctypes

import pytest

from helpers import compare_outputs, run_oracle
from revival_cases import CASES, QUEUE_KINDS, fuzz_fixture, fuzz_rounds, refused_name, verdicts
from update_events import _pg, _two_queues, fixture_after, replay
from update_helpers import _open, abi_cycle

RENUMS = (0, 1, 2, 3)  # KBG_RENUM_TASKS, NODES, JOBS, QUEUES


def renumbering(ssn, kind):
    from kbgpu import _abi
    L = _abi.lib()
    n = ctypes.c_int32(-1)
    _abi.check(L.kbg_session_renumbering(ssn.handle, kind, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_int32 * max(1, n.value))()
    _abi.check(L.kbg_session_renumbering(ssn.handle, kind, buf, n.value, ctypes.byref(n)))
    return list(buf[:n.value])


def same_as_fresh(ssn, fx0, done, got, opts):
    """The cycle `got` of the updated session against a fresh session on the
    replayed cache in the session's order, and against the oracle where a
    fixture can say that cache (tests/test_update_events_gpu.py check_events)."""
    from kbgpu.fixture import _OrderedCache, fixture_tiers, run_fixture
    from kbgpu.framework import open_session
    actions = fx0.get("actions") or ["allocate"]
    order = {"jobs": [j.uid for j in ssn.jobs], "nodes": list(ssn.flat.node_names), "queues": [q.uid for q in ssn.queues]}
    fssn = open_session(_OrderedCache(replay(fx0, done), {"sessionOrder": order}), fixture_tiers(fx0), opts or {})
    try:
        assert [j.uid for j in fssn.jobs] == order["jobs"]
        assert [(q.uid, q.weight) for q in fssn.queues] == [(q.uid, q.weight) for q in ssn.queues]
        assert [(j.queue, j.min_available) for j in fssn.jobs] == [(j.queue, j.min_available) for j in ssn.jobs]
        assert [len(j.tasks) for j in fssn.jobs] == \
               [sum(1 for t in ssn.flat.task_objs if t is not None and t.job == j.uid) for j in ssn.jobs]
        assert got == abi_cycle(fssn, actions)
    finally:
        fssn.close()
    fx1 = fixture_after(fx0, done)
    if fx1 is not None:
        fx1 = dict(fx1, sessionOrder=order)
        out, fs = run_fixture(fx1, opts)
        try:
            compare_outputs(run_oracle(fx1), out)
            if out["status"] == "ok":
                assert got["decisions"] == out["decisions"] and got["binds"] == out["binds"]
        finally:
            if fs:
                fs.close()


def raw_revival(ssn, changes, refusal):
    """The batch up to the refused event as the wrapper marshals it, then that
    event as a caller without the wrapper sends it."""
    from kbgpu import _abi
    plan = ssn.marshal(changes[:refusal.event])
    evs = (_abi.kbg_event * (plan.n_ev + 1))()
    for i in range(plan.n_ev):
        evs[i] = plan.evs[i]
    e = evs[plan.n_ev]
    if refusal.kind in QUEUE_KINDS:
        e.kind, e.name, e.weight = _abi.EV_QUEUE_ADD, refusal.queue.encode(), 1
    else:
        e.kind, e.name = _abi.EV_JOB_ADD, refusal.job.encode()
        e.queue, e.min_available = min(plan.qidx.values()), 1
    return evs, plan.n_ev + 1, plan


def refused_leaves_the_session(ssn, send, name, actions):
    """`send()` is a kbg_session_update the library must refuse: the status,
    the name in kbg_last_error, no renumbering, no rebuild, and the next
    cycle equal to the one before, field by field."""
    from kbgpu import _abi
    L = _abi.lib()
    before = abi_cycle(ssn, actions)
    _abi.check(L.kbg_session_reset(ssn.handle))
    lists = ([j.uid for j in ssn.jobs], [(q.uid, q.weight) for q in ssn.queues], list(ssn.flat.node_names),
             [t.uid for t in ssn.flat.task_objs if t is not None])
    rebuilds = ssn.stats().update_rebuilds
    rc = send()
    assert rc == _abi.KBG_E_UNSUPPORTED, _abi.STATUS_NAMES.get(rc, rc)
    text = L.kbg_last_error().decode()
    assert f"'{name}'" in text and "re-open" in text, text
    assert [renumbering(ssn, k) for k in RENUMS] == [[], [], [], []]
    assert ssn.stats().update_rebuilds == rebuilds
    _abi.check(L.kbg_session_reset(ssn.handle))
    after = abi_cycle(ssn, actions)
    for k in before:
        assert after[k] == before[k], k
    assert after == before
    _abi.check(L.kbg_session_reset(ssn.handle))
    assert lists == ([j.uid for j in ssn.jobs], [(q.uid, q.weight) for q in ssn.queues], list(ssn.flat.node_names),
                     [t.uid for t in ssn.flat.task_objs if t is not None])
    return before


def run_rounds(fx0, rounds, opts=None):
    """One session through the rounds against their verdicts; returns them."""
    from kbgpu import _abi
    L = _abi.lib()
    actions = fx0.get("actions") or ["allocate"]
    want = verdicts(fx0, rounds)
    assert len(want) == len(rounds)
    ssn = _open(fx0, opts)
    try:
        assert abi_cycle(ssn, actions)["status"] != "unsupported"
        _abi.check(L.kbg_session_reset(ssn.handle))
        done = []
        for r, refusal in enumerate(want):
            changes = rounds[r]
            if refusal is None:
                ssn.update(changes)
                done.append(changes)
                got = abi_cycle(ssn, actions)  # (the names the session remembers outlive its cycles and resets)
                same_as_fresh(ssn, fx0, done, got, opts)
                _abi.check(L.kbg_session_reset(ssn.handle))
                continue
            name = refused_name(refusal)
            with pytest.raises(ValueError) as err:  # the wrapper, from what it kept through the rounds
                ssn.update(changes)
            assert repr(name) in str(err.value) and "re-open" in str(err.value), str(err.value)
            if not refusal.seen:  # never a session job: only the holder of the cache can know
                break
            evs, n, plan = raw_revival(ssn, changes, refusal)
            refused_leaves_the_session(ssn, lambda: L.kbg_session_update(ssn.handle, evs, n), name, actions)
            # a valid batch right after it still applies: the refused batch without the name that returns
            # (its own deletions among them), else a weight set in place
            valid = [c for k, c in enumerate(changes) if k != refusal.event]
            if verdicts(fx0, done + [valid])[-1] is not None or not valid:
                q = ssn.queues[0]
                valid = [("queue_add", {"name": q.uid, "weight": q.weight + 1})]
            assert verdicts(fx0, done + [valid])[-1] is None
            ssn.update(valid)
            done.append(valid)
            got = abi_cycle(ssn, actions)
            same_as_fresh(ssn, fx0, done, got, opts)
        return want
    finally:
        ssn.close()


def run_case(case, opts=None):
    fx0, rounds = CASES[case]()
    return run_rounds(fx0, rounds, opts)


def run_seed(seed, opts=None):
    fx0 = fuzz_fixture(seed)
    return run_rounds(fx0, fuzz_rounds(fx0, seed), opts)


def _raw(*events):
    from kbgpu import _abi
    evs = (_abi.kbg_event * len(events))()
    for i, fields in enumerate(events):
        for k, val in fields.items():
            setattr(evs[i], k, val)
    return evs


def run_raw_two_updates(what):
    """Raw ABI, the name deleted in one kbg_session_update and added in the
    next, with an unrelated structural batch, cycles and resets between them."""
    from kbgpu import _abi
    L = _abi.lib()
    fx0 = _two_queues()
    ssn = _open(fx0)
    try:
        if what == "queue":
            first = [("queue_delete", {"name": "qa"})]
            back = dict(kind=_abi.EV_QUEUE_ADD, name=b"qa", weight=1)
            name = "qa"
        else:
            first = [("pod_group_delete", fx0["podGroups"][0])]
            back = dict(kind=_abi.EV_JOB_ADD, name=b"qa/pga", queue=0, min_available=1)
            name = "qa/pga"
        ssn.update(first)
        for _ in range(2):
            abi_cycle(ssn, ["allocate"])
            _abi.check(L.kbg_session_reset(ssn.handle))
        ssn.update([("queue_add", {"name": "qz", "weight": 2})])  # a rebuild between the two
        abi_cycle(ssn, ["allocate"])
        _abi.check(L.kbg_session_reset(ssn.handle))
        evs = _raw(back)
        refused_leaves_the_session(ssn, lambda: L.kbg_session_update(ssn.handle, evs, 1), name, ["allocate"])
        # and a fresh name of either kind is taken still
        ok = _raw(dict(kind=_abi.EV_QUEUE_ADD, name=b"qy", weight=1),
                  dict(kind=_abi.EV_JOB_ADD, name=b"qb/new", queue=0, min_available=1))
        assert L.kbg_session_update(ssn.handle, ok, 2) == _abi.KBG_OK
    finally:
        ssn.close()


def run_refused_batch_records_nothing():
    """A refused batch deleted queue qb (with its job) before the name that
    made it refused: nothing of it may stay recorded. Once qb's job has moved
    to qa, qb leaves without jobs and is free to return."""
    from kbgpu import _abi
    L = _abi.lib()
    fx0 = _two_queues()
    ssn = _open(fx0)
    try:
        bad = [("queue_delete", {"name": "qb"}), ("queue_delete", {"name": "qa"}), ("queue_add", {"name": "qa", "weight": 1})]
        with pytest.raises(ValueError):
            ssn.update(bad)
        want = verdicts(fx0, [bad])[0]
        evs, n, _ = raw_revival(ssn, bad, want)
        refused_leaves_the_session(ssn, lambda: L.kbg_session_update(ssn.handle, evs, n), "qa", ["allocate"])
        rounds = [[("pod_group_update", _pg("qb", "pgb", "qa", created=1))],
                  [("queue_delete", {"name": "qb"}), ("queue_add", {"name": "qb", "weight": 2})]]
        assert verdicts(fx0, rounds) == [None, None]
        for r in range(2):
            ssn.update(rounds[r])
            same_as_fresh(ssn, fx0, rounds[:r + 1], abi_cycle(ssn, ["allocate"]), None)
            _abi.check(L.kbg_session_reset(ssn.handle))
        assert [(q.uid, q.weight) for q in ssn.queues] == [("qa", 1), ("qb", 2)]
    finally:
        ssn.close()


SPECIALS = {"raw_queue_two_updates": lambda: run_raw_two_updates("queue"),
            "raw_job_two_updates": lambda: run_raw_two_updates("job"),
            "refused_batch_records_nothing": run_refused_batch_records_nothing}
