"""PodGroup, PDB, Queue and namespace update events on a resident session
(include/kbgpu.h KBG_EV_JOB_UPDATE, KBG_EV_QUEUE_SET, KBG_EV_QUEUE_UPDATE):
open(S0) + ssn.update(changes) + the cycle's actions must equal a fresh open of
the replayed cache in the session's order, and the oracle on S1 where a
fixture can say S1. JOB_UPDATE / QUEUE_SET batches run kbg_session_update's
in-place branch (no rebuild, nothing renumbered), which only a device session
executes. Nothing here skips: the cases and the listed seeds are accepted."""
import ctypes

import pytest

from helpers import compare_outputs, run_oracle
from update_events import CASES, CHANGES_OUTCOME, GPU_SEEDS, IN_PLACE, fixture_after, fuzz_changes, fuzz_fixture, replay

pytestmark = pytest.mark.gpu

kbgpu = pytest.importorskip("kbgpu")
from kbgpu import _abi  # noqa: E402
from kbgpu.fixture import _OrderedCache, fixture_tiers, run_fixture  # noqa: E402
from kbgpu.framework import open_session  # noqa: E402
from test_update_gpu import _open, abi_cycle  # noqa: E402

RENUMS = (_abi.RENUM_TASKS, _abi.RENUM_NODES, _abi.RENUM_JOBS, _abi.RENUM_QUEUES)


def renumbering(ssn, kind):
    L = _abi.lib()
    n = ctypes.c_int32(-1)
    _abi.check(L.kbg_session_renumbering(ssn.handle, kind, None, 0, ctypes.byref(n)))
    buf = (ctypes.c_int32 * max(1, n.value))()
    _abi.check(L.kbg_session_renumbering(ssn.handle, kind, buf, n.value, ctypes.byref(n)))
    return list(buf[:n.value])


def check_events(fx0, rounds, opts=None, in_place=False, after_round=None):
    """Returns (the cycle before the first update, the cycle after each round)."""
    actions = fx0.get("actions") or ["allocate"]
    ssn = _open(fx0, opts)
    cycles = []
    try:
        before = abi_cycle(ssn, actions)
        _abi.check(_abi.lib().kbg_session_reset(ssn.handle))
        for r, changes in enumerate(rounds):
            rebuilds = ssn.stats().update_rebuilds
            ssn.update(changes)
            if in_place:  # JOB_UPDATE / QUEUE_SET only: every index kept, the session not rebuilt
                assert [renumbering(ssn, k) for k in RENUMS] == [[], [], [], []]
                assert ssn.stats().update_rebuilds == rebuilds
            if after_round:
                after_round(r, ssn)
            renumbered = any(renumbering(ssn, k) for k in RENUMS)
            got = abi_cycle(ssn, actions)
            cycles.append(got)
            order = {"jobs": [j.uid for j in ssn.jobs], "nodes": list(ssn.flat.node_names),
                     "queues": [q.uid for q in ssn.queues]}
            fssn = open_session(_OrderedCache(replay(fx0, rounds[:r + 1]), {"sessionOrder": order}),
                                fixture_tiers(fx0), opts or {})
            try:
                assert [j.uid for j in fssn.jobs] == order["jobs"]
                assert [(q.uid, q.weight) for q in fssn.queues] == [(q.uid, q.weight) for q in ssn.queues]
                assert [(j.queue, j.min_available) for j in fssn.jobs] == [(j.queue, j.min_available) for j in ssn.jobs]
                if renumbered:  # (an in-place batch keeps every task index: new pods last, deleted ones stay)
                    assert [t.uid for t in fssn.flat.task_objs] == [t.uid for t in ssn.flat.task_objs]
                assert got == abi_cycle(fssn, actions)
            finally:
                fssn.close()
            fx1 = fixture_after(fx0, rounds[:r + 1])
            if fx1 is not None:  # also pinned to the oracle on S1
                fx1 = dict(fx1, sessionOrder=order)
                out, fs = run_fixture(fx1, opts)
                try:
                    compare_outputs(run_oracle(fx1), out)
                    if out["status"] == "ok":
                        assert got["decisions"] == out["decisions"] and got["binds"] == out["binds"]
                finally:
                    if fs:
                        fs.close()
            _abi.check(_abi.lib().kbg_session_reset(ssn.handle))
        return before, cycles
    finally:
        ssn.close()


def _placed(cycle, prefix):
    """Pods bound by the cycle whose key starts with `prefix` ("<namespace>/<name...>")."""
    return sum(1 for k in cycle["binds"] if k.startswith(prefix))


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_events_case(case):
    fx0, rounds = CASES[case]()

    def after_round(r, ssn):
        if case.startswith("queue_update") and r == 0:
            # [qa, qb] + the temporary index: qa is last, both of its indices map there
            assert renumbering(ssn, _abi.RENUM_QUEUES)[:3] == [1, 0, 1]
            assert [q.uid for q in ssn.queues][:2] == ["qb", "qa"]
    before, cycles = check_events(fx0, rounds, in_place=case in IN_PLACE, after_round=after_round)
    assert before["status"] == "ok" and all(c["status"] == "ok" for c in cycles)
    if case in CHANGES_OUTCOME:  # otherwise the case proves nothing
        assert cycles[0]["decisions"] != before["decisions"] or cycles[0]["jobs"] != before["jobs"]
    after = cycles[0]
    if case == "min_member_up":  # 2 pods never make 3: allocated in the session, nothing dispatched
        assert len(before["binds"]) == 2 and not after["binds"]
        assert after["jobs"][0]["ready"] is False and after["jobs"][0].get("fit_error")
    if case == "min_member_down":
        assert not before["binds"] and before["jobs"][0]["ready"] is False
        assert len(after["binds"]) == 2 and after["jobs"][0]["ready"] is True
    if case == "queue_set_weight":  # weights 1:1 give 2 + 2 of the node's 4 CPUs, 1:3 give 1 + 3
        assert (_placed(before, "qa/a"), _placed(before, "qb/b")) == (2, 2)
        assert (_placed(after, "qa/a"), _placed(after, "qb/b")) == (1, 3)
    if case == "queue_move":  # qb loses pgc's request, qa gains it: each queue's deserved share moves
        assert before["queues"] != after["queues"]
        assert (_placed(before, "qb/b"), _placed(after, "qb/b")) == (1, 2)


def test_update_events_refused_batch_changes_nothing():
    """A JOB_UPDATE naming a queue the batch deleted: KBG_E_INVALID before
    anything applies, so the next cycle is the cycle before it."""
    fx0, _ = CASES["queue_set_weight"]()
    ssn = _open(fx0)
    try:
        L = _abi.lib()
        before = abi_cycle(ssn, ["allocate"])
        _abi.check(L.kbg_session_reset(ssn.handle))
        evs = (_abi.kbg_event * 3)()
        evs[0] = _abi.kbg_event(kind=_abi.EV_QUEUE_SET, queue=0, weight=5)
        evs[1] = _abi.kbg_event(kind=_abi.EV_QUEUE_DELETE, queue=1)
        evs[2] = _abi.kbg_event(kind=_abi.EV_JOB_UPDATE, job=0, queue=1, min_available=3)
        rebuilds = ssn.stats().update_rebuilds
        assert L.kbg_session_update(ssn.handle, evs, 3) == _abi.KBG_E_INVALID
        assert ssn.stats().update_rebuilds == rebuilds
        _abi.check(L.kbg_session_reset(ssn.handle))
        assert abi_cycle(ssn, ["allocate"]) == before
        assert [(q.uid, q.weight) for q in ssn.queues] == [("qa", 1), ("qb", 1)]
    finally:
        ssn.close()


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_update_events_fuzz(seed):
    from kbgpu.cache import FakeBinder, cache_from_fixture
    from test_update_structural_host import _view
    fx0 = fuzz_fixture(seed)
    # the batch of the CPU test: generated against the session's lists (the same snapshot order)
    batch = fuzz_changes(fx0, seed, _view(cache_from_fixture(fx0, FakeBinder()), fx0))

    def after_round(r, ssn):
        if seed % 2:  # no structural kind in the batch: nothing renumbered (the masks may still be recompiled)
            assert [renumbering(ssn, k) for k in RENUMS] == [[], [], [], []]
    before, cycles = check_events(fx0, [batch], {"batch_tasks": 1 + seed % 7, "full_scan": seed % 2},
                                  after_round=after_round)
    assert before["status"] == "ok" and cycles[0]["status"] != "unsupported", (before["status"], cycles[0]["status"])
