"""kbg_node_reasons on the device: the session checks of
tests/node_why_session.py (expected rows from the fixture and the oracle's
output, the transpose of kbg_task_reasons, the two paths, named nodes, the
logs of the actions that follow, the hand-derived KAT, three resident sessions,
the refusals), one session whose last 64-node word is ragged past 8192 nodes,
and one resident session queried after a preempt that left staged deltas."""
import ctypes

import pytest

import node_why_session as ns
import node_why_worker as nw
import task_why_session as ts
from kbgpu import _abi, synth
from test_task_why_gpu import ragged_fixture

pytestmark = pytest.mark.gpu
OPTS = None
# a subset of the hostsim seeds: every generator, cycles that evict among them, none whose cycle discards a statement
DEVICE_CASES = ["kat_task_why", "kat_reclaim", "kat_preempt", "random5", "contended7", "contended19", "ports1",
                "affinity506"]


@pytest.fixture(scope="module", autouse=True)
def device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_session_rows_match_the_reference(case):
    errs, seen, skipped, differs = nw.run_session_case(case, OPTS)
    assert not errs, "\n".join(errs[:20])
    assert not skipped


def test_hand_derived_kat():
    errs = ns.check_kat(nw.session_fixture("kat_node_why"))
    assert not errs, "\n".join(errs)


def test_refusals():
    errs = ns.check_refusals(nw.session_fixture("kat_task_why"))
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("case", nw.RESIDENT)
def test_resident_session(case):
    errs = ns.check_resident(case, OPTS)
    assert not errs, "\n".join(errs[:20])


def test_ragged_last_word():
    """129 words, the last one ragged: every node answers for every Pending
    task, the only unschedulable node and the only tainted one turn all of
    them away, and the named call reaches the first, a middle and the last
    word in one launch."""
    fx = ragged_fixture()
    n = len(fx["nodes"])
    assert 8193 <= n <= 8300 and n % 64
    ssn, _ = ts.ws.open_with_reasons(dict(fx, actions=["allocate"]), OPTS)
    try:
        ts.run_actions(ssn, ["allocate"])
        rows = ssn.node_reasons()
        assert len(rows) == n and all(r["valid"] for r in rows)
        pending = rows[0]["pending"]
        assert pending >= 2, "no Pending task left: the case says nothing"
        assert ns.host_rows(ssn) == rows
        for r in rows:
            assert r["pending"] == pending == sum(r["count"])
        assert rows[n - 1]["count"][ts.tr.UNSCHEDULABLE] + rows[n - 1]["count"][ts.tr.SELECTOR] == pending
        assert rows[n - 1]["count"][ts.tr.UNSCHEDULABLE] >= 2  # the two pods without a selector
        assert rows[n - 2]["count"][ts.tr.TAINTS] >= 2
        tasks = [t for t in ssn.task_reasons() if t["valid"]]
        for c in range(10):
            assert sum(r["count"][c] for r in rows) == sum(t["count"][c] for t in tasks)
        pick = [n - 1, 0, 4100, n - 1, 63, 64, 8191, 8192]
        assert ssn.node_reasons(pick) == [rows[i] for i in pick]
    finally:
        ssn.close()


def test_query_after_preempt_with_staged_deltas():
    """A resident session (two cycles, kbg_session_reset between them): the
    device table must be current when the kernel reads it, so after every
    action, reclaim and preempt with their evictions included, the rows of the
    device path equal the host mirror's, and the rows at the start of the
    second cycle are those at open."""
    fx = dict(synth.contended_fixture(7), actions=["reclaim", "allocate", "backfill", "preempt"])
    ssn, _ = ts.ws.open_with_reasons(fx, OPTS)
    try:
        at_open = ssn.node_reasons()
        assert at_open and at_open[0]["pending"] > 0 and ns.host_rows(ssn) == at_open
        cap = len(ssn.flat.task_objs) + 1
        buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
        for cycle in range(2):
            for name in fx["actions"]:
                _abi.check(getattr(_abi.lib(), ts.ws.ENTRY[name])(ssn.handle, buf, cap, ctypes.byref(n)))
                rows = ssn.node_reasons()
                assert ns.host_rows(ssn) == rows, f"cycle {cycle} after {name}"
                assert ssn.node_reasons([1, 0, 1]) == [rows[1], rows[0], rows[1]]
            ev, ne = (_abi.kbg_eviction * cap)(), ctypes.c_int32(0)
            _abi.check(_abi.lib().kbg_evictions_get(ssn.handle, ev, cap, ctypes.byref(ne)))
            assert ne.value > 0, "the cycle evicted nothing: the case says nothing"
            assert rows != at_open
            _abi.check(_abi.lib().kbg_session_reset(ssn.handle))
            assert ssn.node_reasons() == at_open, f"after the reset of cycle {cycle}"
    finally:
        ssn.close()
