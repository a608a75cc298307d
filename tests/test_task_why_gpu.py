"""kbg_task_reasons on the device: the session checks of
tests/task_why_session.py (expected rows from the fixture and the oracle's
output, the invariants, the hand-derived KAT, a resident session, the
refusals), one session whose last 64-node word is ragged past 8192 nodes, and
one resident session queried after a preempt that left staged deltas."""
import copy
import ctypes

import pytest

import task_why_session as ts
import task_why_worker as tw
from kbgpu import _abi, synth

pytestmark = pytest.mark.gpu
OPTS = None
# a subset of the hostsim seeds: every generator, cycles that evict among them (contended7, ports1, ports13,
# affinity506), none whose cycle discards a statement
DEVICE_CASES = ["kat_task_why", "kat_reclaim", "kat_preempt", "random5", "random7", "contended7", "contended19",
                "ports0", "ports1", "ports13", "affinity500", "affinity506"]


@pytest.fixture(scope="module", autouse=True)
def device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_session_rows_match_the_reference(case):
    errs, seen, skipped = tw.run_session_case(case, OPTS)
    assert not errs, "\n".join(errs[:20])
    assert not skipped


@pytest.mark.parametrize("name", ["kat_task_why", "kat_task_why_host"])
def test_hand_derived_kat(name):
    errs = ts.check_kat(tw.session_fixture(name))
    assert not errs, "\n".join(errs)


def test_refusals():
    errs = ts.check_refusals(tw.session_fixture("kat_task_why"))
    assert not errs, "\n".join(errs)


def test_resident_session():
    errs, _, _ = tw.run_session_case("resident", OPTS)
    assert not errs, "\n".join(errs[:20])


def ragged_fixture(nodes=8250):
    """contended_fixture's jobs on `nodes` nodes (8193..8300: 129 words, the
    last one ragged): the extra nodes are copies of its first ones, empty.
    Two more Pending pods of a job of their own stay Pending whatever allocate
    does: one asks for more cpu than any node has, one for more memory."""
    fx = copy.deepcopy(synth.contended_fixture(6))
    base = list(fx["nodes"])
    for i in range(len(base), nodes):
        n = copy.deepcopy(base[i % len(base)])
        n["name"] = f"extra{i:05d}"
        fx["nodes"].append(n)
    # the only unschedulable node and the only tainted one sit in the last word
    fx["nodes"][-1]["unschedulable"] = True
    fx["nodes"][-2]["taints"] = [{"key": "dedicated", "value": "x", "effect": "NoSchedule"}]
    fx["podGroups"].append({"namespace": "rag", "name": "rag-pg", "minMember": 1, "queue": fx["queues"][0]["name"],
                            "creationTimestamp": 0})
    for k, req in enumerate(({"cpu": "1000"}, {"cpu": "1", "memory": "4096Gi"})):
        fx["pods"].append({"uid": f"zz-rag{k}", "namespace": "rag", "name": f"rag-pg-t{k}", "phase": "Pending",
                           "nodeName": "", "annotations": {"scheduling.k8s.io/group-name": "rag-pg"},
                           "containers": [{"requests": req}]})
    return fx


def test_ragged_last_word():
    fx = ragged_fixture()
    assert 8193 <= len(fx["nodes"]) <= 8300 and len(fx["nodes"]) % 64
    ssn, _ = ts.ws.open_with_reasons(dict(fx, actions=["allocate"]), OPTS)
    try:
        ts.run_actions(ssn, ["allocate"])
        rows = ssn.task_reasons()
        assert rows, "no Pending task left: the case says nothing"
        assert ts.host_rows(ssn) == rows
        for r in rows:
            assert r["valid"] and sum(r["count"]) == r["visited"] == len(fx["nodes"])
        n = len(fx["nodes"])
        for r in rows:  # (no Pending pod of the generator tolerates a taint)
            assert (r["count"][ts.tr.UNSCHEDULABLE], r["first_node"][ts.tr.UNSCHEDULABLE]) in ((1, n - 1), (0, -1))
            assert (r["count"][ts.tr.TAINTS], r["first_node"][ts.tr.TAINTS]) in ((1, n - 2), (0, -1))
        rag = [r for r in rows if ssn.flat.task_objs[r["task"]].uid.startswith("zz-rag")]
        assert len(rag) == 2
        for r in rag:  # no selector: both nodes are reached, and nothing fits
            assert r["count"][ts.tr.UNSCHEDULABLE] == r["count"][ts.tr.TAINTS] == 1
            assert r["count"][ts.tr.FITS_IDLE] == r["count"][ts.tr.FITS_RELEASING] == 0 and r["count"][ts.tr.SHORT] > 8000
    finally:
        ssn.close()


def test_query_after_preempt_with_staged_deltas():
    """A resident session (two cycles, kbg_session_reset between them): the
    device table must be current when the kernel reads it, so after every
    action, reclaim and preempt with their evictions included, the rows of the
    device path equal the host mirror's, and a task's row at the start of the
    second cycle is its row at open."""
    fx = dict(synth.contended_fixture(7), actions=["reclaim", "allocate", "backfill", "preempt"])
    ssn, _ = ts.ws.open_with_reasons(fx, OPTS)
    try:
        tasks = [r["task"] for r in ssn.task_reasons()]
        at_open = ssn.task_reasons(tasks)
        assert tasks and ts.host_rows(ssn, tasks) == at_open
        cap = len(ssn.flat.task_objs) + 1
        buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
        for cycle in range(2):
            for name in fx["actions"]:
                _abi.check(getattr(_abi.lib(), ts.ws.ENTRY[name])(ssn.handle, buf, cap, ctypes.byref(n)))
                rows = ssn.task_reasons(tasks)
                assert ts.host_rows(ssn, tasks) == rows, f"cycle {cycle} after {name}"
                if name == "preempt":
                    assert any(r["valid"] for r in rows) and not all(r["valid"] for r in rows)
            ev, ne = (_abi.kbg_eviction * cap)(), ctypes.c_int32(0)
            _abi.check(_abi.lib().kbg_evictions_get(ssn.handle, ev, cap, ctypes.byref(ne)))
            assert ne.value > 0, "the cycle evicted nothing: the case says nothing"
            _abi.check(_abi.lib().kbg_session_reset(ssn.handle))
            assert ssn.task_reasons(tasks) == at_open, f"after the reset of cycle {cycle}"
    finally:
        ssn.close()
