"""Per-predicate unschedulable reasons (kbg_job_reasons, include/kbgpu.h)
through device sessions: the hand-written sessions of tests/reasons_cases.py
(the ones with inter-pod affinity included: a device session's cycle carries
it) and seeded sessions, each answered twice — by kbg_reasons_kernel over the
stage planes (sessions without host ports or pod affinity) and by the host
path of the same computation (KBG_HOST_FITDELTA) — struct for struct equal,
and equal to the hand-derived counts or the restatement of
tests/reasons_ref.py. The option leaves the cycle's outputs as they are; a
resident session rebuilds its stage planes with its static masks; a session
whose shards are all local answers like an unsharded one; a session over a
communicator declines."""
import copy
import ctypes

import pytest

import reasons_cases as rc
import reasons_ref
from helpers import run_oracle

pytestmark = pytest.mark.gpu

kbgpu = pytest.importorskip("kbgpu")
from kbgpu import _abi, synth  # noqa: E402
from kbgpu.cache import FakeBinder, cache_from_fixture  # noqa: E402
from kbgpu.fixture import _OrderedCache, fixture_tiers, run_fixture, unschedulable_message  # noqa: E402
from kbgpu.framework import open_session  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


def struct_bytes(st):
    return bytes(memoryview(st).cast("B"))


class DeviceRun:
    """One allocate cycle of `fx` on a device session opened with reasons."""

    def __init__(self, fx, opts=None):
        self.out, ssn = run_fixture(fx, dict({"device": 0, "reasons": 1}, **(opts or {})))
        assert self.out["status"] == "ok", self.out
        try:
            self.jobs = [j.uid for j in ssn.jobs]
            self.reasons = [ssn.job_reasons(j) for j in range(len(ssn.jobs))]
            self.states = [ssn.job_state(j) for j in range(len(ssn.jobs))]
            self.tasks = [t.uid for t in ssn.flat.task_objs]
        finally:
            ssn.close()
        self.log = self.out["decisions"]
        # the nodes as the session opened on them (the wrapper's own were replayed into)
        self.nodes = _OrderedCache(cache_from_fixture(fx, FakeBinder()), fx).snapshot().nodes

    def task_uid(self, j):
        return self.tasks[self.reasons[j].task] if self.reasons[j].valid else None

    def allocated(self, j):
        r = self.reasons[j]
        return r.before < len(self.log) and self.log[r.before]["task"] == self.task_uid(j) and \
            self.log[r.before]["kind"] == "allocate"


def both_paths(fx, monkeypatch, opts=None):
    """The cycle answered by the device path (where the session takes it) and
    by the host path alone: the same structs, byte for byte."""
    monkeypatch.delenv("KBG_HOST_FITDELTA", raising=False)
    dev = DeviceRun(fx, opts)
    monkeypatch.setenv("KBG_HOST_FITDELTA", "1")
    host = DeviceRun(fx, opts)
    monkeypatch.delenv("KBG_HOST_FITDELTA")
    assert dev.log == host.log
    assert [struct_bytes(r) for r in dev.reasons] == [struct_bytes(r) for r in host.reasons]
    return dev


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_hand_written_case(case, monkeypatch):
    fx, want = rc.CASES[case]()
    run = both_paths(fx, monkeypatch)
    ref = run_oracle(fx)
    assert [(d["task"], d["node"], d["kind"]) for d in ref["decisions"]] == \
           [(d["task"], d["node"], d["kind"]) for d in run.log]
    seen = set()
    for j, uid in enumerate(run.jobs):
        if uid in want:
            rc.check_job(run.reasons[j], want[uid], run.task_uid(j), run.states[j].fit_nodes)
            seen.add(uid)
            row = run.out["jobs"][j].get("reasons")
            assert (row is None) == (want[uid] is None)
            if row:
                assert row["count"] == want[uid]["count"]
                assert row["message"] == unschedulable_message(run.reasons[j], run.states[j])
    assert seen == set(want)


def check_accounting(run):
    reported = 0
    for j, uid in enumerate(run.jobs):
        r, st = run.reasons[j], run.states[j]
        if not r.valid:
            continue
        reported += 1
        assert sum(r.count) + st.fit_nodes + (1 if run.allocated(j) else 0) == r.visited, uid
        for k in range(6):
            assert (r.first_node[k] >= 0) == (r.count[k] > 0)
    return reported


@pytest.mark.parametrize("kind,seed", rc.DEVICE_SEEDS)
def test_seeded_session(kind, seed, monkeypatch):
    fx = rc.seeded_fixture(kind, seed)
    run = both_paths(fx, monkeypatch)
    assert check_accounting(run) > 0
    pred = any(p.get("name") == "predicates" and not p.get("disablePredicate") for t in fx["tiers"] for p in t)
    for j, uid in enumerate(run.jobs):
        r = run.reasons[j]
        if r.valid:
            got = (r.visited, list(r.count), list(r.first_node))
            assert got == reasons_ref.job_reasons(fx, run.nodes, run.log, run.task_uid(j), r.before, pred), uid


@pytest.mark.parametrize("kind,seed", rc.AFFINITY_SEEDS)
def test_affinity_session_accounting(kind, seed, monkeypatch):
    """Contended sessions with required pod (anti)affinity: the invariant, and
    stages 0-4 as restated (a node the restatement passes is either passed or
    turned away by the pod affinity)."""
    fx = rc.seeded_fixture(kind, seed)
    run = both_paths(fx, monkeypatch)
    assert check_accounting(run) > 0
    for j, uid in enumerate(run.jobs):
        r = run.reasons[j]
        if r.valid:
            _, count, _ = reasons_ref.job_reasons(fx, run.nodes, run.log, run.task_uid(j), r.before, True)
            assert list(r.count)[:5] == count[:5], uid


def strip(out):
    out = copy.deepcopy(out)
    for row in out["jobs"]:
        row.pop("reasons", None)
    return out


@pytest.mark.parametrize("name", ["c1", "fuzz-21001", "fuzz-21014"])
def test_option_leaves_the_cycle_unchanged(name):
    fx = synth.config_fixture(1) if name == "c1" else synth.random_fixture(int(name.split("-")[1]))
    fx = dict(fx, actions=["allocate"])
    off, s0 = run_fixture(fx, {"device": 0})
    s0.close()
    on, s1 = run_fixture(fx, {"device": 0, "reasons": 1})
    s1.close()
    assert off["status"] == on["status"] == "ok"
    assert not any("reasons" in row for row in off["jobs"])
    assert strip(on) == off


def _cycle(ssn):
    """kbg_allocate through the C ABI, then every job's reasons and FitError counts."""
    L = _abi.lib()
    cap = max(1, len(ssn.flat.task_objs))
    buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
    _abi.check(L.kbg_allocate(ssn.handle, buf, cap, ctypes.byref(n)))
    log = [(ssn.flat.task_objs[buf[i].task].uid, buf[i].node, buf[i].kind) for i in range(n.value)]
    rows = []
    for j in range(len(ssn.jobs)):
        r, st = ssn.job_reasons(j), ssn.job_state(j)
        rows.append((r.valid, ssn.flat.task_objs[r.task].uid if r.valid else None, r.before, r.visited, list(r.count),
                     list(r.first_node), st.fit_nodes))
    return log, rows


def test_resident_session_rebuilds_the_planes(monkeypatch):
    """earlier_stage_wins, then n4 (the one node that passed) is cordoned and n5
    moves to zone a (it stays tainted): the session rebuilds its static masks,
    and the next cycle's reasons are those of a session opened on the updated
    cluster — n4 now unschedulable (3), n5 taints (4) instead of selector (1)."""
    monkeypatch.delenv("KBG_HOST_FITDELTA", raising=False)
    fx, want = rc.earlier_stage_wins()
    fx2 = copy.deepcopy(fx)
    fx2["nodes"][4]["unschedulable"] = True
    fx2["nodes"][5]["labels"]["zone"] = "a"
    changes = [("node_update", fx2["nodes"][4]), ("node_update", fx2["nodes"][5])]

    def opened(f):
        return open_session(_OrderedCache(cache_from_fixture(f, FakeBinder()), f), fixture_tiers(f), {"device": 0},
                            reasons=True)
    ssn = opened(fx)
    try:
        _, rows = _cycle(ssn)
        j = [job.uid for job in ssn.jobs].index("ns/pg1")
        assert rows[j][4] == want["ns/pg1"]["count"]
        _abi.check(_abi.lib().kbg_session_reset(ssn.handle))
        rebuilds = ssn.stats().update_rebuilds
        ssn.update(changes)
        assert ssn.stats().update_rebuilds == rebuilds + 1
        log, rows = _cycle(ssn)
    finally:
        ssn.close()
    fresh = opened(fx2)
    try:
        assert _cycle(fresh) == (log, rows)
    finally:
        fresh.close()
    assert rows[j][4] == [1, 1, 0, 2, 2, 0] and rows[j][5] == [1, 0, -1, 2, 3, -1] and rows[j][3] == 6


@pytest.mark.parametrize("name", ["earlier_stage_wins", "cap_from_this_cycle", "random-21014"])
def test_local_shards_equal_unsharded(name, monkeypatch):
    monkeypatch.delenv("KBG_HOST_FITDELTA", raising=False)
    fx = rc.seeded_fixture("random", 21014) if name.startswith("random") else rc.CASES[name]()[0]
    one, two = DeviceRun(fx), DeviceRun(fx, {"shards": 2})
    assert one.log == two.log
    assert [struct_bytes(r) for r in one.reasons] == [struct_bytes(r) for r in two.reasons]
    assert any(r.valid for r in one.reasons)


def test_refusals():
    """Opened without the option: KBG_E_INVALID. Over a communicator (one
    rank): KBG_E_UNSUPPORTED, and the cycle itself is as without the option."""
    from kbgpu.dist import ShardComm
    fx, _ = rc.earlier_stage_wins()
    out, ssn = run_fixture(fx, {"device": 0})
    try:
        with pytest.raises(_abi.KbgError) as e:
            ssn.job_reasons(0)
        assert e.value.code == _abi.KBG_E_INVALID
    finally:
        ssn.close()
    comm = ShardComm(device=0, rank=0, world=1)
    try:
        got, ssn = run_fixture(fx, {"comm": comm, "reasons": 1})
        try:
            assert got["decisions"] == out["decisions"] and not any("reasons" in row for row in got["jobs"])
            with pytest.raises(_abi.KbgError) as e:
                ssn.job_reasons(0)
            assert e.value.code == _abi.KBG_E_UNSUPPORTED
        finally:
            ssn.close()
    finally:
        comm.close()
