"""Per-predicate unschedulable reasons (kbg_job_reasons, include/kbgpu.h) on
the CPU: one allocate cycle without a device through the tool library
(kbg_tool_reasons_host), whose answers come from the host path of the
FitError computation (compute_fit_deltas' node loop over the rewound mirror,
the static predicate split by the host-evaluated stage planes).

The hand-written sessions and their hand-derived counts live in
tests/reasons_cases.py; each cycle's decision log is also checked against the
oracle, so the evaluation points the derivations assume are the reference's.
The seeded sessions are compared with the plain restatement in
tests/reasons_ref.py, and checked for the accounting invariant
sum(count) + fit_nodes + (allocated ? 1 : 0) == visited and for the mask
identity class_mask == sel_ok & taint_ok & ~unsched & live. No seed skips.
Sessions with inter-pod (anti)affinity need a device session's cycle: the
tool declines them (checked here) and tests/test_reasons_gpu.py runs them."""
import ctypes

import pytest

import reasons_cases as rc
import reasons_ref
from helpers import build_tools, run_oracle


@pytest.fixture(scope="module")
def tools():
    L = ctypes.CDLL(build_tools())
    L.kbg_tool_reasons_host.restype = ctypes.c_int32
    L.kbg_last_error.restype = ctypes.c_char_p
    return L


class HostRun:
    """One cycle of fixture `fx` through kbg_tool_reasons_host."""

    def __init__(self, tools, fx, reasons=1):
        from kbgpu import _abi
        from kbgpu.cache import FakeBinder, cache_from_fixture
        from kbgpu.fixture import _OrderedCache, fixture_tiers
        from kbgpu.snapshot import FlatSnapshot
        self.snap = _OrderedCache(cache_from_fixture(fx, FakeBinder()), fx).snapshot()
        self.flat = f = FlatSnapshot(self.snap.nodes, self.snap.jobs, self.snap.queues, self.snap.others,
                                     fixture_tiers(fx))
        o = _abi.kbg_options()
        o.reasons = reasons
        cap, J = len(f.task_objs) + 1, max(1, len(self.snap.jobs))
        out, n = (_abi.kbg_decision * cap)(), ctypes.c_int32()
        self.reasons, self.states = (_abi.kbg_job_reasons * J)(), (_abi.kbg_job_state * J)()
        status, dims = ctypes.c_int32(-1), (ctypes.c_int32 * 3)()
        mcap = 1 << 14
        masks = (ctypes.c_uint64 * mcap)()
        self.rc = tools.kbg_tool_reasons_host(ctypes.byref(f.snap), ctypes.byref(o), out, cap, ctypes.byref(n),
                                              self.reasons, ctypes.byref(status), self.states, dims, masks,
                                              ctypes.c_int64(mcap))
        self.error = tools.kbg_last_error().decode() if self.rc else ""
        self.get_status = status.value
        self.n_classes, self.W, self.pred = dims
        self.masks = masks
        self.log = [{"task": f.task_objs[out[i].task].uid, "node": f.node_names[out[i].node],
                     "kind": "allocate" if out[i].kind == _abi.KIND_ALLOCATE else "pipeline"} for i in range(n.value)]

    def task_uid(self, j):
        return self.flat.task_objs[self.reasons[j].task].uid if self.reasons[j].valid else None

    def allocated(self, j):
        """The job's described task was allocated (its own decision follows its evaluation point)."""
        r = self.reasons[j]
        return r.before < len(self.log) and self.log[r.before]["task"] == self.task_uid(j) and \
            self.log[r.before]["kind"] == "allocate"


@pytest.mark.parametrize("case", rc.HOST_CASES)
def test_hand_written_case(tools, case):
    fx, want = rc.CASES[case]()
    run = HostRun(tools, fx)
    assert run.rc == 0, run.error
    assert run.get_status == 0
    ref = run_oracle(fx)
    assert [(d["task"], d["node"], d["kind"]) for d in ref["decisions"]] == \
           [(d["task"], d["node"], d["kind"]) for d in run.log]
    seen = set()
    for j, job in enumerate(run.snap.jobs):
        if job.uid in want:
            rc.check_job(run.reasons[j], want[job.uid], run.task_uid(j), run.states[j].fit_nodes)
            seen.add(job.uid)
    assert seen == set(want)


@pytest.mark.parametrize("case", rc.AFFINITY_CASES)
def test_tool_declines_pod_affinity(tools, case):
    from kbgpu import _abi
    run = HostRun(tools, rc.CASES[case]()[0])
    assert run.rc == -_abi.KBG_E_UNSUPPORTED and "affinity" in run.error


def test_option_off_is_invalid(tools):
    """A session opened without kbg_options.reasons: KBG_E_INVALID, and the
    FitError counts are what they are with the option on."""
    from kbgpu import _abi
    fx, _ = rc.earlier_stage_wins()
    off, on = HostRun(tools, fx, reasons=0), HostRun(tools, fx, reasons=1)
    assert off.rc == 0 and off.get_status == _abi.KBG_E_INVALID
    assert on.rc == 0 and on.get_status == _abi.KBG_OK
    assert off.log == on.log
    for a, b in zip(off.states, on.states):
        assert (a.ready_num, a.fit_valid, a.fit_nodes, a.fit_cpu, a.fit_memory, a.fit_gpu) == \
               (b.ready_num, b.fit_valid, b.fit_nodes, b.fit_cpu, b.fit_memory, b.fit_gpu)


def test_ready_job_is_not_reported(tools):
    """minMember 0: the job is ready whatever happens to t1, so valid == 0;
    the same session with a PodGroup that cannot get ready is reported."""
    fx, want = rc.selector_alone()
    fx["podGroups"][0]["minMember"] = 0
    run = HostRun(tools, fx)
    assert run.rc == 0 and run.get_status == 0
    assert run.states[0].ready == 1 and run.reasons[0].valid == 0 and run.reasons[0].visited == 0
    fx["podGroups"][0]["minMember"] = rc.NEVER_READY
    assert HostRun(tools, fx).reasons[0].valid == 1


@pytest.mark.parametrize("kind,seed", rc.SEEDS)
def test_seeded_session(tools, kind, seed):
    fx = rc.seeded_fixture(kind, seed)
    run = HostRun(tools, fx)
    assert run.rc == 0, run.error  # the listed seeds open: none may skip
    assert run.get_status == 0
    assert all(n.node is not None for n in run.snap.nodes)  # the invariant is stated without nil Nodes
    # the mask identity, every class (with the predicates plugin off the one class is `always`)
    C, W = run.n_classes, run.W
    m = list(run.masks[:3 * C * W + 2 * W])
    cm, sel, taint = m[:C * W], m[C * W:2 * C * W], m[2 * C * W:3 * C * W]
    unsched, live = m[3 * C * W:3 * C * W + W], m[3 * C * W + W:]
    if run.pred:
        for c in range(C):
            for w in range(W):
                assert cm[c * W + w] == sel[c * W + w] & taint[c * W + w] & ~unsched[w] & live[w], (c, w)
    assert sum(bin(w).count("1") for w in live) == len(run.snap.nodes)
    reported = 0
    for j, job in enumerate(run.snap.jobs):
        r, st = run.reasons[j], run.states[j]
        if not r.valid:
            continue
        reported += 1
        assert st.fit_valid == 1
        assert sum(r.count) + st.fit_nodes + (1 if run.allocated(j) else 0) == r.visited, job.uid
        for k in range(6):
            assert (r.first_node[k] >= 0) == (r.count[k] > 0)
        if not run.pred:
            assert list(r.count) == [0] * 6
        got = (r.visited, list(r.count), list(r.first_node))
        assert got == reasons_ref.job_reasons(fx, run.snap.nodes, run.log, run.task_uid(j), r.before, bool(run.pred)), \
            job.uid
    assert reported > 0


def test_abi_is_additive(tmp_path):
    """kbg_job_reasons and kbg_options as C lays them out against the ctypes
    mirror: `reasons` took one reserved slot, kbg_options keeps its size."""
    import os
    import subprocess
    from helpers import ROOT
    from kbgpu import _abi
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "kbgpu.h"', "int main(void){"]
    for s in ("kbg_job_reasons", "kbg_options"):
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for fname, _ in getattr(_abi, s)._fields_:
            lines.append(f'printf("{s}.{fname} %zu\\n", offsetof({s}, {fname}));')
    lines.append('printf("why %d %d\\n", KBG_WHY_POD_CAP, KBG_WHY_POD_AFFINITY);')
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.split("\n") if l)
    for s in ("kbg_job_reasons", "kbg_options"):
        cls = getattr(_abi, s)
        assert int(got[s]) == ctypes.sizeof(cls), s
        for fname, _ in cls._fields_:
            assert int(got[f"{s}.{fname}"]) == getattr(cls, fname).offset, (s, fname)
    assert ctypes.sizeof(_abi.kbg_options) == 48 and ctypes.sizeof(_abi.kbg_job_reasons) == 72
    assert got["why"].split() == [str(_abi.WHY_POD_CAP), str(_abi.WHY_POD_AFFINITY)]
    assert _abi.lib().kbg_abi_version() == 13


def test_unschedulable_message():
    from kbgpu import _abi
    from kbgpu.fixture import unschedulable_message
    r, st = _abi.kbg_job_reasons(), _abi.kbg_job_state()
    assert unschedulable_message(r) == "0 nodes are available"  # valid == 0
    r.valid, r.visited = 1, 12
    assert unschedulable_message(r, st) == "0/12 nodes are available."
    r.count[_abi.WHY_TAINTS], r.count[_abi.WHY_SELECTOR], r.count[_abi.WHY_POD_CAP] = 3, 5, 10
    st.fit_valid, st.fit_nodes, st.fit_memory, st.fit_cpu = 1, 2, 2, 1
    # each group sorted as sort.Strings sorts FitError's parts ("10 ..." before "3 ...")
    assert unschedulable_message(r, st) == (
        "0/12 nodes are available: 10 can not allow more task running on it, 3 does not tolerate node taints, "
        "5 didn't match node selector, 1 insufficient cpu, 2 insufficient memory.")
    r.count[_abi.WHY_HOST_PORTS], r.count[_abi.WHY_UNSCHEDULABLE], r.count[_abi.WHY_POD_AFFINITY] = 1, 1, 1
    msg = unschedulable_message(r)
    for text in ("1 didn't have available host ports", "1 set to unschedulable", "1 affinity/anti-affinity failed"):
        assert text in msg
    assert "insufficient" not in msg
