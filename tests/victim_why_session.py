"""Session-level checks of kbg_victim_reasons, shared by the hostsim tests
(tests/test_hostsim_victim_why.py, through tests/victim_why_worker.py) and
the device tests (tests/test_victim_why_gpu.py).

`check_fixture` opens a session with reasons, runs the fixture's actions one
by one and, after each, asks for the rows of every job in the three modes.
The expected rows are tests/victim_why_ref.py's rule applied to tables built
here in Python from
  - the fixture (node labels, taints, unschedulable; pod selectors, tolerations),
  - the Python cache mirror at open (which session tasks are Running on which
    node, in NodeInfo.Tasks order; MaxTaskNum; Allocatable; Pending tasks), and
  - the ORACLE's output of the same actions up to that point (evictions,
    decisions, job ready_num / allocated, queue allocated / deserved, node
    ntasks): kbref run on the fixture with the action list cut there;
nothing comes from the library's getters. At the end the four actions' logs,
evictions and final states must equal the oracle's, calls in between or not.

The oracle's log does not show the evictions of a discarded statement, which
leave the node's copy of the task Releasing (statement.go:81-108: unevict's
AddTask fails). `discard_free` tells from the oracle's output alone (node
Releasing against the committed evictions and pipelines) whether a fixture's
cycle has any; the seeded cases of `check_fixture` are picked among those that
have none. For seeds that do discard, `check_discard` compares the
device-shaped path with host_why on the same session instead."""
import copy

import reasons_ref as rr
import victim_ref as vr
import victim_why_ref as wr
from helpers import compare_outputs, run_oracle
from kbgpu import _abi
from kbgpu.api import PENDING, RUNNING
from kbgpu.cache import FakeBinder, cache_from_fixture
from kbgpu.fixture import _OrderedCache, fixture_tiers, session_output
from kbgpu.framework import get_action, open_session

MODES = (_abi.VMODE_PREEMPT_JOBS, _abi.VMODE_PREEMPT_TASKS, _abi.VMODE_RECLAIM)


def plugin_rules(tiers):
    """What the session reads of the tiers: the victim fns of the first tier
    that has any, per mode (session_plugins.go:59-140: a later tier's result is
    intersected with the first's, so the first decides alone), the predicates
    plugin and the priority plugin's task order."""
    pre, rec = [], []
    for t in tiers:
        p = r = 0
        for o in t.plugins:
            if o.name == "gang":
                p |= 0 if o.preemptable_disabled else wr.VP_GANG
                r |= 0 if o.reclaimable_disabled else wr.VP_GANG
            if o.name == "drf" and not o.preemptable_disabled:
                p |= wr.VP_DRF
            if o.name == "proportion" and not o.reclaimable_disabled:
                r |= wr.VP_PROP
        if p and not pre:
            pre = [p]
        if r and not rec:
            rec = [r]
    names = [(o.name, o) for t in tiers for o in t.plugins]
    return dict(pre=pre, rec=rec, predicates=any(n == "predicates" and not o.predicate_disabled for n, o in names),
                task_prio=any(n == "priority" and not o.task_order_disabled for n, o in names),
                proportion=any(n == "proportion" for n, _ in names))


class Mirror:
    """The session's Python cache mirror as it is at open."""

    def __init__(self, ssn):
        self.job_uids = [j.uid for j in ssn.jobs]
        jidx = {u: i for i, u in enumerate(self.job_uids)}
        qidx = {q.uid: i for i, q in enumerate(ssn.queues)}
        self.queue_uids = [q.uid for q in ssn.queues]
        self.job_queue = [qidx[j.queue] for j in ssn.jobs]
        self.job_min = [j.min_available for j in ssn.jobs]
        self.pending = [[(t.uid, t.priority, t.resreq.as_tuple(), t.pod) for t in j.tasks.values()
                         if t.status == PENDING] for j in ssn.jobs]
        self.task_index = {t.uid: i for i, t in enumerate(ssn.flat.task_objs) if t is not None}
        self.req = {t.uid: t.resreq.as_tuple() for j in ssn.jobs for t in j.tasks.values()}
        self.task_job = {t.uid: jidx[j.uid] for j in ssn.jobs for t in j.tasks.values()}
        self.node_names = [n.name for n in ssn.nodes]
        self.node_objs = [n.node for n in ssn.nodes]
        self.maxtasks = [n.allocatable.max_task_num for n in ssn.nodes]
        self.total = [sum(n.allocatable.as_tuple()[d] for n in ssn.nodes) for d in range(3)]
        self.rel0 = [n.releasing.as_tuple() for n in ssn.nodes]
        # the session tasks Running on each node, in NodeInfo.Tasks order
        self.cands = [[t.uid for t in n.tasks.values() if t.uid in self.task_job and t.status == RUNNING]
                      for n in ssn.nodes]


def fixture_mirror(fx):
    """The Mirror of a fixture's fresh Python cache, without a session."""
    from types import SimpleNamespace
    snap = _OrderedCache(cache_from_fixture(fx, FakeBinder()), fx).snapshot()
    tasks = [t for j in snap.jobs for t in j.tasks.values()]
    return Mirror(SimpleNamespace(jobs=snap.jobs, queues=snap.queues, nodes=snap.nodes,
                                  flat=SimpleNamespace(task_objs=tasks)))


def discard_free(m, ref):
    """No statement of the oracle's cycle was discarded after evicting: every
    node's Releasing is its value at open plus the committed evictions on it
    minus the pipelines onto it."""
    rel = [list(r) for r in m.rel0]
    at = {u: n for n, us in enumerate(m.cands) for u in us}
    for e in ref.get("evictions", []):
        if e["task"] not in at:
            return False
        for d in range(3):
            rel[at[e["task"]]][d] += m.req[e["task"]][d]
    names = {nm: i for i, nm in enumerate(m.node_names)}
    for dcs in ref["decisions"]:
        if dcs["kind"] == "pipeline":
            for d in range(3):
                rel[names[dcs["node"]]][d] -= m.req[dcs["task"]][d]
    return all(list(map(float, a["releasing"])) == list(map(float, r)) for a, r in zip(ref["nodes"], rel))


def tables(m, ref, rules, mode):
    """The reference's case of one call: the victim tables now, one class per
    query (its task's pod against every node), the queries of the jobs that
    hold a Pending task. Returns (case, job index of each query)."""
    from types import SimpleNamespace

    import numpy as np
    c = SimpleNamespace()
    N = len(m.node_names)
    evicted = {e["task"] for e in ref.get("evictions", [])}
    decided = {d["task"] for d in ref["decisions"]}
    jobs = {j["uid"]: j for j in ref["jobs"]}
    queues = {q["uid"]: q for q in ref["queues"]}
    c.p = dict(node_lo=0, node_n=N, n_nodes=N)
    c.nt_off = np.concatenate([[0], np.cumsum([len(x) for x in m.cands])]).astype(np.int64)
    flat = [u for us in m.cands for u in us]
    c.c_jq = [(m.task_job[u], m.job_queue[m.task_job[u]]) for u in flat] or [(0, 0)]
    c.c_req = [list(map(float, m.req[u])) for u in flat] or [[0.0] * 3]
    c.c_run = [int(u not in evicted) for u in flat] or [0]
    c.j_min = list(m.job_min)
    c.j_ready = [jobs[u]["ready_num"] for u in m.job_uids]
    # drf's allocated: the AllocatedStatus tasks (JobInfo.Allocated) and the pipelined ones (drf.go:130-148)
    c.j_alloc = [list(map(float, jobs[u]["allocated"])) for u in m.job_uids]
    for d in ref["decisions"]:
        if d["kind"] == "pipeline":
            for k in range(3):
                c.j_alloc[m.task_job[d["task"]]][k] += m.req[d["task"]][k]
    zero = {"allocated": [0.0] * 3, "deserved": [0.0] * 3}
    c.q_alloc = [list(map(float, queues.get(u, zero)["allocated"])) for u in m.queue_uids]
    c.q_deserved = [list(map(float, queues.get(u, zero)["deserved"])) for u in m.queue_uids]
    by_name = {n["name"]: n for n in ref["nodes"]}
    c.ntasks = [by_name[nm]["ntasks"] for nm in m.node_names]
    c.maxtasks = list(m.maxtasks)
    c.panic_node = [0] * N
    c.dbl = [0.0] * 4 + [float(v) for v in m.total]
    c.live = [True] * N
    c.unsched = [bool(n.get("unschedulable")) for n in m.node_objs]
    c.sel_ok, c.taint_ok, c.queries, owners, tasks, over = [], [], [], [], [], []
    fns = rules["rec"] if mode == _abi.VMODE_RECLAIM else rules["pre"]
    for j, pend in enumerate(m.pending):
        left = [t for t in pend if t[0] not in decided]
        if not left:
            continue
        # TaskOrderFn (the priority plugin's), then UID
        uid, _, req, pod = min(left, key=lambda t: ((-t[1]) if rules["task_prio"] else 0, t[0]))
        la = [c.j_alloc[j][d] + req[d] for d in range(3)]
        c.queries.append(dict(mode=mode, cls=len(c.queries), cap_check=int(rules["predicates"]), n_tiers=len(fns),
                              tier_fns=list(fns), job=j, queue=m.job_queue[j], req=[float(v) for v in req],
                              ls=vr.share(la, [float(v) for v in m.total])))
        c.sel_ok.append([rr.selector_ok(pod, n) for n in m.node_objs])
        c.taint_ok.append([rr.taints_ok(pod, n) for n in m.node_objs])
        owners.append(j)
        tasks.append(m.task_index[uid])
        q = queues.get(m.queue_uids[m.job_queue[j]])  # Overused (proportion.go:188-194): only queues with an attr
        over.append(int(mode == _abi.VMODE_RECLAIM and rules["proportion"] and q is not None and
                        vr.less_equal(list(map(float, q["deserved"])), list(map(float, q["allocated"])))))
    return c, owners, tasks, over


def got_rows(whys):
    return [dict(count=list(w.count), first_node=list(w.first_node), fn_empty=list(w.fn_empty)) for w in whys]


def check_call(ssn, m, ref, rules, mode, tag):
    """Errors of one kbg_victim_reasons call against the reference."""
    c, owners, tasks, over = tables(m, ref, rules, mode)
    whys = ssn.victim_reasons(mode)
    errs = []
    valid = [j for j, w in enumerate(whys) if w.valid]
    if valid != owners:
        return [f"{tag}: jobs with a row {valid}, reference {owners}"]
    mine = [whys[j] for j in owners]
    want = wr.rows(c)
    errs += [f"{tag}: {e}" for e in wr.compare(c, want, got_rows(mine))]
    for w, r, t, o, j in zip(mine, want, tasks, over, owners):
        if w.task != t:
            errs.append(f"{tag}: job {j}: task {w.task}, reference {t}")
        if w.visited != sum(r["count"]):
            errs.append(f"{tag}: job {j}: visited {w.visited}, reference {sum(r['count'])}")
        if w.queue_overused != o:
            errs.append(f"{tag}: job {j}: queue_overused {w.queue_overused}, reference {o}")
    # a subset asked by index gives the same rows, in the order asked
    if len(owners) > 1:
        pick = [owners[-1], owners[0]]
        sub = ssn.victim_reasons(mode, pick)
        if got_rows(sub) != got_rows([whys[j] for j in pick]) or [w.task for w in sub] != [whys[j].task for j in pick]:
            errs.append(f"{tag}: jobs {pick} asked by index differ from their rows of the whole call")
    return errs


def open_with_reasons(fx, opts=None):
    binder = FakeBinder()
    cache = _OrderedCache(cache_from_fixture(fx, binder), fx)
    return open_session(cache, fixture_tiers(fx), dict(opts or {}), reasons=True), binder


def check_fixture(fx, opts=None, need_discard_free=True):
    """Every check of one fixture; returns (errors, seen): `seen` sums the
    reference's counts per cause over all calls, and fn_empty."""
    actions = fx.get("actions") or ["allocate"]
    ref_full = run_oracle(fx)
    assert ref_full["status"] == "ok", ref_full.get("error")
    ssn, binder = open_with_reasons(fx, opts)
    errs, seen = [], dict(count=[0] * wr.N_CAUSES, fn_empty=[0, 0, 0])
    try:
        m = Mirror(ssn)
        if need_discard_free:
            assert discard_free(m, ref_full), "the oracle's cycle discards a statement: pick another fixture"
        rules = plugin_rules(ssn.tiers)
        try:
            ssn.victim_reasons(_abi.VMODE_RECLAIM)
            errs.append("a call before the cycle's first action did not fail")
        except _abi.KbgError as e:
            if e.status != "invalid":
                errs.append(f"a call before the cycle's first action: {e}")
        status = "ok"
        for k, name in enumerate(actions):
            status = get_action(name).execute(ssn).status
            ref = ref_full if k + 1 == len(actions) else run_oracle(dict(fx, actions=actions[:k + 1]))
            for mode in MODES:
                errs += check_call(ssn, m, ref, rules, mode, f"after {name}, mode {mode}")
                c = tables(m, ref, rules, mode)[0]
                for r in wr.rows(c):
                    seen["count"] = [a + b for a, b in zip(seen["count"], r["count"])]
                    seen["fn_empty"] = [a + b for a, b in zip(seen["fn_empty"], r["fn_empty"])]
        try:  # the calls changed nothing: logs, evictions and final states are the oracle's
            compare_outputs(ref_full, session_output(ssn, binder.binds, status))
        except AssertionError as e:
            errs.append(f"the cycle with calls in between differs from the oracle's: {e}")
    finally:
        ssn.close()
    return errs, seen


def check_refusals(fx):
    """reasons = 0 gives KBG_E_INVALID, before and after the first action."""
    errs = []
    ssn = open_session(_OrderedCache(cache_from_fixture(fx, FakeBinder()), fx), fixture_tiers(fx), {})
    try:
        for when in ("before", "after"):
            try:
                ssn.victim_reasons(_abi.VMODE_RECLAIM)
                errs.append(f"reasons = 0, {when} the first action: the call did not fail")
            except _abi.KbgError as e:
                if e.status != "invalid":
                    errs.append(f"reasons = 0, {when} the first action: {e}")
            if when == "before":
                get_action((fx.get("actions") or ["allocate"])[0]).execute(ssn)
    finally:
        ssn.close()
    return errs


ENTRY = {"allocate": "kbg_allocate", "backfill": "kbg_backfill", "reclaim": "kbg_reclaim", "preempt": "kbg_preempt"}


def resident_rounds(fx0, seed, rounds):
    """[(fixture, changes, the oracle's output)] of a churn chain (helpers.churn_chain), from the oracle alone."""
    from helpers import churn_chain
    return [(fx, list(ch), out) for _, ch, fx, out in churn_chain(fx0, seed, rounds, lambda fx, ch: run_oracle(fx))]


def check_resident(fx0, seed, rounds, opts=None):
    """A resident session updated between cycles (kbg_session_reset,
    kbg_session_update): every round's rows against the reference on a fresh
    Python mirror of that round's fixture, read in the resident session's own
    numbering, and the round's decisions and node states against the oracle's."""
    import ctypes
    from types import SimpleNamespace
    errs = []
    ssn = None
    L = _abi.lib()
    try:
        for r, (fx, changes, ref_full) in enumerate(resident_rounds(fx0, seed, rounds)):
            assert ref_full["status"] == "ok", ref_full.get("error")
            actions = fx.get("actions") or ["allocate"]
            if ssn is None:
                ssn, _ = open_with_reasons(fx, opts)
            else:
                _abi.check(L.kbg_session_reset(ssn.handle))
                ssn.update(changes)
            fresh = _OrderedCache(cache_from_fixture(fx, FakeBinder()), fx).snapshot()
            fj, fq, fn = ({j.uid: j for j in fresh.jobs}, {q.uid: q for q in fresh.queues},
                          {n.name: n for n in fresh.nodes})
            view = SimpleNamespace(jobs=[fj[j.uid] for j in ssn.jobs], queues=[fq[q.uid] for q in ssn.queues],
                                   nodes=[fn[nm] for nm in ssn.flat.node_names],
                                   flat=SimpleNamespace(task_objs=[t for t in ssn.flat.task_objs]))
            m = Mirror(view)
            assert discard_free(m, ref_full), f"round {r}: the oracle's cycle discards a statement"
            rules = plugin_rules(ssn.tiers)
            cap = max(1, len(ssn.flat.task_objs))
            buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
            for k, name in enumerate(actions):
                _abi.check(getattr(L, ENTRY[name])(ssn.handle, buf, cap, ctypes.byref(n)))
                ref = ref_full if k + 1 == len(actions) else run_oracle(dict(fx, actions=actions[:k + 1]))
                for mode in MODES:
                    errs += check_call(ssn, m, ref, rules, mode, f"round {r} after {name}, mode {mode}")
            got = [(ssn.flat.task_objs[buf[i].task].uid, ssn.flat.node_names[buf[i].node],
                    "allocate" if buf[i].kind == _abi.KIND_ALLOCATE else "pipeline") for i in range(n.value)]
            if got != [(d["task"], d["node"], d["kind"]) for d in ref_full["decisions"]]:
                errs.append(f"round {r}: the decision log differs from the oracle's")
            for i, nm in enumerate(ssn.flat.node_names):
                st, want = ssn.node_state(i), next(x for x in ref_full["nodes"] if x["name"] == nm)
                if st.num_tasks != want["ntasks"] or \
                        [st.releasing.milli_cpu, st.releasing.memory, st.releasing.milli_gpu] != want["releasing"]:
                    errs.append(f"round {r}: node {nm} ends differently from the oracle's")
    finally:
        if ssn is not None:
            ssn.close()
    return errs


# ----------------------------------------------------------------- fixtures
def port_twin(fx):
    """The fixture with one more Running pod, of a job and queue of its own,
    that holds a host port nothing else asks for: the session has host ports,
    so kbg_victim_reasons evaluates every node on the host (host_why)."""
    fx = copy.deepcopy(fx)
    node = fx["nodes"][0]["name"]
    fx["queues"] = list(fx["queues"]) + [{"name": "twin-q", "weight": 1}]
    fx["podGroups"] = list(fx["podGroups"]) + [{"namespace": "twin", "name": "twin-pg", "minMember": 1,
                                                "queue": "twin-q", "creationTimestamp": 0}]
    fx["pods"] = list(fx["pods"]) + [{
        "uid": "zz-twin", "namespace": "twin", "name": "twin-pg-t0", "phase": "Running", "nodeName": node,
        "annotations": {"scheduling.k8s.io/group-name": "twin-pg"},
        "containers": [{"requests": {"cpu": "1m"}, "ports": [{"hostPort": 31999, "protocol": "TCP"}]}]}]
    return fx


def huge_fixture(running=1025):
    """Two nodes; n00 runs `running` 10m tasks of one gang job of queue q1
    (more than the device kernels take: kMaxNodeCandidates is 1024, so the
    session evaluates it on the host), n01 runs 130 (the big-node kernel's).
    Queue q2 holds Pending jobs whose reclaim / preempt tries look at both."""
    nds = [{"name": f"n{i:02d}", "allocatable": {"cpu": "64", "memory": "256Gi", "pods": "3000"}, "labels": {}}
           for i in range(2)]
    pods, pgs = [], []

    def job(name, queue, ts, n_tasks, cpu, node, min_member=1):
        pgs.append({"namespace": "ns", "name": name, "minMember": min_member, "queue": queue,
                    "creationTimestamp": ts * 1_000_000_000})
        for t in range(n_tasks):
            pods.append({"uid": f"{name}-{t:04d}", "namespace": "ns", "name": f"{name}-{t:04d}",
                         "phase": "Running" if node else "Pending", "nodeName": node or "",
                         "annotations": {"scheduling.k8s.io/group-name": name},
                         # (cpu alone: the eviction loop's Sub stays exact)
                         "containers": [{"requests": {"cpu": f"{cpu}m"}}]})

    job("runa", "q1", 0, running, 10, "n00")
    job("runb", "q1", 0, 130, 10, "n01", min_member=130)  # gang holds every task of it
    job("own", "q2", 0, 2, 10, "n01")
    for j in range(3):
        job(f"pend{j}", "q2", 100 + j, 2, 500 * (j + 1), None)
    job("pendq1", "q1", 200, 1, 20, None)  # (what the two tasks of `own` free: the pipeline after them fits)
    return {"name": "huge-node", "tiers": None, "nodes": nds, "pods": pods, "podGroups": pgs,
            "queues": [{"name": "q1", "weight": 1}, {"name": "q2", "weight": 1}],
            "actions": ["reclaim", "allocate", "backfill", "preempt"]}


def check_kat(fx):
    """The hand-derived rows of a KAT (expected.victim_why,
    tests/golden/make_kat_victim_why.py) after the fixture's actions."""
    modes = {"preempt_jobs": _abi.VMODE_PREEMPT_JOBS, "preempt_tasks": _abi.VMODE_PREEMPT_TASKS,
             "reclaim": _abi.VMODE_RECLAIM}
    ssn, _ = open_with_reasons(fx)
    errs = []
    try:
        for name in fx.get("actions") or ["allocate"]:
            get_action(name).execute(ssn)
        names = ssn.flat.node_names
        for exp in fx["expected"]["victim_why"]:
            j = next(i for i, job in enumerate(ssn.jobs) if job.uid == exp["job"])
            (w,) = ssn.victim_reasons(modes[exp["mode"]], [j])
            got = dict(valid=w.valid, task=ssn.flat.task_objs[w.task].uid if w.valid else None, visited=w.visited,
                       queue_overused=w.queue_overused, count=list(w.count),
                       first_node=[names[n] if n >= 0 else None for n in w.first_node], fn_empty=list(w.fn_empty))
            want = dict(valid=1, task=exp["task"], visited=sum(exp["count"]), queue_overused=exp["queue_overused"],
                        count=exp["count"], first_node=exp["first_node"], fn_empty=exp["fn_empty"])
            errs += [f"{exp['mode']} for {exp['job']}: {k} is {got[k]}, hand-derived {want[k]}"
                     for k in want if got[k] != want[k]]
    finally:
        ssn.close()
    return errs


def why_fields(w):
    return (w.valid, w.task, w.visited, w.queue_overused, list(w.count), list(w.first_node), list(w.fn_empty))


def check_discard(fx, opts=None):
    """A fixture whose oracle cycle discards a statement after evicting (the
    node keeps its copy of the task Releasing, statement.go:81-108, and the
    job's next try sees that): the oracle's output cannot give the tables, so
    after every action the rows of the device-shaped path are compared with the
    rows host_why gives for the same session (KBG_HOST_VICTIM_WHY, read per
    call), every row must account for every node, and the cycle must end as
    the oracle's. Returns (errors, seen)."""
    import os
    actions = fx.get("actions") or ["allocate"]
    ref_full = run_oracle(fx)
    assert ref_full["status"] == "ok", ref_full.get("error")
    assert not discard_free(fixture_mirror(fx), ref_full), "the oracle's cycle discards nothing: not a discard case"
    ssn, binder = open_with_reasons(fx, opts)
    errs, seen = [], dict(count=[0] * wr.N_CAUSES, fn_empty=[0, 0, 0])
    try:
        status = "ok"
        for name in actions:
            status = get_action(name).execute(ssn).status
            for mode in MODES:
                dev = ssn.victim_reasons(mode)
                os.environ["KBG_HOST_VICTIM_WHY"] = "1"
                try:
                    host = ssn.victim_reasons(mode)
                finally:
                    del os.environ["KBG_HOST_VICTIM_WHY"]
                for j, (a, b) in enumerate(zip(dev, host)):
                    if why_fields(a) != why_fields(b):
                        errs.append(f"after {name}, mode {mode}, job {j}: device path {why_fields(a)}, "
                                    f"host path {why_fields(b)}")
                    if a.valid and (a.visited != len(ssn.nodes) or sum(a.count) != a.visited):
                        errs.append(f"after {name}, mode {mode}, job {j}: visited {a.visited}, sum {sum(a.count)}, "
                                    f"{len(ssn.nodes)} nodes")
                    if a.valid:
                        seen["count"] = [x + y for x, y in zip(seen["count"], a.count)]
                        seen["fn_empty"] = [x + y for x, y in zip(seen["fn_empty"], a.fn_empty)]
        try:
            compare_outputs(ref_full, session_output(ssn, binder.binds, status))
        except AssertionError as e:
            errs.append(f"the cycle with calls in between differs from the oracle's: {e}")
    finally:
        ssn.close()
    return errs, seen
