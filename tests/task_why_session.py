"""Session-level checks of kbg_task_reasons, shared by the hostsim tests
(tests/test_hostsim_task_why.py, through tests/task_why_worker.py) and the
device tests (tests/test_task_why_gpu.py).

`check_fixture` opens a session with reasons and, for each action prefix,
runs the prefix and asks for the rows of every Pending task. The expected rows
are built here without the library and without what the actions' replay
leaves in the Python mirror (everything of the mirror is copied at open):
  - node Idle, Releasing and pod counts from the ORACLE's output of the same
    prefix (kbref run on the fixture with the action list cut there);
  - the Pending tasks and the pods a node holds from the mirror at open plus
    the oracle's decisions, for the host-port stage;
  - the stages from reasons_ref.first_failing_stage (the pod cap from the
    oracle's pod count, ahead of it);
  - the resource test and FitDelta in Python (tests/task_why_ref.py).
reasons_ref has no inter-pod affinity stage. That stage is the predicates
plugin's last (predicates.go:185-198), so on a session with pod affinity the
nodes under causes 0..4 are exactly the reference's, and the nodes the
reference puts under 6, 7 and 8 are under 5, 6, 7 or 8: the counts of 0..4
and their first nodes are compared exactly, and count[5..8] by their sum.
Such sessions take the host path whole, so the two paths' comparison says
nothing there; tests/golden/kat_task_why_host.json holds hand-derived
host-port and pod-affinity rows instead.

A statement discarded after evicting leaves a node without the task's copy
(statement.go:81-108), which neither the oracle's log nor its node rows show;
on seeds with host ports or pod affinity the stage then depends on pods the
fixture and the log cannot give, so `check_fixture` builds no expected rows
there (victim_why_session.discard_free on the mirror at open tells such seeds
from node Releasing) and checks the invariants alone. The seed lists (tests/task_why_worker.py
SEEDS) were picked with the oracle so that at most a quarter of a generator's
seeds are skipped this way; the callers assert it from the `skipped` each case
reports."""
import os

import reasons_ref as rr
import task_why_ref as tr
import victim_why_session as ws
from helpers import run_oracle
from kbgpu import _abi
from kbgpu.api import PENDING
from kbgpu.fixture import pending_message, run_fixture
from kbgpu.framework import get_action

PREFIXES = (["allocate"], ["allocate", "backfill"], ["reclaim", "allocate", "backfill", "preempt"])


def seeded_fixture(kind, seed):
    from kbgpu import synth
    if kind == "random":
        return synth.random_fixture(seed)
    if kind == "contended":
        return synth.contended_fixture(seed)
    if kind == "ports":
        return synth.contended_fixture(seed, ports=0.3)
    return synth.contended_fixture(seed, aff=0.4, ports=0.2)


def has_pod_affinity(fx):
    return any((p.get("affinity") or {}).get(k) for p in fx["pods"] for k in ("podAffinity", "podAntiAffinity"))


def has_host_ports(fx):
    return any(rr._ports(p) for p in fx["pods"])


def empty(req):
    return all(req[d] < tr.MIN[d] for d in range(3))  # Resource.IsEmpty (resource_info.go:58-60)


class OpenSnap:
    """What the expected rows take from the Python cache mirror, copied at
    open, before any action's replay changes it: the Pending tasks, the pods
    each node holds, the nodes' own objects and the discard detection's Mirror."""

    def __init__(self, ssn):
        self.mirror = ws.Mirror(ssn)
        job_queue = {j.uid: j.queue for j in ssn.jobs}
        self.pending = [(t, obj.uid, [float(v) for v in obj.resreq.as_tuple()], obj.pod, job_queue[obj.job])
                        for t, obj in enumerate(ssn.flat.task_objs) if obj is not None and obj.status == PENDING]
        self.held = [{k: t.pod for k, t in n.tasks.items()} for n in ssn.nodes]
        self.nodes = [(n.name, n.node, n.allocatable.max_task_num) for n in ssn.nodes]
        self.state = dict(decisions=[], queues=None,  # the oracle's output rows of a cycle without actions
                          nodes=[dict(name=n.name, idle=n.idle.as_tuple(), releasing=n.releasing.as_tuple(),
                                      ntasks=len(n.tasks)) for n in ssn.nodes])


def expected_rows(snap, fx, ref, rules):
    """{task index: row} of every task Pending after the oracle's prefix
    (ref: its output; snap.state: no action yet, queue_overused not compared)."""
    pods = {p["uid"]: p for p in fx["pods"]}
    decided = {d["task"] for d in ref["decisions"]}
    by_name = {n["name"]: n for n in ref["nodes"]}
    held = [dict(h) for h in snap.held]  # a decision whose key the node holds leaves it as it is (node_info.go:101-106)
    index = {name: i for i, (name, _, _) in enumerate(snap.nodes)}
    for d in ref["decisions"]:
        held[index[d["node"]]].setdefault(rr.pod_key(pods[d["task"]]), pods[d["task"]])
    queues = {q["uid"]: q for q in ref["queues"] or []}
    out = {}
    for t, uid, req, pod, queue in snap.pending:
        if uid in decided:
            continue
        row = dict(tr.empty_row(), best_effort=empty(req), visited=len(snap.nodes))
        for i, (name, node, max_task_num) in enumerate(snap.nodes):
            st = by_name[name]
            idle, rel = [float(v) for v in st["idle"]], [float(v) for v in st["releasing"]]
            k, short = None, [False] * 3
            if rules["predicates"]:
                if node is None:
                    k = tr.PANIC
                elif max_task_num <= st["ntasks"]:
                    k = tr.POD_CAP
                else:
                    s = rr.first_failing_stage(pod, node, 1 << 30, held[i])
                    k = s if s >= 0 else None
            if k is None:
                if row["best_effort"] or tr.less_equal(req, idle):
                    k = tr.FITS_IDLE
                else:
                    k = tr.FITS_RELEASING if tr.less_equal(req, rel) else tr.SHORT
                    short = tr.fit_delta_negative(idle, req)
            row["count"][k] += 1
            if row["first_node"][k] < 0:
                row["first_node"][k] = i
            for d in range(3):
                row["idle_short"][d] += bool(short[d])
        q = queues.get(queue)  # Overused (proportion.go:188-194): only queues with an attr
        row["queue_overused"] = bool(rules["proportion"] and q is not None and
                                     tr.less_equal([float(v) for v in q["deserved"]], [float(v) for v in q["allocated"]]))
        if ref["queues"] is None:
            row["queue_overused"] = None
        out[t] = row
    return out


def compare_rows(want, got, aff, tag):
    errs = []
    if sorted(want) != sorted(r["task"] for r in got):
        return [f"{tag}: rows of tasks {sorted(r['task'] for r in got)}, reference {sorted(want)}"]
    for g in got:
        w = want[g["task"]]
        keys = ("best_effort", "visited") + (() if w["queue_overused"] is None else ("queue_overused",)) + \
            (() if aff else ("count", "first_node", "idle_short"))
        errs += [f"{tag}: task {g['task']}: {k} is {g[k]}, reference {w[k]}" for k in keys if g[k] != w[k]]
        if aff:  # (module docstring) the stages before pod affinity exactly, the rest by its sum
            if g["count"][:5] != w["count"][:5] or g["first_node"][:5] != w["first_node"][:5]:
                errs.append(f"{tag}: task {g['task']}: stages 0..4 are {g['count'][:5]} at {g['first_node'][:5]}, "
                            f"reference {w['count'][:5]} at {w['first_node'][:5]}")
            if sum(g["count"][5:9]) != sum(w["count"][5:9]) or g["count"][9] != w["count"][9]:
                errs.append(f"{tag}: task {g['task']}: count {g['count']}, reference {w['count']} before pod affinity")
    return errs


def host_rows(ssn, tasks=None):
    os.environ["KBG_HOST_TASK_WHY"] = "1"
    try:
        return ssn.task_reasons(tasks)
    finally:
        del os.environ["KBG_HOST_TASK_WHY"]


def accounting(ssn, rows, tag):
    """Every row accounts for every node, and the device-shaped path equals the host path."""
    errs = []
    n_nodes = len(ssn.nodes)
    for r in rows:
        if not r["valid"]:
            errs.append(f"{tag}: task {r['task']} of the mirror's Pending tasks has no row")
        elif not (sum(r["count"]) == r["visited"] == n_nodes):
            errs.append(f"{tag}: task {r['task']}: sum {sum(r['count'])}, visited {r['visited']}, {n_nodes} live nodes")
        elif not isinstance(pending_message(r), str) or str(n_nodes) not in pending_message(r):
            errs.append(f"{tag}: task {r['task']}: message {pending_message(r)!r}")
    host = host_rows(ssn)
    if host != rows:
        bad = [(a, b) for a, b in zip(rows, host) if a != b][:3]
        errs.append(f"{tag}: the device-shaped path differs from KBG_HOST_TASK_WHY=1: {bad}")
    return errs


def invariants(ssn, fx, rows, prefix, tag):
    errs = accounting(ssn, rows, tag)
    n_nodes, aff = len(ssn.nodes), has_pod_affinity(fx)
    by_task = {r["task"]: r for r in rows}
    n_log = len(ssn.decisions)
    for j, job in enumerate(ssn.jobs):
        why = ssn.job_reasons(j)
        st = ssn.job_state(j)
        if not why.valid or st.ready or why.task not in by_task:
            continue  # (a task with a row is still Pending: it found no node)
        r = by_task[why.task]
        # Without pod affinity a node only loses feasibility during allocate, so a task that failed at its
        # evaluation point fits nowhere at the end. With pod affinity a pod placed later can satisfy the task's
        # own affinity term on a node that turned it away before (predicates.go:185-198): not asserted there.
        if prefix == ["allocate"] and (r["count"][tr.FITS_IDLE] or r["count"][tr.FITS_RELEASING]) and not aff:
            errs.append(f"{tag}: job {job.uid}: its failed task {why.task} fits {r['count'][6:8]} nodes now")
        if why.before != n_log or why.visited != n_nodes:
            continue
        if list(why.count) != r["count"][:6] or list(why.first_node) != r["first_node"][:6]:
            errs.append(f"{tag}: job {job.uid}: stages {r['count'][:6]} at {r['first_node'][:6]}, kbg_job_reasons "
                        f"{list(why.count)} at {list(why.first_node)}")
        if st.fit_valid and (st.fit_nodes, [st.fit_cpu, st.fit_memory, st.fit_gpu]) != \
                (r["count"][tr.FITS_RELEASING] + r["count"][tr.SHORT], r["idle_short"]):
            errs.append(f"{tag}: job {job.uid}: FitError {st.fit_nodes} nodes {[st.fit_cpu, st.fit_memory, st.fit_gpu]}, "
                        f"row {r['count'][7] + r['count'][8]} nodes {r['idle_short']}")
    if "backfill" in prefix and not aff:
        for r in rows:
            if r["valid"] and r["best_effort"] and r["count"][tr.FITS_IDLE]:
                errs.append(f"{tag}: BestEffort task {r['task']} is Pending after backfill with "
                            f"{r['count'][tr.FITS_IDLE]} nodes open")
    return errs


def run_actions(ssn, names):
    """Runs the actions in order; an action the reference would panic in ends the list ("ref_panic")."""
    status = "ok"
    for name in names:
        try:
            status = get_action(name).execute(ssn).status
        except _abi.KbgError as e:
            if e.status != "ref_panic":
                raise
            return "ref_panic"
    return status


def log_of(ssn):
    return [tuple(d) for d in ssn.decisions], [(t.uid, by.uid, a) for t, by, a in ssn.evictions]


# the actions that may still follow each prefix (reclaim runs first or not at all, backfill before preempt)
REST = {("allocate",): ["backfill", "preempt"], ("allocate", "backfill"): ["preempt"],
        ("reclaim", "allocate", "backfill", "preempt"): []}


def check_fixture(fx, opts=None):
    """Every check of one fixture over the three prefixes. The session is
    asked after every action of the prefix (between actions: the accounting
    and the two paths; after the prefix: everything), then runs the actions of
    REST, and its decision and eviction logs must equal those of a session
    that ran the same actions without a call. Returns (errors, seen, skipped):
    `seen` sums the expected counts per cause, `skipped` says that for some
    prefix no expected rows were built (module docstring). A prefix the oracle
    does not end ok is an error: the seed lists hold none."""
    errs, seen, skipped = [], [0] * tr.N_CAUSES, False
    aff = has_pod_affinity(fx)
    for prefix in PREFIXES:
        tag = "+".join(prefix)
        fxp = dict(fx, actions=list(prefix))
        ref = run_oracle(fxp)
        if ref["status"] != "ok":
            errs.append(f"{tag}: the oracle ends {ref['status']}: pick another fixture")
            continue
        rest = REST[tuple(prefix)]
        ssn, _ = ws.open_with_reasons(fxp, opts)
        try:
            snap = OpenSnap(ssn)
            rules = ws.plugin_rules(ssn.tiers)
            if prefix is PREFIXES[0]:  # before the first action: the snapshot
                errs += compare_rows(expected_rows(snap, fx, snap.state, rules), ssn.task_reasons(), aff, "at open")
            for k, name in enumerate(prefix):
                if run_actions(ssn, [name]) == "ref_panic":
                    errs.append(f"{tag}: {name} ends ref_panic where the oracle ends ok")
                if k + 1 < len(prefix):
                    errs += accounting(ssn, ssn.task_reasons(), f"{tag}, after {name}")
            rows = ssn.task_reasons()
            errs += invariants(ssn, fx, rows, list(prefix), tag)
            if (aff or has_host_ports(fx)) and not ws.discard_free(snap.mirror, ref):
                skipped = True
            else:
                want = expected_rows(snap, fx, ref, rules)
                errs += compare_rows(want, rows, aff, tag)
                for w in want.values():
                    seen = [a + b for a, b in zip(seen, w["count"])]
            if rows:  # a subset asked by index, in the order asked
                pick = [rows[-1]["task"], rows[0]["task"]]
                if ssn.task_reasons(pick) != [rows[-1], rows[0]]:
                    errs.append(f"{tag}: tasks {pick} asked by index differ from their rows of the whole call")
            with_calls = (run_actions(ssn, rest), log_of(ssn))
        finally:
            ssn.close()
        plain, _ = ws.open_with_reasons(fxp, opts)
        try:
            if (run_actions(plain, list(prefix) + rest), log_of(plain)) != with_calls:
                errs.append(f"{tag}: the logs of {list(prefix) + rest} differ with the calls in between")
        finally:
            plain.close()
    return errs, seen, skipped


def check_refusals(fx):
    """No reasons: KBG_E_INVALID. A task that is not Pending: valid == 0. An index out of range: KBG_E_INVALID."""
    errs = []
    got, ssn = run_fixture(dict(fx, actions=["allocate"]), {})
    try:
        try:
            ssn.task_reasons([0])
            errs.append("reasons = 0: the call did not fail")
        except _abi.KbgError as e:
            if e.status != "invalid":
                errs.append(f"reasons = 0: {e}")
    finally:
        ssn.close()
    ssn, _ = ws.open_with_reasons(fx)
    try:
        run_actions(ssn, ["allocate"])
        placed = [d[0] for d in ssn.decisions]
        assert placed, "the fixture's allocate places nothing"
        row = ssn.task_reasons([placed[0]])[0]
        if row["valid"] or any(row["count"]) or row["visited"]:
            errs.append(f"a placed task has the row {row}")
        for bad in (-1, len(ssn.flat.task_objs)):
            try:
                ssn.task_reasons([bad])
                errs.append(f"task index {bad}: the call did not fail")
            except _abi.KbgError as e:
                if e.status != "invalid":
                    errs.append(f"task index {bad}: {e}")
        if _abi.lib().kbg_task_reasons(ssn.handle, None, 1, (_abi.kbg_task_why * 1)()) != _abi.KBG_E_INVALID:
            errs.append("tasks == NULL: the call did not return KBG_E_INVALID")
    finally:
        ssn.close()
    return errs


def check_resident(fx0, seed, rounds, opts=None):
    """A resident session (kbg_session_reset, kbg_session_update) against a
    fresh session opened on the round's fixture: the rows before the round's
    first action and after its actions, task by uid and node by name."""
    import ctypes
    errs = []
    ssn = None
    L = _abi.lib()

    def named(s, rows):
        names = s.flat.node_names
        return sorted((s.flat.task_objs[r["task"]].uid, r["valid"], r["visited"], r["best_effort"], r["queue_overused"],
                       tuple(r["count"]), tuple(names[n] if n >= 0 else None for n in r["first_node"]),
                       tuple(r["idle_short"])) for r in rows)

    said = 0  # rows compared (the resident mirror's statuses are not replayed: asked by the fresh session's uids)
    try:
        for r, (fx, changes, ref_full) in enumerate(ws.resident_rounds(fx0, seed, rounds)):
            actions = fx.get("actions") or ["allocate"]
            if ssn is None:
                ssn, _ = ws.open_with_reasons(fx, opts)
            else:
                _abi.check(L.kbg_session_reset(ssn.handle))
                ssn.update(changes)
            fresh, _ = ws.open_with_reasons(fx, opts)
            try:
                uid_task = {t.uid: i for i, t in enumerate(ssn.flat.task_objs) if t is not None}
                for when in ("before", "after"):
                    if when == "after":
                        cap = max(1, len(ssn.flat.task_objs))
                        buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
                        for name in actions:
                            _abi.check(getattr(L, ws.ENTRY[name])(ssn.handle, buf, cap, ctypes.byref(n)))
                        run_actions(fresh, actions)
                    want = fresh.task_reasons()
                    mine = [uid_task[fresh.flat.task_objs[w["task"]].uid] for w in want]
                    got = ssn.task_reasons(mine)
                    if named(fresh, want) != named(ssn, got):
                        errs.append(f"round {r}, {when} the actions: the resident session's rows differ from a fresh "
                                    f"session's")
                    said += len(want)
            finally:
                fresh.close()
    finally:
        if ssn is not None:
            ssn.close()
    if not said:
        errs.append("no round held a Pending task: the case says nothing")
    return errs


def check_kat(fx):
    """The hand-derived rows of a KAT of tests/golden/make_kat_task_why.py, at open, on both paths."""
    ssn, _ = ws.open_with_reasons(fx)
    errs = []
    try:
        names = ssn.flat.node_names
        uid_task = {t.uid: i for i, t in enumerate(ssn.flat.task_objs)}
        for exp in fx["expected"]["task_why"]:
            for rows_of in (ssn.task_reasons, lambda ts: host_rows(ssn, ts)):
                (g,) = rows_of([uid_task[exp["task"]]])
                got = dict(valid=g["valid"], best_effort=g["best_effort"], queue_overused=g["queue_overused"],
                           visited=g["visited"], count=g["count"], idle_short=g["idle_short"],
                           first_node=[names[n] if n >= 0 else None for n in g["first_node"]],
                           message=pending_message(g))
                want = dict(valid=True, best_effort=exp["best_effort"], queue_overused=exp["queue_overused"],
                            visited=sum(exp["count"]), count=exp["count"], idle_short=exp["idle_short"],
                            first_node=exp["first_node"], message=exp["message"])
                errs += [f"{exp['task']}: {k} is {got[k]}, hand-derived {want[k]}" for k in want if got[k] != want[k]]
    finally:
        ssn.close()
    return errs
