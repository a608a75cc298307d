"""The four query calls after an update, from the references alone: no kbg
library is loaded here. `reference_points` gives, for a fixture in a session
order and a list of actions, the rows kbg_task_reasons, kbg_task_headroom and
kbg_victim_reasons must return before the first action and after each one,
with tasks by uid, jobs by uid and nodes by name. They come from
  - the Python cache of the fixture (its snapshot in the session's order),
  - the oracle's output of each action prefix,
  - tests/task_why_session.py, tests/headroom_session.py and
    tests/victim_why_session.py's reference builders.
tests/query_update_session.py compares a library's rows with these;
tests/test_query_update_ref.py reads the claims of the committed cases off them
and shows that the comparator notices a stale session's rows."""
from types import SimpleNamespace

import headroom_session as hs
import reasons_ref as rr
import task_why_session as ts
import victim_why_ref as wr
import victim_why_session as ws
from helpers import run_oracle
from kbgpu import _abi
from kbgpu.cache import FakeBinder, cache_from_fixture
from kbgpu.fixture import _OrderedCache, fixture_tiers

LIMITS = (1, 64)
MODES = ws.MODES
CONTENDED_ACTIONS = ["reclaim", "allocate", "backfill", "preempt"]


def view_of(cache, order, fx):
    """What the reference builders read of a session, from the Python cache
    alone: the snapshot in `order` (names the cache no longer holds are
    ignored, new ones follow in the cache's own order)."""
    snap = _OrderedCache(cache, {"sessionOrder": order}).snapshot()
    tasks = [t for j in snap.jobs for t in j.tasks.values()]
    return SimpleNamespace(jobs=snap.jobs, queues=snap.queues, nodes=snap.nodes, tiers=fixture_tiers(fx),
                           flat=SimpleNamespace(task_objs=tasks, node_names=[n.name for n in snap.nodes]))


def order_of(view):
    return {"jobs": [j.uid for j in view.jobs], "nodes": [n.name for n in view.nodes],
            "queues": [q.uid for q in view.queues]}


def fixture_view(fx, order=None):
    return view_of(cache_from_fixture(fx, FakeBinder()), order or fx.get("sessionOrder") or {}, fx)


def actions_of(fx):
    return list(fx.get("actions") or ["allocate"])


def _name(names, n):
    return names[n] if n >= 0 else None


def name_task_rows(rows, uid_of, names):
    """{task uid: kbg_task_why row with its first nodes by name}; `rows`: {task index: row}."""
    return {uid_of(t): dict(r, task=uid_of(t), first_node=[_name(names, n) for n in r["first_node"]])
            for t, r in rows.items()}


def name_room_rows(rows, uid_of, names):
    return {uid_of(t): dict(r, task=uid_of(t), first_node=_name(names, r["first_node"])) for t, r in rows.items()}


def reference_points(fx, order=None, actions=None):
    """[point]: "before", then one per action. A point holds `when`, `ref` (the
    oracle's output of the prefix; the snapshot's own state before), `task`
    ({uid: row}), `room` ({limit: {uid: row}}) and `victim` ({mode: {job uid:
    row}}; None before the first action, where the call is refused). `task`
    and `room` are None where the references cannot say them (a cycle with
    host ports or pod affinity that discards a statement after evicting), and
    `victim` wherever a statement was discarded (tests/victim_why_session.py)
    and on fixtures with host ports or pod affinity, stages its tables lack."""
    actions = actions_of(fx) if actions is None else list(actions)
    fx = dict(fx, sessionOrder=order) if order else fx
    view = fixture_view(fx)
    snap = ts.OpenSnap(view)
    rules = ws.plugin_rules(view.tiers)
    names = view.flat.node_names
    uid_of = lambda t: view.flat.task_objs[t].uid  # noqa: E731
    stagey = ts.has_pod_affinity(fx) or ts.has_host_ports(fx)
    points = []
    for k in range(len(actions) + 1):
        ref = snap.state if k == 0 else run_oracle(dict(fx, actions=actions[:k]))
        if k and ref["status"] != "ok":
            raise ValueError(f"the oracle ends {ref['status']} after {actions[:k]}: pick another fixture")
        clean = k == 0 or ws.discard_free(snap.mirror, ref)
        pt = dict(when="before" if k == 0 else actions[k - 1], ref=ref, task=None, room=None, victim=None)
        if clean or not stagey:
            pt["task"] = name_task_rows(ts.expected_rows(snap, fx, ref, rules), uid_of, names)
            pt["room"] = {lim: name_room_rows(hs.expected_rows(snap, fx, ref, rules, lim), uid_of, names)
                          for lim in LIMITS}
        if k and clean and not stagey:  # (the victim reference has no host-port or pod-affinity stage)
            pt["victim"] = {mode: victim_rows(snap.mirror, ref, rules, mode, uid_of, names) for mode in MODES}
        points.append(pt)
    return SimpleNamespace(points=points, view=view, snap=snap, rules=rules, fx=fx, actions=actions)


def victim_rows(m, ref, rules, mode, uid_of, names, job_min=None):
    """{job uid: row} of one kbg_victim_reasons call (`job_min`: MinAvailable per
    job instead of the mirror's, for the stale stand-in of the comparator's test)."""
    c, owners, tasks, over = ws.tables(m, ref, rules, mode)
    if job_min is not None:
        c.j_min = list(job_min)
    out = {}
    for r, j, t, o in zip(wr.rows(c), owners, tasks, over):
        out[m.job_uids[j]] = dict(task=uid_of(t), visited=sum(r["count"]), queue_overused=o, count=list(r["count"]),
                                  first_node=[_name(names, n) for n in r["first_node"]], fn_empty=list(r["fn_empty"]))
    return out


def job_reason_row(refs, log, task_uid, before):
    """(visited, count, first node names) of kbg_job_reasons for the task evaluated after log[:before]."""
    visited, count, first = rr.job_reasons(refs.fx, refs.view.nodes, log, task_uid, before, refs.rules["predicates"])
    return visited, count, [_name(refs.view.flat.node_names, n) for n in first]


# ----------------------------------------------------------------- comparator
def compare_point(want, got, aff, tag):
    """Differences between a reference point and a library's named rows of the
    same point (`got`: task, room and victim as reference_points names them,
    only the valid rows). Returns (errors, rows compared)."""
    errs, said = [], 0
    if want["task"] is not None:
        errs += ts.compare_rows(want["task"], list(got["task"].values()), aff, f"{tag}: kbg_task_reasons")
        said += len(want["task"])
        for lim in LIMITS:
            errs += hs.compare_rows(want["room"][lim], list(got["room"][lim].values()), aff,
                                    f"{tag}: kbg_task_headroom, limit {lim}")
            said += len(want["room"][lim])
    if want["victim"] is not None:
        if got["victim"] is None:
            errs.append(f"{tag}: kbg_victim_reasons was refused")
        else:
            for mode in MODES:
                w, g = want["victim"][mode], got["victim"][mode]
                if sorted(w) != sorted(g):
                    errs.append(f"{tag}: mode {mode}: jobs with a row {sorted(g)}, reference {sorted(w)}")
                    continue
                for j in w:
                    errs += [f"{tag}: mode {mode}, job {j}: {k} is {g[j][k]}, reference {w[j][k]}"
                             for k in w[j] if g[j][k] != w[j][k]]
                said += len(w)
    elif want["when"] == "before" and got["victim"] is not None:
        errs.append(f"{tag}: kbg_victim_reasons answered before the cycle's first action")
    return errs, said


def point_as_rows(pt):
    """A reference point in the shape compare_point takes a library's rows in."""
    return dict(task=pt["task"], room=pt["room"], victim=pt["victim"])


assert _abi.ROOM_MAX_LIMIT >= max(LIMITS)
