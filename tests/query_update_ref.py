"""The seven query calls after an update, from the references alone: no kbg
library is loaded here. `reference_points` gives, for a fixture in a session
order and a list of actions, the rows kbg_task_reasons, kbg_task_headroom,
kbg_victim_reasons, kbg_job_fit, kbg_node_reasons and kbg_node_drain must
return before the first action and after each one, with tasks by uid, jobs by
uid and nodes by name (kbg_job_reasons is held to reasons_ref by the caller:
`job_reason_row`). They come from
  - the Python cache of the fixture (its snapshot in the session's order),
  - the oracle's output of each action prefix,
  - the reference builders of tests/task_why_session.py,
    tests/headroom_session.py, tests/victim_why_session.py,
    tests/job_fit_session.py, tests/node_why_session.py and
    tests/drain_session.py.
tests/query_update_session.py compares a library's rows with these;
tests/test_query_update_ref.py reads the claims of the committed cases off them
and shows that the comparator notices a stale session's rows."""
import copy
from types import SimpleNamespace

import drain_session as ds
import headroom_session as hs
import job_fit_session as js
import node_why_session as ns
import reasons_ref as rr
import task_why_session as ts
import victim_why_ref as wr
import victim_why_session as ws
from helpers import run_oracle
from kbgpu import _abi
from kbgpu.cache import FakeBinder, cache_from_fixture
from kbgpu.fixture import _OrderedCache, fixture_tiers

LIMITS = (1, 64)
FIT_LIMITS = (2, 512)  # kbg_job_fit's and kbg_node_drain's
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


def name_fit_rows(rows, job_uids, uid_of, names):
    """{job uid: kbg_job_fit row with its places as (task uid, node name or None, kind)}; `rows`: {job index: row}."""
    return {job_uids[j]: dict(r, valid=True, job=job_uids[j], first_unplaced=uid_of(r["first_unplaced"]),
                              places=[(uid_of(t), _name(names, n), k) for t, n, k in r["places"]])
            for j, r in rows.items()}


def name_node_rows(rows, uid_of, names):
    """{node name: kbg_node_reasons row with its first tasks by uid}; `rows`: one per node, in order."""
    return {names[r["node"]]: dict(r, node=names[r["node"]], first_task=[uid_of(t) for t in r["first_task"]])
            for r in rows}


def name_drain_rows(rows, uid_of, names):
    return {names[x]: dict(r, valid=True, node=names[x], first_unplaced=uid_of(r["first_unplaced"]),
                           places=[(uid_of(t), _name(names, n), k) for t, n, k in r["places"]])
            for x, r in rows.items()}


def with_job_min(snap, job_min):
    """`snap` with another MinAvailable per job (the stale stand-ins of the comparator's test)."""
    out = copy.copy(snap)
    out.job_min = list(job_min)
    return out


def in_numbers(snap, numbers):
    """`snap` with its Pending tasks numbered by `numbers` ({uid: index}): the
    lowest task of a cause in kbg_node_reasons is the lowest in the asked
    session's own numbering, which an in-place batch leaves as it was."""
    out = copy.copy(snap)
    out.pending = [(numbers[uid], uid, req, pod, queue) for _, uid, req, pod, queue in snap.pending]
    return out


def walk_rows(r, ref, fit_min=None, drain_min=None):
    """(fit, drain) of one point of `r` (a reference_points result) after the
    oracle's output `ref`, named. `fit_min`, `drain_min`: MinAvailable per job
    for the derived fields in place of the snapshot's own."""
    names = r.view.flat.node_names
    uid_of = lambda t: r.view.flat.task_objs[t].uid if t >= 0 else None  # noqa: E731
    fsnap = r.fsnap if fit_min is None else with_job_min(r.fsnap, fit_min)
    dsnap = r.dsnap if drain_min is None else with_job_min(r.dsnap, drain_min)
    fit = {lim: js.expected_rows(fsnap, r.fx, ref, r.rules, lim) for lim in FIT_LIMITS}
    if fit_min is not None:  # (the field itself is asked of the session's table, not derived)
        for rows in fit.values():
            for j, row in rows.items():
                row["min_available"] = r.fsnap.job_min[j]
    plain = {lim: ds.expected_rows(dsnap, r.fx, ref, r.rules, lim) for lim in FIT_LIMITS}
    cordon = ds.pick_cordon(plain[FIT_LIMITS[-1]])
    drain = {(lim, ()): name_drain_rows(plain[lim], uid_of, names) for lim in FIT_LIMITS}
    drain[(FIT_LIMITS[-1], tuple(names[c] for c in cordon))] = name_drain_rows(
        ds.expected_rows(dsnap, r.fx, ref, r.rules, FIT_LIMITS[-1], cordon), uid_of, names)
    return {lim: name_fit_rows(rows, r.fsnap.job_uids, uid_of, names) for lim, rows in fit.items()}, drain


def reference_points(fx, order=None, actions=None, task_numbers=None):
    """[point]: "before", then one per action. A point holds `when`, `ref` (the
    oracle's output of the prefix; the snapshot's own state before), `task`
    ({uid: row}), `room` ({limit: {uid: row}}) and `victim` ({mode: {job uid:
    row}}; None before the first action, where the call is refused). `task`
    and `room` are None where the references cannot say them (a cycle with
    host ports or pod affinity that discards a statement after evicting), and
    `victim` wherever a statement was discarded (tests/victim_why_session.py)
    and on fixtures with host ports or pod affinity, stages its tables lack.

    `fit` ({limit: {job uid: row}}, FIT_LIMITS), `node` ({node name: row}) and
    `drain` ({(limit, cordon by name): {node name: row}}: both limits without a
    cordon, and the higher with drain_session.pick_cordon of its uncordoned
    rows) follow the rules of their own modules' check_fixture: `node` is None
    where `task` is, `fit` and `drain` on fixtures with pod affinity (the walks'
    reference has no such stage) and after a discarded statement on fixtures
    with host ports. `nodes` lists the node names in the view's order.
    `task_numbers` ({uid: index}): the asked session's task numbering where it
    is not the view's (`in_numbers`)."""
    actions = actions_of(fx) if actions is None else list(actions)
    fx = dict(fx, sessionOrder=order) if order else fx
    view = fixture_view(fx)
    snap = ts.OpenSnap(view)
    rules = ws.plugin_rules(view.tiers)
    names = view.flat.node_names
    uid_of = lambda t: view.flat.task_objs[t].uid if t >= 0 else None  # noqa: E731
    aff = ts.has_pod_affinity(fx)
    stagey = aff or ts.has_host_ports(fx)
    out = SimpleNamespace(view=view, snap=snap, rules=rules, fx=fx, actions=actions, fsnap=js.Snap(view),
                          dsnap=ds.Snap(view))
    nsnap = snap if task_numbers is None else in_numbers(snap, task_numbers)
    by_number = None if task_numbers is None else {i: u for u, i in task_numbers.items()}
    node_uid = uid_of if by_number is None else (lambda t: by_number[t] if t >= 0 else None)
    points = []
    for k in range(len(actions) + 1):
        ref = snap.state if k == 0 else run_oracle(dict(fx, actions=actions[:k]))
        if k and ref["status"] != "ok":
            raise ValueError(f"the oracle ends {ref['status']} after {actions[:k]}: pick another fixture")
        clean = k == 0 or ws.discard_free(snap.mirror, ref)
        pt = dict(when="before" if k == 0 else actions[k - 1], ref=ref, task=None, room=None, victim=None,
                  fit=None, node=None, drain=None, nodes=list(names))
        if clean or not stagey:
            pt["task"] = name_task_rows(ts.expected_rows(snap, fx, ref, rules), uid_of, names)
            pt["room"] = {lim: name_room_rows(hs.expected_rows(snap, fx, ref, rules, lim), uid_of, names)
                          for lim in LIMITS}
            pt["node"] = name_node_rows(ns.expected_rows(nsnap, fx, ref, rules), node_uid, names)
        if k and clean and not stagey:  # (the victim reference has no host-port or pod-affinity stage)
            pt["victim"] = {mode: victim_rows(snap.mirror, ref, rules, mode, uid_of, names) for mode in MODES}
        if not aff and (clean or not ts.has_host_ports(fx)):
            pt["fit"], pt["drain"] = walk_rows(out, ref)
        points.append(pt)
    out.points = points
    return out


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
def compare_point(want, got, aff, tag, counts=None):
    """Differences between a reference point and a library's named rows of the
    same point (`got`: task, room, victim, fit, node and drain as
    reference_points names them, only the valid rows). Returns (errors, rows
    compared); `counts` ({"fit", "node", "drain": rows}) is added to."""
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
    new = {"fit": 0, "node": 0, "drain": 0}
    # the three later calls, each through its own module's comparator; node names back to the view's indices
    at = {name: i for i, name in enumerate(want["nodes"])}
    if want["fit"] is not None:
        if got.get("fit") is None:
            errs.append(f"{tag}: kbg_job_fit was refused")
        else:
            for lim in FIT_LIMITS:
                errs += js.compare_rows(want["fit"][lim], list(got["fit"][lim].values()),
                                        f"{tag}: kbg_job_fit, limit {lim}")
                new["fit"] += len(want["fit"][lim])
    if want["node"] is not None:
        if got.get("node") is None:
            errs.append(f"{tag}: kbg_node_reasons was refused")
        elif sorted(got["node"]) != sorted(want["node"]):
            errs.append(f"{tag}: kbg_node_reasons: rows of {sorted(got['node'])}, reference {sorted(want['node'])}")
        else:
            errs += ns.compare_rows([dict(want["node"][name], node=at[name]) for name in want["nodes"]],
                                    [dict(got["node"][name], node=at[name]) for name in want["nodes"]], aff,
                                    f"{tag}: kbg_node_reasons")
            new["node"] += len(want["node"])
    if want["drain"] is not None:
        if got.get("drain") is None:
            errs.append(f"{tag}: kbg_node_drain was refused")
        else:
            for key, rows in want["drain"].items():
                if key not in got["drain"]:
                    errs.append(f"{tag}: kbg_node_drain was not asked at limit {key[0]} with cordon {key[1]}")
                    continue
                errs += ds.compare_rows(rows, list(got["drain"][key].values()),
                                        f"{tag}: kbg_node_drain, limit {key[0]}, cordon {key[1]}")
                new["drain"] += len(rows)
    if counts is not None:
        for k, v in new.items():
            counts[k] = counts.get(k, 0) + v
    return errs, said + sum(new.values())


def point_as_rows(pt):
    """A reference point in the shape compare_point takes a library's rows in."""
    return dict(task=pt["task"], room=pt["room"], victim=pt["victim"], fit=pt["fit"], node=pt["node"],
                drain=pt["drain"])


assert _abi.ROOM_MAX_LIMIT >= max(LIMITS)
