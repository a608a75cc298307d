"""The cases of tests/query_update_cases.py say something, and the comparator
of tests/query_update_ref.py would notice a stale session: both shown from the
references alone (fixtures, the oracle's output, the reference rows of S0 and
S1). No kbg library is loaded here.

Per case: Pending tasks before the first action after the update and after
the last one, and reference rows of S1 that differ from those of the session
before the update at the same point of the cycle, or the update is invisible
to the seven calls: some row of the four older calls, some row of
kbg_job_fit, kbg_node_reasons or kbg_node_drain (on the seeded cases some row
of each), and a drain walk that holds a pod.

Per family, over its cases, the claims its events can carry (CLAIMS): a node
that moved and is some row's first node, a deleted node that was one, a task
whose index moved, queue_overused flipping, the victims the gang plugin
protects changing with MinAvailable, a node moving between two predicate
stages, copies_idle changing under the same nodes_pass; and for the three
later calls a place on a node whose index moved, a place on a node the update
added, ready_after or jobs_short following MinAvailable, a (node, cause) count
of kbg_node_reasons moving between two predicate stages, a walked Running
pod landing elsewhere after a relabel (kbg_node_drain compiles such a pod's
class on its own), queue_overused of a fit row flipping.

The comparator is handed stand-ins for what a stale session would answer
(STALE for the four older calls, LATER_STALE for the three later ones, which
leave the older calls' rows right); each must be noticed on at least one
case, the later ones in the rows of the three later calls."""
import copy
from types import SimpleNamespace

import pytest

import drain_session as ds
import query_update_cases as qc
import query_update_ref as qr
import reasons_ref as rr
import task_why_session as ts
from update_events import fixture_after, replay

CASES = qc.all_cases()
# The thirteen claims, per family, less those its events cannot carry:
#   structural: node, PodGroup and queue adds and deletes set no MinAvailable of a job that stays
#     (gang_protection_changes, ready_after_follows_min_available) and update no node (stage_moves,
#     node_cause_moves, drained_pod_stage_moves);
#   in_place: JOB_UPDATE / QUEUE_SET and pod churn renumber nothing, add no node and touch no node's labels or
#     taints (moved_first_node, deleted_first_node, task_index_moved, stage_moves, place_on_moved_node,
#     place_on_new_node, node_cause_moves, drained_pod_stage_moves);
#   recompile: node updates alone add, delete and renumber nothing, and leave queues and MinAvailable as they are
#     (everything but stage_moves, copies_idle_alone, node_cause_moves and drained_pod_stage_moves);
#   chain: all thirteen.
CLAIMS = {
    "structural": ("moved_first_node", "deleted_first_node", "task_index_moved", "queue_overused_flips",
                   "copies_idle_alone", "place_on_moved_node", "place_on_new_node", "fit_queue_overused_flips"),
    "in_place": ("queue_overused_flips", "gang_protection_changes", "copies_idle_alone",
                 "ready_after_follows_min_available", "fit_queue_overused_flips"),
    "recompile": ("stage_moves", "copies_idle_alone", "node_cause_moves", "drained_pod_stage_moves"),
    "chain": ("moved_first_node", "deleted_first_node", "task_index_moved", "queue_overused_flips",
              "gang_protection_changes", "stage_moves", "copies_idle_alone", "place_on_moved_node",
              "place_on_new_node", "ready_after_follows_min_available", "node_cause_moves",
              "drained_pod_stage_moves", "fit_queue_overused_flips"),
}
STALE = ("rows0_unchanged", "first_node_old_numbers", "old_queue_overused", "old_min_available", "other_limit",
         "wrong_order")
# for kbg_job_fit, kbg_node_reasons and kbg_node_drain: S0's rows unchanged, places and first_task read in S0's
# numbering, S0's MinAvailable in ready_after / jobs_short, the cordon applied by S0's node indices, the rows of
# the other limit, each node answered with its neighbour's row, a walk that still holds a pod the update deleted
LATER_STALE = ("later_rows0_unchanged", "places_old_numbers", "later_old_min_available", "cordon_old_indices",
               "later_other_limit", "node_neighbour", "deleted_pod_walked")
LATER_CALLS = ("kbg_job_fit", "kbg_node_reasons", "kbg_node_drain")
# the cases drawn from a seed (the others are made by hand, each for the calls its docstring names)
SEEDED = {case for case in CASES if case.split("/")[1].rstrip("0123456789") in
          ("random", "contended", "ports", "affinity", "fuzz", "relabel")}


def case_references(build):
    """S0's references and, per round, the batch, the fixture after it and S1's references in the order the
    session takes (the old order, new names after it: tests/query_update_session.py checks that it does)."""
    fx0, rounds_of, _ = build()
    actions = qr.actions_of(fx0)
    r0 = qr.reference_points(fx0)
    order, done, rounds = qr.order_of(r0.view), [], []
    for changes_of in rounds_of:
        fx_now = fixture_after(fx0, done) if done else fx0
        ch = changes_of(qr.view_of(replay(fx0, done), order, fx0), fx_now)
        done.append(ch)
        fx1 = fixture_after(fx0, done)
        assert fx1 is not None, "no fixture says the cache after the events"
        order = qr.order_of(qr.view_of(replay(fx0, done), order, fx0))
        rounds.append(SimpleNamespace(changes=ch, fx=fx1, refs=qr.reference_points(fx1, order, actions)))
    return SimpleNamespace(fx0=fx0, r0=r0, rounds=rounds)


@pytest.fixture(scope="module")
def refs():
    return {case: case_references(build) for case, (_, build) in CASES.items()}


def pending_left(r, k):
    decided = {d["task"] for d in r.points[k]["ref"]["decisions"]}
    return sum(1 for _, uid, *_ in r.snap.pending if uid not in decided)


def rows_of(pt):
    return {k: pt[k] for k in ("task", "room", "victim") if pt[k] is not None}


def steps(c):
    """(references before, references after) of every round."""
    prev = c.r0
    for rnd in c.rounds:
        yield prev, rnd
        prev = rnd.refs


@pytest.mark.parametrize("case", sorted(CASES))
def test_case_says_something(refs, case):
    c = refs[case]
    last = c.rounds[-1].refs
    assert pending_left(last, 0) > 0 and pending_left(last, len(last.points) - 1) > 0
    # what a session that missed the update would answer at a point is what the references before it say there
    for prev, rnd in steps(c):
        pairs = [(rows_of(p0), rows_of(p1)) for p0, p1 in zip(prev.points, rnd.refs.points)]
        shared = [(a[k], b[k]) for a, b in pairs for k in a if k in b]
        assert shared, "the references say no rows of both S0 and S1"
        assert any(a != b for a, b in shared), "the update is invisible to the calls"
    # kbg_job_fit, kbg_node_reasons, kbg_node_drain: some row of theirs differs too, and on the seeded cases some
    # row of each of the three wherever its reference speaks (a hand-made batch is aimed at the calls it names)
    later = {what: [(p0[what], p1[what]) for prev, rnd in steps(c) for p0, p1 in zip(prev.points, rnd.refs.points)
                    if p0[what] is not None and p1[what] is not None] for what in ("fit", "node", "drain")}
    assert later["node"], "the references say no kbg_node_reasons rows of both S0 and S1"
    differs = {what: any(a != b for a, b in pairs) for what, pairs in later.items() if pairs}
    print(f"{case}: rows of S1 differ from S0's for {sorted(w for w, d in differs.items() if d)}")
    assert any(differs.values()), "the update is invisible to kbg_job_fit, kbg_node_reasons and kbg_node_drain"
    if case in SEEDED:
        assert all(differs.values()), f"the update is invisible to {sorted(w for w, d in differs.items() if not d)}"
    # some drain walk holds a pod (where the walks' reference is silent, pod affinity: some node holds a pod of
    # the session jobs in an AllocatedStatus, which is what the call walks)
    if any(pt["drain"] is not None for pt in last.points):
        assert any(r["walked"] > 0 for pt in last.points for rows in (pt["drain"] or {}).values()
                   for r in rows.values())
    else:
        assert ts.has_pod_affinity(c.rounds[-1].fx)
        assert any(e[0] is not None and e[2] in ds.MOVABLE for tasks in last.dsnap.order for e in tasks)


# ------------------------------------------------------------------- claims
def first_nodes(pt):
    out = set()
    for r in (pt["task"] or {}).values():
        out |= {n for n in r["first_node"] if n is not None}
    for rows in (pt["room"] or {}).values():
        out |= {r["first_node"] for r in rows.values() if r["first_node"] is not None}
    for rows in (pt["victim"] or {}).values():
        for r in rows.values():
            out |= {n for n in r["first_node"] if n is not None}
    return out


def claim_moved_first_node(a, rnd):
    n0, n1 = a.view.flat.node_names, rnd.refs.view.flat.node_names
    moved = {n for n in n1 if n in n0 and n0.index(n) != n1.index(n)}
    return bool(moved & set().union(*(first_nodes(pt) for pt in rnd.refs.points)))


def claim_deleted_first_node(a, rnd):
    gone = set(a.view.flat.node_names) - set(rnd.refs.view.flat.node_names)
    return bool(gone & first_nodes(a.points[-1]))


def claim_task_index_moved(a, rnd):
    i0 = {t.uid: i for i, t in enumerate(a.view.flat.task_objs)}
    i1 = {t.uid: i for i, t in enumerate(rnd.refs.view.flat.task_objs)}
    with_rows = lambda r: set().union(*((pt["task"] or {}).keys() for pt in r.points))  # noqa: E731
    return any(i0[u] != i1[u] for u in with_rows(a) & with_rows(rnd.refs))


def overused(pt):
    out = {("task", u): r["queue_overused"] for u, r in (pt["task"] or {}).items()}
    for mode, rows in (pt["victim"] or {}).items():
        out.update({("victim", mode, j): r["queue_overused"] for j, r in rows.items()})
    return out


def claim_queue_overused_flips(a, rnd):
    o0, o1 = overused(a.points[-1]), overused(rnd.refs.points[-1])
    return any(o0[k] is not None and o1[k] is not None and bool(o0[k]) != bool(o1[k]) for k in o0 if k in o1)


def stale_min_victims(a, rnd, k=-1):
    """S1's victim rows with S0's MinAvailable where the job was there, or None."""
    r1 = rnd.refs
    if r1.points[k]["victim"] is None:
        return None
    old = dict(zip(a.snap.mirror.job_uids, a.snap.mirror.job_min))
    mins = [old.get(u, m) for u, m in zip(r1.snap.mirror.job_uids, r1.snap.mirror.job_min)]
    uid_of = lambda t: r1.view.flat.task_objs[t].uid  # noqa: E731
    return {mode: qr.victim_rows(r1.snap.mirror, r1.points[k]["ref"], r1.rules, mode, uid_of, r1.view.flat.node_names,
                                 job_min=mins) for mode in qr.MODES}


def claim_gang_protection_changes(a, rnd):
    if not any(kind.startswith("pod_group") for kind, _ in rnd.changes):
        return False
    return any((stale := stale_min_victims(a, rnd, k)) is not None and stale != rnd.refs.points[k]["victim"]
               for k in range(1, len(rnd.refs.points)))


def claim_stage_moves(a, rnd):
    if not any(kind == "node_update" for kind, _ in rnd.changes):
        return False
    old = {n.name: n.node for n in a.view.nodes}
    for _, _, _, pod, _ in rnd.refs.snap.pending:
        for n in rnd.refs.view.nodes:
            if n.name in old and old[n.name] is not None and n.node is not None:
                s0, s1 = (rr.first_failing_stage(pod, node, 1 << 30, {}) for node in (old[n.name], n.node))
                if s0 >= 0 and s1 >= 0 and s0 != s1:
                    return True
    return False


def claim_copies_idle_alone(a, rnd):
    for k0, k1 in ((-1, -1), (0, 0), (-1, 0)):
        r0, r1 = a.points[k0]["room"], rnd.refs.points[k1]["room"]
        if r0 is None or r1 is None:
            continue
        for lim in qr.LIMITS:
            for u in set(r0[lim]) & set(r1[lim]):
                if r0[lim][u]["copies_idle"] != r1[lim][u]["copies_idle"] and \
                        r0[lim][u]["nodes_pass"] == r1[lim][u]["nodes_pass"]:
                    return True
    return False


# ------------------------------- claims of kbg_job_fit, kbg_node_reasons, kbg_node_drain
def places(pt):
    """{(call, question, row, task uid): (node name or None, kind)} of a point's fit and drain references."""
    out = {}
    for what in ("fit", "drain"):
        for key, rows in (pt[what] or {}).items():
            for name, r in rows.items():
                out.update({(what, key, name, t): (n, kind) for t, n, kind in r["places"]})
    return out


def placed_nodes(r):
    return {n for pt in r.points for n, _ in places(pt).values() if n is not None}


def claim_place_on_moved_node(a, rnd):
    n0, n1 = a.view.flat.node_names, rnd.refs.view.flat.node_names
    return bool({n for n in n1 if n in n0 and n0.index(n) != n1.index(n)} & placed_nodes(rnd.refs))


def claim_place_on_new_node(a, rnd):
    return bool((set(rnd.refs.view.flat.node_names) - set(a.view.flat.node_names)) & placed_nodes(rnd.refs))


def stale_min_walks(a, rnd, k):
    """S1's fit and drain rows at point k with S0's MinAvailable where the job was there, or None."""
    r1 = rnd.refs
    if r1.points[k]["fit"] is None:
        return None
    old = dict(zip(a.snap.mirror.job_uids, a.snap.mirror.job_min))
    mins = [old.get(u, m) for u, m in zip(r1.snap.mirror.job_uids, r1.snap.mirror.job_min)]
    return qr.walk_rows(r1, r1.points[k]["ref"], fit_min=mins, drain_min=mins)


def claim_ready_after_follows_min_available(a, rnd):
    for k in range(1, len(rnd.refs.points)):  # (before the first action the snapshot says no ready_num)
        if (stale := stale_min_walks(a, rnd, k)) is None:
            continue
        pt = rnd.refs.points[k]
        if any(stale[0][lim][j]["ready_after"] != r["ready_after"] for lim, rows in pt["fit"].items()
               for j, r in rows.items()) or \
                any(stale[1][key][n]["jobs_short"] != r["jobs_short"] for key, rows in pt["drain"].items()
                    for n, r in rows.items()):
            return True
    return False


PREDICATE_STAGES = range(ts.tr.POD_CAP, ts.tr.POD_AFFINITY + 1)


def claim_node_cause_moves(a, rnd):
    if not any(kind == "node_update" for kind, _ in rnd.changes):
        return False
    updated = {n["name"] for kind, n in rnd.changes if kind == "node_update"}
    for p0, p1 in zip(a.points, rnd.refs.points):
        for name in updated & set(p0["node"] or {}) & set(p1["node"] or {}):
            c0, c1 = p0["node"][name]["count"], p1["node"][name]["count"]
            if any(c1[x] < c0[x] and c1[y] > c0[y] for x in PREDICATE_STAGES for y in PREDICATE_STAGES if x != y):
                return True
    return False


def claim_drained_pod_stage_moves(a, rnd):
    """A pod Running at S0's open, walked off the same node at the same point
    of both cycles, lands elsewhere, and a node whose labels or taints the
    batch changed is one its selector or tolerations read differently."""
    changed = {n["name"]: n for kind, n in rnd.changes if kind == "node_update"}
    if not changed:
        return False
    old = {n.name: n.node for n in a.view.nodes}
    new = {n.name: n.node for n in rnd.refs.view.nodes}
    running = {e[1]: e[4] for tasks in a.dsnap.order for e in tasks if e[0] is not None and e[2] == ds.api.RUNNING}
    for p0, p1 in zip(a.points, rnd.refs.points):
        pl0, pl1 = places(p0), places(p1)
        for key in set(pl0) & set(pl1):
            if key[0] != "drain" or key[3] not in running or pl0[key] == pl1[key]:
                continue
            pod = running[key[3]]
            if any(old.get(n) is not None and new.get(n) is not None and
                   rr.first_failing_stage(pod, old[n], 1 << 30, {}) != rr.first_failing_stage(pod, new[n], 1 << 30, {})
                   for n in changed):
                return True
    return False


def claim_fit_queue_overused_flips(a, rnd):
    f0, f1 = a.points[-1]["fit"], rnd.refs.points[-1]["fit"]
    if f0 is None or f1 is None:
        return False
    return any(f0[lim][j]["queue_overused"] is not None and r["queue_overused"] is not None and
               bool(f0[lim][j]["queue_overused"]) != bool(r["queue_overused"])
               for lim, rows in f1.items() for j, r in rows.items() if j in f0[lim])


@pytest.mark.parametrize("family,claim", [(f, c) for f, cs in CLAIMS.items() for c in cs])
def test_family_carries_the_claim(refs, family, claim):
    fn = globals()["claim_" + claim]
    holds = [case for case, (fam, _) in CASES.items() if fam == family
             and any(fn(a, rnd) for a, rnd in steps(refs[case]))]
    print(f"{family}: {claim} holds on {holds}")
    assert holds, f"no {family} case carries {claim}"


# ------------------------------------------------------- the comparator sees
def stale_rows(kind, a, rnd, k):
    """What a stale session would hand in at point k of S1, or None where the stand-in does not apply."""
    r1 = rnd.refs
    pt = r1.points[k]
    got = copy.deepcopy(qr.point_as_rows(pt))
    if got["task"] is None:
        return None
    if kind == "rows0_unchanged":
        old = a.points[-1]
        return None if old["task"] is None else copy.deepcopy(qr.point_as_rows(old))
    if kind == "first_node_old_numbers":  # the index of S1 read in S0's list of names
        n0, n1 = a.view.flat.node_names, r1.view.flat.node_names
        back = lambda n: None if n is None else (n0[n1.index(n)] if n1.index(n) < len(n0) else None)  # noqa: E731
        for r in got["task"].values():
            r["first_node"] = [back(n) for n in r["first_node"]]
        for rows in got["room"].values():
            for r in rows.values():
                r["first_node"] = back(r["first_node"])
        return got
    if kind == "old_queue_overused":
        old = overused(a.points[-1])
        for u, r in got["task"].items():
            if old.get(("task", u)) is not None:
                r["queue_overused"] = old[("task", u)]
        for rows in got["room"].values():
            for u, r in rows.items():
                if old.get(("task", u)) is not None:
                    r["queue_overused"] = old[("task", u)]
        return got
    if kind == "old_min_available":
        got["victim"] = stale_min_victims(a, rnd, k)
        return None if got["victim"] is None else got
    if kind == "other_limit":  # the rows of the other limit under this one's name
        lo, hi = qr.LIMITS
        got["room"] = {lo: {u: dict(r, limit=lo) for u, r in got["room"][hi].items()},
                       hi: {u: dict(r, limit=hi) for u, r in got["room"][lo].items()}}
        return got
    if kind == "wrong_order":  # each task answered with its neighbour's row
        def rotate(rows):
            us = sorted(rows)
            return {u: dict(rows[v], task=u) for u, v in zip(us, us[1:] + us[:1])}
        got["task"] = rotate(got["task"])
        got["room"] = {lim: rotate(rows) for lim, rows in got["room"].items()}
        return got
    return stale_later_rows(kind, a, rnd, k, got)


def stale_later_rows(kind, a, rnd, k, got):
    """The stand-ins of LATER_STALE: `got` (S1's own references at point k)
    with the rows of kbg_job_fit, kbg_node_reasons and kbg_node_drain a stale
    session would give; the four older calls' rows stay S1's."""
    r1 = rnd.refs
    pt, old = r1.points[k], a.points[k]
    if got["fit"] is None or got["node"] is None:
        return None
    n0, n1 = a.view.flat.node_names, r1.view.flat.node_names
    t0 = [t.uid for t in a.view.flat.task_objs]
    t1 = {t.uid: i for i, t in enumerate(r1.view.flat.task_objs)}
    top = qr.FIT_LIMITS[-1]
    if kind == "later_rows0_unchanged":
        if old["fit"] is None or old["node"] is None:
            return None
        got["fit"], got["node"] = copy.deepcopy(old["fit"]), copy.deepcopy(old["node"])
        got["drain"] = {key: copy.deepcopy(old["drain"].get(key, old["drain"][(key[0], ())])) for key in got["drain"]}
        return got
    if kind == "places_old_numbers":  # S1's node and task indices read in S0's lists
        node = lambda n: None if n is None else (n0[n1.index(n)] if n1.index(n) < len(n0) else None)  # noqa: E731
        task = lambda u: None if u is None else (t0[t1[u]] if t1[u] < len(t0) else None)  # noqa: E731
        for rows in list(got["fit"].values()) + list(got["drain"].values()):
            for r in rows.values():
                r["places"] = [(task(t), node(n), kind_) for t, n, kind_ in r["places"]]
                r["first_unplaced"] = task(r["first_unplaced"])
        for r in got["node"].values():
            r["first_task"] = [task(u) for u in r["first_task"]]
        return got
    if kind == "later_old_min_available":
        if k == 0 or (stale := stale_min_walks(a, rnd, k)) is None:
            return None
        got["fit"], got["drain"] = stale
        return got
    if kind == "cordon_old_indices":  # asked to leave out S1's nodes i, the session leaves out those S0 had at i
        key = next((key for key in got["drain"] if key[1]), None)
        if key is None:
            return None
        stale = [n0[n1.index(c)] for c in key[1] if n1.index(c) < len(n0)]
        uid_of = lambda t: r1.view.flat.task_objs[t].uid if t >= 0 else None  # noqa: E731
        left_out = tuple(n1.index(c) for c in stale if c in n1)
        got["drain"][key] = qr.name_drain_rows(
            ds.expected_rows(r1.dsnap, r1.fx, pt["ref"], r1.rules, key[0], left_out), uid_of, n1)
        return got
    if kind == "later_other_limit":  # the rows of the other limit under this one's name
        lo, hi = qr.FIT_LIMITS
        got["fit"] = {lo: got["fit"][hi], hi: got["fit"][lo]}
        got["drain"][(lo, ())], got["drain"][(hi, ())] = got["drain"][(hi, ())], got["drain"][(lo, ())]
        return got
    if kind == "node_neighbour":  # each node answered with its neighbour's row
        def rotate(rows):
            ns_ = list(rows)
            return {n: dict(rows[v], node=n) for n, v in zip(ns_, ns_[1:] + ns_[:1])}
        got["node"] = rotate(got["node"])
        got["drain"] = {key: rotate(rows) for key, rows in got["drain"].items()}
        return got
    if kind == "deleted_pod_walked":  # a node's walk as S0 made it, with a pod that S1 no longer holds
        if old["drain"] is None:
            return None
        for name, r in old["drain"][(top, ())].items():
            if name in got["drain"][(top, ())] and any(t not in t1 for t, _, _ in r["places"]):
                mine = got["drain"][(top, ())][name]
                gone = [(i, p) for i, p in enumerate(r["places"]) if p[0] not in t1]
                for i, p in gone:
                    mine["places"].insert(min(i, len(mine["places"])), p)
                mine["tasks"] += len(gone)
                mine["walked"] += len(gone)
                return got
        return None
    raise ValueError(kind)


@pytest.mark.parametrize("kind", STALE + LATER_STALE)
def test_comparator_notices_a_stale_session(refs, kind):
    noticed, tried = [], 0
    for case, c in refs.items():
        for a, rnd in steps(c):
            aff = ts.has_pod_affinity(rnd.fx)
            for k in range(len(rnd.refs.points)):
                got = stale_rows(kind, a, rnd, k)
                if got is None:
                    continue
                tried += 1
                for rows in got["room"].values():  # (the references do not say the flag; the comparator asks for it)
                    for r in rows.values():
                        r.setdefault("affinity_now", aff)
                errs, said = qr.compare_point(rnd.refs.points[k], got, aff, case)
                assert said > 0
                if kind in LATER_STALE:  # (the older calls' rows are S1's own: nothing of them is reported)
                    assert all(any(call in e for call in LATER_CALLS) for e in errs), errs[:5]
                if errs:
                    noticed.append(case)
    print(f"{kind}: noticed on {len(set(noticed))} cases of {tried} points tried")
    assert noticed, f"the comparator notices {kind} on no case"


def test_comparator_passes_the_references_themselves(refs):
    said = 0
    for case, c in refs.items():
        for a, rnd in steps(c):
            aff = ts.has_pod_affinity(rnd.fx)
            for pt in rnd.refs.points:
                got = copy.deepcopy(qr.point_as_rows(pt))
                for rows in (got["room"] or {}).values():
                    for r in rows.values():
                        r.setdefault("affinity_now", aff)
                errs, n = qr.compare_point(pt, got, aff, case)
                assert not errs, errs[:5]
                said += n
    print(f"{said} reference rows compared with themselves")
    assert said > 0
