"""Session-level checks of kbg_task_headroom, shared by the hostsim tests
(tests/test_hostsim_headroom.py, through tests/headroom_worker.py) and the
device tests (tests/test_headroom_gpu.py).

`check_fixture` opens a session with reasons and, for each action prefix of
tests/task_why_session.py, runs the prefix and asks for the rows of every
Pending task. The expected rows are built as that module builds its own,
without the library and without what the actions' replay leaves in the
Python mirror: node Idle, Releasing and pod counts from the ORACLE's output of
the same prefix, the stages from reasons_ref.first_failing_stage, the loops
from tests/headroom_ref.py. A pod with a host port holds one copy a node.
reasons_ref has no inter-pod affinity stage, the predicates plugin's last:
on a session with pod affinity the nodes past the stages are a subset of the
reference's, so nodes_pass, both sums, both node counts and the max are
compared as upper bounds there and the rest exactly;
tests/golden/kat_headroom.json holds hand-derived pod-affinity rows instead.
Seeds whose cycle discards a statement after evicting get no expected rows
(tests/task_why_session.py: the same rule, the same quarter).

Against kbg_task_reasons on the same session and task the rows must satisfy,
whatever the session holds:
  nodes_idle == count[FITS_IDLE], nodes_releasing_only == count[FITS_RELEASING],
  nodes_pass == count[6] + count[7] + count[8], first_node the lower of the
  two causes' first nodes, panic_nodes == count[PANIC].

`check_resident` takes one session through helpers.churn_chain
(kbg_session_reset, kbg_session_update between the cycles) and holds its rows,
before and after each round's actions and at two limits, to a fresh session's
on the round's fixture and to `expected_rows` on that fixture.

`check_allocate` is independent of all that: on small hand-built clusters
whose only Pending pods are M identical copies, the ORACLE's allocate itself
places copies until none fits; its Allocate and Pipeline decisions, counted
per node, are what the row and the Python reference must give."""
import os

import headroom_ref as hr
import reasons_ref as rr
import task_why_ref as tr
import task_why_session as ts
import victim_why_session as ws
from helpers import run_oracle
from kbgpu import _abi
from kbgpu.fixture import headroom_message

PREFIXES, REST = ts.PREFIXES, ts.REST
SUMS = ("nodes_pass", "copies_idle", "copies_releasing", "nodes_idle", "nodes_releasing_only", "max_node_copies",
        "limit_hit")
EXACT = SUMS + ("first_node",)


def expected_rows(snap, fx, ref, rules, limit):
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
        row = dict(hr.empty_row(), best_effort=ts.empty(req), limit=limit, panic_nodes=0)
        for i, (name, node, max_task_num) in enumerate(snap.nodes):
            st = by_name[name]
            room = hr.INT32_MAX
            if rules["predicates"]:
                if node is None:
                    row["panic_nodes"] += 1
                    continue
                if max_task_num <= st["ntasks"] or rr.first_failing_stage(pod, node, 1 << 30, held[i]) >= 0:
                    continue
                room = max_task_num - st["ntasks"]
                if rr._ports(pod):  # the first copy's ports conflict with the second's (predicates.go:143-155)
                    room = 1
            ki, kr, cut = hr.copies(req, [float(v) for v in st["idle"]], [float(v) for v in st["releasing"]], room,
                                    limit, row["best_effort"])
            hr.add_node(row, i, ki, kr, cut)
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
        keys = ("best_effort", "limit", "panic_nodes") + (() if w["queue_overused"] is None else ("queue_overused",)) + \
            (() if aff else EXACT)
        errs += [f"{tag}: task {g['task']}: {k} is {g[k]}, reference {w[k]}" for k in keys if g[k] != w[k]]
        if aff:  # (module docstring) the reference's nodes past the stages hold the session's
            errs += [f"{tag}: task {g['task']}: {k} is {g[k]}, above the reference's {w[k]} before pod affinity"
                     for k in SUMS if g[k] > w[k]]
            if not g["affinity_now"]:
                errs.append(f"{tag}: task {g['task']}: affinity_now is not set on a session with pod affinity")
    return errs


def host_rows(ssn, tasks=None, limit=_abi.ROOM_MAX_LIMIT):
    os.environ["KBG_HOST_TASK_HEADROOM"] = "1"
    try:
        return ssn.task_headroom(tasks, limit)
    finally:
        del os.environ["KBG_HOST_TASK_HEADROOM"]


def invariants(ssn, rows, limit, tag):
    """The rows against kbg_task_reasons on the same session, the two paths, the message."""
    errs = []
    why = {r["task"]: r for r in ssn.task_reasons([r["task"] for r in rows])} if rows else {}
    for r in rows:
        t = r["task"]
        if not r["valid"]:
            errs.append(f"{tag}: task {t} of the mirror's Pending tasks has no row")
            continue
        c, f = why[t]["count"], why[t]["first_node"]
        firsts = [v for v in (f[tr.FITS_IDLE], f[tr.FITS_RELEASING]) if v >= 0]
        want = dict(nodes_idle=c[tr.FITS_IDLE], nodes_releasing_only=c[tr.FITS_RELEASING],
                    nodes_pass=c[tr.FITS_IDLE] + c[tr.FITS_RELEASING] + c[tr.SHORT],
                    first_node=min(firsts) if firsts else -1, panic_nodes=c[tr.PANIC],
                    best_effort=why[t]["best_effort"], queue_overused=why[t]["queue_overused"], limit=limit)
        errs += [f"{tag}: task {t}: {k} is {r[k]}, kbg_task_reasons gives {v}" for k, v in want.items() if r[k] != v]
        total = r["copies_idle"] + r["copies_releasing"]
        if not (r["nodes_idle"] <= r["copies_idle"] and r["nodes_releasing_only"] <= r["copies_releasing"] and
                r["max_node_copies"] <= limit and total <= r["max_node_copies"] * r["nodes_pass"] and
                (r["max_node_copies"] > 0) == (total > 0) and r["limit_hit"] <= r["nodes_pass"]):
            errs.append(f"{tag}: task {t}: the row contradicts itself: {r}")
        msg = headroom_message(r, 3)
        if not (msg.startswith(f"needs 3 more; room for {r['copies_idle']} now, {r['copies_releasing']} more") and
                ("lower bound" in msg) == bool(r["limit_hit"])):
            errs.append(f"{tag}: task {t}: message {msg!r}")
    host = host_rows(ssn, [r["task"] for r in rows], limit) if rows else []
    if host != rows:
        bad = [(a, b) for a, b in zip(rows, host) if a != b][:3]
        errs.append(f"{tag}: the device-shaped path differs from KBG_HOST_TASK_HEADROOM=1: {bad}")
    return errs


def check_fixture(fx, opts=None):
    """Every check of one fixture over the three prefixes: (errors, seen,
    skipped) as tests/task_why_session.py's check_fixture gives them; `seen`
    holds the largest expected value of each of hr.KEYS. The session is asked
    with limit 2 between the actions and with the largest limit after the
    prefix, then runs the actions of REST: its logs must equal those of a
    session that ran the same actions without a call."""
    errs, seen, skipped = [], [0] * len(hr.KEYS), False
    aff = ts.has_pod_affinity(fx)
    big = _abi.ROOM_MAX_LIMIT
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
            snap = ts.OpenSnap(ssn)
            rules = ws.plugin_rules(ssn.tiers)
            if prefix is PREFIXES[0]:  # before the first action: the snapshot
                errs += compare_rows(expected_rows(snap, fx, snap.state, rules, 7), ssn.task_headroom(limit=7), aff,
                                     "at open")
            for k, name in enumerate(prefix):
                if ts.run_actions(ssn, [name]) == "ref_panic":
                    errs.append(f"{tag}: {name} ends ref_panic where the oracle ends ok")
                if k + 1 < len(prefix):
                    errs += invariants(ssn, ssn.task_headroom(limit=2), 2, f"{tag}, after {name}")
            rows = ssn.task_headroom(limit=big)
            errs += invariants(ssn, rows, big, tag)
            if (aff or ts.has_host_ports(fx)) and not ws.discard_free(snap.mirror, ref):
                skipped = True
            else:
                want = expected_rows(snap, fx, ref, rules, big)
                errs += compare_rows(want, rows, aff, tag)
                for w in want.values():
                    seen = [max(a, w[k]) for a, k in zip(seen, hr.KEYS)]
            if rows:  # a subset asked by index, in the order asked
                pick = [rows[-1]["task"], rows[0]["task"]]
                if ssn.task_headroom(pick, big) != [rows[-1], rows[0]]:
                    errs.append(f"{tag}: tasks {pick} asked by index differ from their rows of the whole call")
            with_calls = (ts.run_actions(ssn, rest), ts.log_of(ssn))
        finally:
            ssn.close()
        plain, _ = ws.open_with_reasons(fxp, opts)
        try:
            if (ts.run_actions(plain, list(prefix) + rest), ts.log_of(plain)) != with_calls:
                errs.append(f"{tag}: the logs of {list(prefix) + rest} differ with the calls in between")
        finally:
            plain.close()
    return errs, seen, skipped


def check_refusals(fx):
    """No reasons: KBG_E_INVALID. A limit outside [1, 1024]: KBG_E_INVALID. A task that is not Pending: valid == 0.
    An index out of range, tasks == NULL: KBG_E_INVALID."""
    from kbgpu.fixture import run_fixture
    errs = []

    def refused(ssn, what, *args):
        try:
            ssn.task_headroom(*args)
            errs.append(f"{what}: the call did not fail")
        except _abi.KbgError as e:
            if e.status != "invalid":
                errs.append(f"{what}: {e}")

    _, ssn = run_fixture(dict(fx, actions=["allocate"]), {})
    try:
        refused(ssn, "reasons = 0", [0], 4)
    finally:
        ssn.close()
    ssn, _ = ws.open_with_reasons(fx)
    try:
        for limit in (0, -1, 1025, 1 << 30):
            refused(ssn, f"limit {limit}", None, limit)
        if not ssn.task_headroom(limit=1) or not ssn.task_headroom(limit=1024):
            errs.append("limits 1 and 1024 give no rows")
        ts.run_actions(ssn, ["allocate"])
        placed = [d[0] for d in ssn.decisions]
        assert placed, "the fixture's allocate places nothing"
        row = ssn.task_headroom([placed[0]], 4)[0]
        if row["valid"] or any(v for k, v in row.items() if k != "task"):
            errs.append(f"a placed task has the row {row}")
        for bad in (-1, len(ssn.flat.task_objs)):
            refused(ssn, f"task index {bad}", [bad], 4)
        if _abi.lib().kbg_task_headroom(ssn.handle, None, 1, 4, (_abi.kbg_task_room * 1)()) != _abi.KBG_E_INVALID:
            errs.append("tasks == NULL: the call did not return KBG_E_INVALID")
    finally:
        ssn.close()
    return errs


def check_resident(fx0, seed, rounds, opts=None, limits=(2, _abi.ROOM_MAX_LIMIT)):
    """A resident session (kbg_session_reset, kbg_session_update) over
    helpers.churn_chain: before the round's first action and after its
    actions, at both limits, its rows against a fresh session's on the round's
    fixture (task by uid, node by name) and against `expected_rows` on that
    fixture, the fresh mirror at open and the oracle's output of the round.
    Returns (errors, rows compared)."""
    import ctypes
    errs, said = [], 0
    ssn = None
    L = _abi.lib()
    aff = ts.has_pod_affinity(fx0)

    def named(s, rows):
        names = s.flat.node_names
        return sorted([s.flat.task_objs[r["task"]].uid] +
                      [names[v] if k == "first_node" and v >= 0 else v for k, v in sorted(r.items()) if k != "task"]
                      for r in rows)

    try:
        for r, (fx, changes, ref_full) in enumerate(ws.resident_rounds(fx0, seed, rounds)):
            assert ref_full["status"] == "ok", ref_full.get("error")
            actions = fx.get("actions") or ["allocate"]
            if ssn is None:
                ssn, _ = ws.open_with_reasons(fx, opts)
            else:
                _abi.check(L.kbg_session_reset(ssn.handle))
                ssn.update(changes)
            fresh, _ = ws.open_with_reasons(fx, opts)
            try:
                snap = ts.OpenSnap(fresh)
                rules = ws.plugin_rules(fresh.tiers)
                if list(ssn.flat.node_names) != list(fresh.flat.node_names):
                    errs.append(f"round {r}: the resident session's nodes are not in the fresh session's order")
                    break
                uid_task = {t.uid: i for i, t in enumerate(ssn.flat.task_objs) if t is not None}
                refs_ok = not ((aff or ts.has_host_ports(fx)) and not ws.discard_free(snap.mirror, ref_full))
                for when in ("before", "after"):
                    if when == "after":
                        cap = max(1, len(ssn.flat.task_objs))
                        buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
                        for name in actions:
                            _abi.check(getattr(L, ws.ENTRY[name])(ssn.handle, buf, cap, ctypes.byref(n)))
                        ts.run_actions(fresh, actions)
                    for limit in limits:
                        tag = f"round {r}, {when} the actions, limit {limit}"
                        want = fresh.task_headroom(limit=limit)
                        mine = [uid_task[fresh.flat.task_objs[w["task"]].uid] for w in want]
                        got = ssn.task_headroom(mine, limit)
                        if named(fresh, want) != named(ssn, got):
                            errs.append(f"{tag}: the resident session's rows differ from a fresh session's")
                        said += len(want)
                        if refs_ok:  # in the fresh session's task numbering, which expected_rows speaks
                            exp = expected_rows(snap, fx, snap.state if when == "before" else ref_full, rules, limit)
                            errs += compare_rows(exp, [dict(g, task=w["task"]) for g, w in zip(got, want)], aff, tag)
            finally:
                fresh.close()
    finally:
        if ssn is not None:
            ssn.close()
    if not said:
        errs.append("no round held a Pending task: the case says nothing")
    return errs, said


def check_kat(fx):
    """The hand-derived rows of a KAT of tests/golden/make_kat_headroom.py, at open, on both paths."""
    ssn, _ = ws.open_with_reasons(fx)
    errs = []
    try:
        names = ssn.flat.node_names
        uid_task = {t.uid: i for i, t in enumerate(ssn.flat.task_objs)}
        limit = fx["expected"]["limit"]
        for exp in fx["expected"]["task_room"]:
            for rows_of in (lambda ts_: ssn.task_headroom(ts_, limit), lambda ts_: host_rows(ssn, ts_, limit)):
                (g,) = rows_of([uid_task[exp["task"]]])
                got = dict(g, task=exp["task"], needed=exp["needed"],
                           first_node=names[g["first_node"]] if g["first_node"] >= 0 else None,
                           message=headroom_message(g, exp["needed"]))
                want = dict(exp, valid=True)
                errs += [f"{exp['task']}: {k} is {got[k]}, hand-derived {want[k]}" for k in want if got[k] != want[k]]
    finally:
        ssn.close()
    return errs


# ------------------------------------------------- against the oracle's allocate
TIERS = [[{"name": "priority"}, {"name": "gang"}], [{"name": "drf"}, {"name": "predicates"}]]


def copies_fixture(name, nodes, held, req, copies):
    """`nodes`: (cpu, memory Mi, pods); `held`: (node index, cpu m, memory Mi,
    being deleted) of the pods of job X; `copies` identical Pending pods
    asking `req` in job P, MinMember 1, everything in one queue."""
    def pod(uid, group, r, node_name="", **kw):
        return dict({"uid": uid, "namespace": "ns", "name": uid, "phase": "Running" if node_name else "Pending",
                     "nodeName": node_name, "annotations": {"scheduling.k8s.io/group-name": group},
                     "containers": [{"requests": r}]}, **kw)
    ns = [{"name": f"c{i:02d}", "allocatable": {"cpu": f"{c}m", "memory": f"{m}Mi", "pods": str(p)}, "labels": {}}
          for i, (c, m, p) in enumerate(nodes)]
    pods = [pod(f"p{i:04d}", "P", req) for i in range(copies)]
    for k, (n, c, m, deleted) in enumerate(held):
        kw = {"deletionTimestamp": "2026-01-01T00:00:00Z"} if deleted else {}
        pods.append(pod(f"x{k:03d}", "X", {"cpu": f"{c}m", "memory": f"{m}Mi"}, ns[n]["name"], **kw))
    groups = [{"namespace": "ns", "name": g, "minMember": 1, "queue": "q", "creationTimestamp": ts_ * 10 ** 9}
              for g, ts_ in (("P", 100), ("X", 1))]
    return {"name": name, "actions": ["allocate"], "tiers": TIERS, "nodes": ns, "queues": [{"name": "q", "weight": 1}],
            "podGroups": groups, "pods": pods}


def seeded_copies_fixture(seed, n_nodes, copies):
    import numpy as np
    rng = np.random.default_rng(seed)
    nodes = [(int(rng.choice((1000, 2000, 4000))), int(rng.choice((1024, 2048, 4096))), int(rng.choice((3, 6, 110))))
             for _ in range(n_nodes)]
    held = []
    for n, (c, m, p) in enumerate(nodes):
        for _ in range(int(rng.integers(0, min(p, 3) + 1))):
            pc, pm = int(rng.choice((250, 500, 1000))), int(rng.choice((128, 512)))
            if pc <= c and pm <= m:  # (a node never holds more than it has)
                held.append((n, pc, pm, bool(rng.random() < 0.5)))
                c, m = c - pc, m - pm
    return copies_fixture(f"copies-{seed}", nodes, held, {"cpu": "500m", "memory": "256Mi"}, copies)


def allocate_fixtures():
    hand = copies_fixture(
        "copies-hand",
        # c00: Idle 2500m: 2 of 1000m, then Releasing 1500m: 1. c01: pod cap 3 with one pod: 2 of its 4. c02: none fits
        [(4000, 8192, 110), (4000, 8192, 3), (1500, 8192, 110)],
        [(0, 1500, 1024, True), (1, 0, 0, False), (2, 1000, 128, False)], {"cpu": "1", "memory": "512Mi"}, 8)
    return {"hand": hand, "seed17": seeded_copies_fixture(41, 17, 120), "seed70": seeded_copies_fixture(42, 70, 500)}


def check_allocate(fx):
    errs = []
    ref = run_oracle(fx)
    copies = {p["uid"] for p in fx["pods"] if p["phase"] == "Pending"}
    per = {}
    for d in ref["decisions"]:
        assert d["task"] in copies and d["kind"] in ("allocate", "pipeline"), d
        k = per.setdefault(d["node"], [0, 0])
        k[d["kind"] == "pipeline"] += 1
    assert ref["status"] == "ok" and 0 < len(ref["decisions"]) < len(copies), \
        f"{fx['name']}: the oracle places {len(ref['decisions'])} of {len(copies)}: no copy is left unplaced"
    ssn, _ = ws.open_with_reasons(fx)
    try:
        names = ssn.flat.node_names
        snap = ts.OpenSnap(ssn)
        task = snap.pending[0][0]
        req = snap.pending[0][2]
        # the Python reference, node by node, on the mirror at open
        for st, (name, node, max_task_num) in zip(snap.state["nodes"], snap.nodes):
            ki, kr, _ = hr.copies(req, [float(v) for v in st["idle"]], [float(v) for v in st["releasing"]],
                                  max_task_num - st["ntasks"] if max_task_num > st["ntasks"] else 0, 1024, False)
            if [ki, kr] != per.get(name, [0, 0]):
                errs.append(f"{fx['name']}: node {name}: the reference gives {[ki, kr]}, the oracle's allocate "
                            f"{per.get(name, [0, 0])}")
        for rows_of in (ssn.task_headroom, lambda tasks, limit: host_rows(ssn, tasks, limit)):
            (g,) = rows_of([task], 1024)
            placed = [n for n in names if n in per]
            want = dict(copies_idle=sum(k[0] for k in per.values()), copies_releasing=sum(k[1] for k in per.values()),
                        first_node=names.index(placed[0]), max_node_copies=max(sum(k) for k in per.values()),
                        nodes_idle=sum(k[0] > 0 for k in per.values()),
                        nodes_releasing_only=sum(k[0] == 0 for k in per.values()), limit_hit=0, valid=True)
            errs += [f"{fx['name']}: {k} is {g[k]}, the oracle's allocate gives {v}" for k, v in want.items() if g[k] != v]
    finally:
        ssn.close()
    return errs
