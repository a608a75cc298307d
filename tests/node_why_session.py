"""Session-level checks of kbg_node_reasons, shared by the hostsim tests
(tests/test_hostsim_node_why.py, through tests/node_why_worker.py) and the
device tests (tests/test_node_why_gpu.py).

`check_fixture` opens a session with reasons and, for each action prefix of
tests/task_why_session.py, runs the prefix and asks for the row of every node.
The expected rows are built here, node by node and task by task, from what
task_why_session.OpenSnap copied at open and the ORACLE's output of the same
prefix (node Idle, Releasing, pod counts, decisions, queues), with the stage
from reasons_ref.first_failing_stage and the resource test of
tests/task_why_ref.py: nothing of them comes from the library. What that
module says about pod affinity (no such stage in the reference: causes 0..4
exactly, 5..8 by their sum) and about discarded statements (no expected rows
on such seeds with host ports or pod affinity) holds here in the same way.

Beside the expected rows, every asked point is held to the transpose of
kbg_task_reasons on the same session (`transpose`): the two calls reduce one
table along its two axes."""
import ctypes
import os

import reasons_ref as rr
import task_why_ref as tr
import task_why_session as ts
import victim_why_session as ws
from helpers import run_oracle
from kbgpu import _abi
from kbgpu.fixture import _OrderedCache, fixture_tiers, node_message
from kbgpu.framework import open_session

N = tr.N_CAUSES


def empty_row(node, pending):
    return dict(valid=True, node=node, pending=pending, count=[0] * N, first_task=[-1] * N, idle_short=[0, 0, 0],
                open_idle=0, open_releasing=0, idle_best_effort=0)


def expected_rows(snap, fx, ref, rules):
    """One row per node of the session (all of them live) after the oracle's
    prefix (ref: its output; snap.state: no action yet, open_* then None)."""
    pods = {p["uid"]: p for p in fx["pods"]}
    decided = {d["task"] for d in ref["decisions"]}
    by_name = {n["name"]: n for n in ref["nodes"]}
    held = [dict(h) for h in snap.held]  # a decision whose key the node holds leaves it as it is (node_info.go:101-106)
    index = {name: i for i, (name, _, _) in enumerate(snap.nodes)}
    for d in ref["decisions"]:
        held[index[d["node"]]].setdefault(rr.pod_key(pods[d["task"]]), pods[d["task"]])
    queues = {q["uid"]: q for q in ref["queues"] or []}

    def overused(queue):  # Overused (proportion.go:188-194): only queues with an attr
        q = queues.get(queue)
        return bool(rules["proportion"] and q is not None and
                    tr.less_equal([float(v) for v in q["deserved"]], [float(v) for v in q["allocated"]]))

    pending = [p for p in snap.pending if p[1] not in decided]
    out = []
    for i, (name, node, max_task_num) in enumerate(snap.nodes):
        st = by_name[name]
        idle, rel = [float(v) for v in st["idle"]], [float(v) for v in st["releasing"]]
        row = empty_row(i, len(pending))
        for t, uid, req, pod, queue in pending:
            k, short, be = None, [False] * 3, ts.empty(req)
            if rules["predicates"]:
                if node is None:
                    k = tr.PANIC
                elif max_task_num <= st["ntasks"]:
                    k = tr.POD_CAP
                else:
                    s = rr.first_failing_stage(pod, node, 1 << 30, held[i])
                    k = s if s >= 0 else None
            if k is None:
                if be or tr.less_equal(req, idle):
                    k = tr.FITS_IDLE
                else:
                    k = tr.FITS_RELEASING if tr.less_equal(req, rel) else tr.SHORT
                    short = tr.fit_delta_negative(idle, req)
            row["count"][k] += 1
            if row["first_task"][k] < 0 or t < row["first_task"][k]:
                row["first_task"][k] = t
            for d in range(3):
                row["idle_short"][d] += bool(short[d])
            if k == tr.FITS_IDLE:
                row["open_idle"] += not overused(queue)
                row["idle_best_effort"] += be
            elif k == tr.FITS_RELEASING:
                row["open_releasing"] += not overused(queue)
        if ref["queues"] is None:
            row["open_idle"] = row["open_releasing"] = None
        out.append(row)
    return out


def compare_rows(want, got, aff, tag):
    errs = []
    if len(want) != len(got):
        return [f"{tag}: {len(got)} rows, reference {len(want)}"]
    for w, g in zip(want, got):
        keys = ("valid", "node", "pending") + (() if w["open_idle"] is None or aff else ("open_idle", "open_releasing")) + \
            (() if aff else ("count", "first_task", "idle_short", "idle_best_effort"))
        errs += [f"{tag}: node {w['node']}: {k} is {g[k]}, reference {w[k]}" for k in keys if g[k] != w[k]]
        if aff:  # the stages before pod affinity exactly, the rest by its sum
            if g["count"][:5] != w["count"][:5] or g["first_task"][:5] != w["first_task"][:5]:
                errs.append(f"{tag}: node {w['node']}: stages 0..4 are {g['count'][:5]} at {g['first_task'][:5]}, "
                            f"reference {w['count'][:5]} at {w['first_task'][:5]}")
            if sum(g["count"][5:9]) != sum(w["count"][5:9]) or g["count"][9] != w["count"][9]:
                errs.append(f"{tag}: node {w['node']}: count {g['count']}, reference {w['count']} before pod affinity")
    return errs


def host_rows(ssn, nodes=None):
    os.environ["KBG_HOST_NODE_WHY"] = "1"
    try:
        return ssn.node_reasons(nodes)
    finally:
        del os.environ["KBG_HOST_NODE_WHY"]


def transpose(ssn, rows, tag):
    """(errors, some node's open_idle or open_releasing is below its count):
    the rows against kbg_task_reasons for every Pending task of the same
    session, the named-node call and the host path."""
    errs = []
    # (every task is asked: a row is valid where the session, not the Python mirror, holds the task Pending)
    tasks = [r for r in ssn.task_reasons([t for t, obj in enumerate(ssn.flat.task_objs) if obj is not None]) if r["valid"]]
    live = [r for r in rows if r["valid"]]
    if len(live) != len(ssn.flat.node_names):
        errs.append(f"{tag}: {len(live)} valid rows, {len(ssn.flat.node_names)} live nodes")
    for c in range(N):
        a, b = sum(r["count"][c] for r in live), sum(t["count"][c] for t in tasks)
        if a != b:
            errs.append(f"{tag}: cause {c}: {a} (node, task) pairs by node, {b} by task")
    for d in range(3):
        a, b = sum(r["idle_short"][d] for r in live), sum(t["idle_short"][d] for t in tasks)
        if a != b:
            errs.append(f"{tag}: idle_short[{d}]: {a} by node, {b} by task")
    for r in live:
        if r["pending"] != len(tasks) or sum(r["count"]) != r["pending"]:
            errs.append(f"{tag}: node {r['node']}: pending {r['pending']}, sum {sum(r['count'])}, {len(tasks)} Pending tasks")
        if not isinstance(node_message(r), str) or (tasks and str(len(tasks)) not in node_message(r)):
            errs.append(f"{tag}: node {r['node']}: message {node_message(r)!r}")
    by_node = {r["node"]: r for r in live}
    for t in tasks:
        for c in range(N):
            f = t["first_node"][c]
            if f >= 0 and (f not in by_node or by_node[f]["count"][c] < 1 or not 0 <= by_node[f]["first_task"][c] <= t["task"]):
                errs.append(f"{tag}: task {t['task']} has node {f} first under cause {c}; its row: {by_node.get(f)}")
    # each node's lowest task of a cause names that node under the cause, at or after its own first node
    by_task = {t["task"]: t for t in tasks}
    for r in live:
        for c in range(N):
            f = r["first_task"][c]
            if (f >= 0) != (r["count"][c] > 0):
                errs.append(f"{tag}: node {r['node']}: cause {c}: count {r['count'][c]}, first task {f}")
            elif f >= 0 and (f not in by_task or not 0 <= by_task[f]["first_node"][c] <= r["node"]):
                errs.append(f"{tag}: node {r['node']} has task {f} first under cause {c}; its row: {by_task.get(f)}")
    any_over, all_over = any(t["queue_overused"] for t in tasks), all(t["queue_overused"] for t in tasks)
    differs = False
    for r in live:
        oi, orl, ci, cr = r["open_idle"], r["open_releasing"], r["count"][tr.FITS_IDLE], r["count"][tr.FITS_RELEASING]
        if not (0 <= oi <= ci and 0 <= orl <= cr) or not 0 <= r["idle_best_effort"] <= ci:
            errs.append(f"{tag}: node {r['node']}: open {oi}, {orl} and best-effort {r['idle_best_effort']} of {ci}, {cr}")
        if not any_over and (oi, orl) != (ci, cr):
            errs.append(f"{tag}: node {r['node']}: no queue is overused, yet open {oi}, {orl} of {ci}, {cr}")
        if all_over and tasks and (oi or orl):
            errs.append(f"{tag}: node {r['node']}: every queue is overused, yet open {oi}, {orl}")
        differs |= (oi, orl) != (ci, cr)
    host = host_rows(ssn)
    if host != rows:
        bad = [(a, b) for a, b in zip(rows, host) if a != b][:3]
        errs.append(f"{tag}: the device-shaped path differs from KBG_HOST_NODE_WHY=1: {bad}")
    if rows:  # named nodes, one of them twice, in the order asked
        n = len(rows)
        pick = [n - 1, 0, n - 1, n // 2] + ([65] if n > 65 else [])
        if ssn.node_reasons(pick) != [rows[i] for i in pick]:
            errs.append(f"{tag}: nodes {pick} asked by index differ from their rows of the whole call")
        if host_rows(ssn, pick) != [rows[i] for i in pick]:
            errs.append(f"{tag}: nodes {pick} asked by index on the host path differ from their rows of the whole call")
    return errs, differs


def check_fixture(fx, opts=None):
    """Every check of one fixture over the three prefixes (the order of
    task_why_session.check_fixture: asked before the first action, between the
    actions and after the prefix; then the actions of REST, whose logs must
    equal those of a session without a call). Returns (errors, seen, skipped,
    differs): `seen` sums the expected counts per cause, `differs` says that
    some asked row had tasks of an overused queue under cause 6 or 7."""
    errs, seen, skipped, differs = [], [0] * N, False, False
    aff = ts.has_pod_affinity(fx)
    for prefix in ts.PREFIXES:
        tag = "+".join(prefix)
        fxp = dict(fx, actions=list(prefix))
        ref = run_oracle(fxp)
        if ref["status"] != "ok":
            errs.append(f"{tag}: the oracle ends {ref['status']}: pick another fixture")
            continue
        rest = ts.REST[tuple(prefix)]
        ssn, _ = ws.open_with_reasons(fxp, opts)
        try:
            snap = ts.OpenSnap(ssn)
            rules = ws.plugin_rules(ssn.tiers)
            if prefix is ts.PREFIXES[0]:  # before the first action: the snapshot
                rows = ssn.node_reasons()
                errs += compare_rows(expected_rows(snap, fx, snap.state, rules), rows, aff, "at open")
                errs += transpose(ssn, rows, "at open")[0]
            for k, name in enumerate(prefix):
                if ts.run_actions(ssn, [name]) == "ref_panic":
                    errs.append(f"{tag}: {name} ends ref_panic where the oracle ends ok")
                if k + 1 < len(prefix):
                    e, d = transpose(ssn, ssn.node_reasons(), f"{tag}, after {name}")
                    errs += e
                    differs |= d
            rows = ssn.node_reasons()
            e, d = transpose(ssn, rows, tag)
            errs += e
            differs |= d
            if (aff or ts.has_host_ports(fx)) and not ws.discard_free(snap.mirror, ref):
                skipped = True
            else:
                want = expected_rows(snap, fx, ref, rules)
                errs += compare_rows(want, rows, aff, tag)
                for w in want:
                    seen = [a + b for a, b in zip(seen, w["count"])]
            with_calls = (ts.run_actions(ssn, rest), ts.log_of(ssn))
        finally:
            ssn.close()
        plain, _ = ws.open_with_reasons(fxp, opts)
        try:
            if (ts.run_actions(plain, list(prefix) + rest), ts.log_of(plain)) != with_calls:
                errs.append(f"{tag}: the logs of {list(prefix) + rest} differ with the calls in between")
        finally:
            plain.close()
    return errs, seen, skipped, differs


def check_refusals(fx):
    """No reasons: KBG_E_INVALID. An index out of range: KBG_E_INVALID.
    nodes == NULL with another count than the session's: KBG_E_INVALID."""
    from kbgpu.fixture import run_fixture
    errs = []
    _, ssn = run_fixture(dict(fx, actions=["allocate"]), {})
    try:
        try:
            ssn.node_reasons([0])
            errs.append("reasons = 0: the call did not fail")
        except _abi.KbgError as e:
            if e.status != "invalid":
                errs.append(f"reasons = 0: {e}")
    finally:
        ssn.close()
    ssn, _ = ws.open_with_reasons(fx)
    try:
        n = len(ssn.flat.node_names)
        for bad in (-1, n):
            try:
                ssn.node_reasons([0, bad])
                errs.append(f"node index {bad}: the call did not fail")
            except _abi.KbgError as e:
                if e.status != "invalid":
                    errs.append(f"node index {bad}: {e}")
        out = (_abi.kbg_node_why * (n + 1))()
        for count in (n - 1, n + 1):
            if _abi.lib().kbg_node_reasons(ssn.handle, None, count, out) != _abi.KBG_E_INVALID:
                errs.append(f"nodes == NULL with n_nodes {count} of {n}: the call did not return KBG_E_INVALID")
        if _abi.lib().kbg_node_reasons(ssn.handle, None, n, None) != _abi.KBG_E_INVALID:
            errs.append("out == NULL: the call did not return KBG_E_INVALID")
        if ssn.node_reasons([]) != []:
            errs.append("no node asked: rows")
    finally:
        ssn.close()
    return errs


def named(s, rows):
    """Rows by node name with their tasks by uid: what two sessions that number differently share."""
    uid = lambda t: s.flat.task_objs[t].uid if t >= 0 else None  # noqa: E731
    return {s.flat.node_names[r["node"]]: dict(r, node=None, first_task=[uid(t) for t in r["first_task"]])
            for r in rows if r["valid"]}


def check_resident(case, opts=None):
    """A case of tests/query_update_cases.py: the session is asked after its
    first cycle (every buffer sized for it), then reset and updated; before
    the next cycle's first action and after each of its actions its rows must
    be those of a fresh session opened on the cache replayed through the same
    events, node by name and task by uid. The lowest task index of a cause is
    compared by uid only where both sessions number their tasks alike."""
    import query_update_cases as qc
    import query_update_ref as qr
    import query_update_session as qs
    from update_events import fixture_after, replay
    L = _abi.lib()
    fam, build = qc.all_cases()[case]
    fx0, rounds_of, flags = build()
    errs, said = [], 0
    actions = qr.actions_of(fx0)
    ssn, _ = ws.open_with_reasons(fx0, opts)
    try:
        cap = 4 * len(ssn.flat.task_objs) + 64
        buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
        for name in actions:
            if (status := qs.call_action(ssn, name, buf, cap, n)) != "ok":
                return [f"S0: {name} ends {status}"]
        warm = named(ssn, ssn.node_reasons())
        done = []
        for r, changes_of in enumerate(rounds_of):
            fx_now = fixture_after(fx0, done) if done else fx0
            _abi.check(L.kbg_session_reset(ssn.handle))
            changes = changes_of(ssn, fx_now)
            ssn.update(changes)
            done.append(changes)
            order = {"jobs": [j.uid for j in ssn.jobs], "nodes": list(ssn.flat.node_names),
                     "queues": [q.uid for q in ssn.queues]}
            fssn = open_session(_OrderedCache(replay(fx0, done), {"sessionOrder": order}), fixture_tiers(fx0),
                                dict(opts or {}), reasons=True)
            try:
                if list(fssn.flat.node_names) != order["nodes"]:
                    return errs + [f"round {r}: the fresh session is not in the updated session's node order"]
                same_numbers = [t.uid if t is not None else None for t in ssn.flat.task_objs] == \
                    [t.uid if t is not None else None for t in fssn.flat.task_objs]
                fbuf, fn = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
                for k in range(len(actions) + 1):
                    tag = f"round {r}, " + ("before the first action" if k == 0 else f"after {actions[k - 1]}")
                    if k:
                        a = qs.call_action(ssn, actions[k - 1], buf, cap, n)
                        b = qs.call_action(fssn, actions[k - 1], fbuf, cap, fn)
                        if a != "ok" or b != "ok":
                            return errs + [f"{tag}: the action ends {a}, the fresh session's {b}"]
                    raw, fraw = ssn.node_reasons(), fssn.node_reasons()
                    got, want = named(ssn, raw), named(fssn, fraw)
                    if not same_numbers:  # the lowest index of a cause is another task in another numbering
                        for rows in (got, want):
                            for row in rows.values():
                                row["first_task"] = [u is not None for u in row["first_task"]]
                    elif raw != fraw:
                        errs.append(f"{tag}: the rows differ index by index from the fresh session's")
                    if sorted(got) != sorted(want):
                        errs.append(f"{tag}: rows of {sorted(got)}, the fresh session's {sorted(want)}")
                    else:
                        errs += [f"{tag}: node {name}: {got[name]}, the fresh session's {want[name]}"
                                 for name in got if got[name] != want[name]]
                    errs += transpose(ssn, raw, tag)[0]
                    said += sum(row["pending"] for row in got.values())
                    last = got
            finally:
                fssn.close()
        if last == warm:
            errs.append("the rows after the updates equal the warm-up's: the case says nothing")
    finally:
        ssn.close()
    if not said:
        errs.append("no asked point held a Pending task: the case says nothing")
    return errs


def check_kat(fx):
    """The hand-derived rows of tests/golden/kat_node_why.json (tests/golden/
    make_kat_node_why.py), at open: per node the Pending pods under each cause
    by uid, from which count, first_task (the lowest session index of those
    pods) and the open and best-effort parts follow. Asked for all nodes and
    for each node alone."""
    ssn, _ = ws.open_with_reasons(fx)
    errs = []
    try:
        names = ssn.flat.node_names
        uid_task = {t.uid: i for i, t in enumerate(ssn.flat.task_objs) if t is not None}
        exp = fx["expected"]["node_why"]
        if sorted(e["node"] for e in exp) != sorted(names):
            return [f"the session's nodes {names}, hand-derived {[e['node'] for e in exp]}"]
        whole = ssn.node_reasons()
        for e in exp:
            i = names.index(e["node"])
            want = dict(empty_row(i, e["pending"]), idle_short=e["idle_short"], open_idle=e["open_idle"],
                        open_releasing=e["open_releasing"], idle_best_effort=e["idle_best_effort"])
            for cause, uids in e["tasks"].items():
                want["count"][int(cause)] = len(uids)
                want["first_task"][int(cause)] = min(uid_task[u] for u in uids)
            for what, g in (("all nodes", whole[i]), ("alone", ssn.node_reasons([i])[0])):
                errs += [f"{e['node']} ({what}): {k} is {g[k]}, hand-derived {want[k]}" for k in want if g[k] != want[k]]
                if node_message(g) != e["message"]:
                    errs.append(f"{e['node']} ({what}): message {node_message(g)!r}, hand-derived {e['message']!r}")
    finally:
        ssn.close()
    return errs
