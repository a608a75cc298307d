"""The seven query calls (kbg_job_reasons, kbg_victim_reasons,
kbg_task_reasons, kbg_task_headroom, kbg_job_fit, kbg_node_reasons,
kbg_node_drain) on a session that was asked, then updated, then asked again:
the only order in which a stale stage plane, a query buffer sized for the old
session, an index in the old numbering or a MinAvailable from before the
update can show. Shared by tests/test_hostsim_query_update.py (through
tests/query_update_worker.py) and tests/test_query_update_gpu.py; it works
with whichever library KBG_LIB_PATH names.

`check_rounds` opens S0 with reasons, runs the actions and asks all seven
calls for every job, every task and every node (kbg_task_headroom at limits 1
and 64, kbg_job_fit at 2 and 512, kbg_node_drain at both without a cordon and
at 512 with one): the planes are valid, the victim tables ready, every query
buffer sized for S0. Then, per round: kbg_session_reset, kbg_session_update,
the seven calls with no action since the update (the two task calls answer
for every Pending task, kbg_victim_reasons is refused, kbg_job_reasons is not
valid, the three later calls answer for the jobs with a Pending task with a
request and for every live node), and the seven calls after each action. At a
point all seven are asked of the one session: they share the stage planes,
the pinned staging and the device pool. Their order at the session's k-th
asked point is ORDER rotated by k (`call_order`; k starts at `first_point`,
which the worker sets per case), so that over the points of a case a call
runs before and after others and is, on some case, the first after an update;
the order is said with every difference. Every point is compared with
  A. a fresh session opened on the Python cache replayed through the same
     events, in the updated session's order, driven through the same actions
     and asked the same questions (the cordon by node name): field by field
     by uid and name, and index by index where the two number their tasks
     alike (an in-place batch keeps the old task indices);
  B. the references of tests/query_update_ref.py on the fixture after the
     events and the oracle's output of the same prefix, where a fixture can
     say the cache after the events: nothing of B comes from the library.
     Where the drain reference is silent the cordon is
     drain_session.pick_cordon of the session's own rows.
and held to the self-checks of the three later calls that need only the
session and its rows: node_why_session.transpose, job_fit_session.invariants
and drain_session.invariants (each also asks the call's host path).
The updated session's decision log and final node states must be the
oracle's (the fresh session's where no fixture says S1), so that a wrong cycle
is not reported as a wrong query: with seven calls between the actions this
is also the check that none of them changes anything."""
import ctypes
import os

import drain_session as ds
import job_fit_session as js
import node_why_session as ns
import query_update_ref as qr
import reasons_ref as rr
import task_why_session as ts
import victim_why_session as ws
from kbgpu import _abi
from kbgpu.api import PENDING
from kbgpu.fixture import _OrderedCache, fixture_tiers
from kbgpu.framework import open_session
from update_events import fixture_after, replay

LIMITS, FIT_LIMITS = qr.LIMITS, qr.FIT_LIMITS
ORDER = ("job", "victim", "task", "room", "fit", "node", "drain")
HOST_SWITCHES = ("KBG_HOST_TASK_WHY", "KBG_HOST_TASK_HEADROOM", "KBG_HOST_JOB_FIT", "KBG_HOST_NODE_WHY",
                 "KBG_HOST_NODE_DRAIN")


def _name(names, n):
    return names[n] if n >= 0 else None


def call_order(k):
    """The order of the seven calls at the session's k-th asked point: ORDER rotated by k."""
    return [ORDER[(i + k) % len(ORDER)] for i in range(len(ORDER))]


def drain_questions(s, cordons):
    """kbg_node_drain's questions as {(limit, cordon by name): rows}: `cordons`
    as given, or both limits uncordoned and the higher with
    drain_session.pick_cordon of the session's own uncordoned rows."""
    names = s.flat.node_names
    out = {}
    for lim, cordon in cordons if cordons is not None else [(lim, ()) for lim in FIT_LIMITS]:
        out[(lim, tuple(cordon))] = s.node_drain(None, [names.index(c) for c in cordon], lim)
    if cordons is None:
        own = ds.pick_cordon({r["node"]: r for r in out[(FIT_LIMITS[-1], ())] if r["valid"]})
        out.setdefault((FIT_LIMITS[-1], tuple(names[c] for c in own)), s.node_drain(None, own, FIT_LIMITS[-1]))
    return out


def ask(s, uids, k=0, cordons=None):
    """All seven calls on every job and node of `s` and on the tasks `uids`, in
    call_order(k), raw and named. `cordons`: [(limit, node names)] for
    kbg_node_drain (drain_questions). A call of the three later ones that is
    refused leaves None."""
    tix = {t.uid: i for i, t in enumerate(s.flat.task_objs) if t is not None}
    tasks = [tix[u] for u in uids]
    names, objs = s.flat.node_names, s.flat.task_objs
    raw = dict(task=None, room=None, job=[], victim=None, fit=None, node=None, drain=None)

    def job():
        for j in range(len(s.jobs)):
            r = s.job_reasons(j)
            raw["job"].append((r.valid, r.task, r.before, r.visited, list(r.count), list(r.first_node)))

    def victim():
        try:
            raw["victim"] = {mode: [ws.why_fields(w) for w in s.victim_reasons(mode)] for mode in qr.MODES}
        except _abi.KbgError as e:
            if e.status != "invalid":
                raise

    def later(what, rows_of):
        try:
            raw[what] = rows_of()
        except _abi.KbgError as e:
            if e.status != "invalid":
                raise

    calls = dict(job=job, victim=victim, task=lambda: raw.update(task=s.task_reasons(tasks)),
                 room=lambda: raw.update(room={lim: s.task_headroom(tasks, lim) for lim in LIMITS}),
                 fit=lambda: later("fit", lambda: {lim: s.job_fit(None, lim) for lim in FIT_LIMITS}),
                 node=lambda: later("node", s.node_reasons),
                 drain=lambda: later("drain", lambda: drain_questions(s, cordons)))
    for what in call_order(k):
        calls[what]()
    uid = lambda t: objs[t].uid  # noqa: E731
    at = lambda n: _name(names, n)  # noqa: E731

    def walk(r, key, own):  # a kbg_job_fit or kbg_node_drain row: the tasks by uid, the nodes by name
        if not r["valid"]:
            return dict(r, **{key: own}, first_unplaced=None, places=[])
        return dict(r, **{key: own}, first_unplaced=uid(r["first_unplaced"]) if r["first_unplaced"] >= 0 else None,
                    places=[(uid(t), at(n), kind) for t, n, kind in r["places"]])
    # (a row that is not valid is all zeros, its task index included: the rows are in the order asked)
    named = dict(
        task={u: dict(r, task=u, first_node=[_name(names, n) for n in r["first_node"]])
              for u, r in zip(uids, raw["task"])},
        room={lim: {u: dict(r, task=u, first_node=_name(names, r["first_node"])) for u, r in zip(uids, rows)}
              for lim, rows in raw["room"].items()},
        job={s.jobs[j].uid: (v, uid(t) if v else None, b, vis, c, [_name(names, n) for n in f] if v else f)
             for j, (v, t, b, vis, c, f) in enumerate(raw["job"])},
        victim=None if raw["victim"] is None else {
            mode: {s.jobs[j].uid: dict(valid=v, task=uid(t) if v else None, visited=vis, queue_overused=o, count=c,
                                       first_node=[_name(names, n) for n in f] if v else f, fn_empty=fe)
                   for j, (v, t, vis, o, c, f, fe) in enumerate(rows)} for mode, rows in raw["victim"].items()},
        fit=None if raw["fit"] is None else {
            lim: {s.jobs[j].uid: walk(r, "job", s.jobs[j].uid) for j, r in enumerate(rows)}
            for lim, rows in raw["fit"].items()},
        node=None if raw["node"] is None else {
            names[i]: dict(r, node=names[i],
                           first_task=[uid(t) if t >= 0 and r["valid"] else None for t in r["first_task"]])
            for i, r in enumerate(raw["node"])},
        drain=None if raw["drain"] is None else {
            key: {names[i]: walk(r, "node", names[i]) for i, r in enumerate(rows)}
            for key, rows in raw["drain"].items()})
    for what in ("fit", "drain"):  # (the rows are in the order asked: every job, every node)
        for rows in (raw[what] or {}).values():
            assert all(not r["valid"] or r["job" if what == "fit" else "node"] == i for i, r in enumerate(rows)), rows
    assert all(not r["valid"] or r["node"] == i for i, r in enumerate(raw["node"] or [])), raw["node"]
    for u, t, r in zip(uids, tasks, raw["task"]):
        assert not r["valid"] or r["task"] == t, (u, t, r)
    return raw, named


def n_rows(named):
    return len(named["task"]) * (1 + len(LIMITS)) + len(named["job"]) + len(named["node"] or ()) + \
        sum(len(v) for what in ("victim", "fit", "drain") for v in (named[what] or {}).values())


def valid_only(named):
    """The named rows as query_update_ref.compare_point takes them: the valid ones, without `valid`."""
    def strip(r):
        return {k: v for k, v in r.items() if k != "valid"}
    return dict(task={u: r for u, r in named["task"].items() if r["valid"]},
                room={lim: {u: r for u, r in rows.items() if r["valid"]} for lim, rows in named["room"].items()},
                victim=None if named["victim"] is None else {
                    mode: {j: strip(r) for j, r in rows.items() if r["valid"]}
                    for mode, rows in named["victim"].items()},
                fit=None if named["fit"] is None else {
                    lim: {j: r for j, r in rows.items() if r["valid"]} for lim, rows in named["fit"].items()},
                node=None if named["node"] is None else {n: r for n, r in named["node"].items() if r["valid"]},
                drain=None if named["drain"] is None else {
                    key: {n: r for n, r in rows.items() if r["valid"]} for key, rows in named["drain"].items()})


def diff_named(a, b, tag, by_uid_only=False):
    """Differences of two sessions' named rows, said by query, uid and field.
    `by_uid_only`: the two number their tasks differently, so the lowest task
    of a cause in kbg_node_reasons is another task in each: only whether there
    is one is compared."""
    errs = []
    for what in ("task", "job"):
        errs += _diff_rows(a[what], b[what], f"{tag}: {what}")
    for lim in LIMITS:
        errs += _diff_rows(a["room"][lim], b["room"][lim], f"{tag}: headroom, limit {lim}")
    if (a["victim"] is None) != (b["victim"] is None):
        errs.append(f"{tag}: kbg_victim_reasons is refused by one session only")
    elif a["victim"] is not None:
        for mode in qr.MODES:
            errs += _diff_rows(a["victim"][mode], b["victim"][mode], f"{tag}: victim mode {mode}")
    for what, call in (("fit", "kbg_job_fit"), ("node", "kbg_node_reasons"), ("drain", "kbg_node_drain")):
        if a[what] is None or b[what] is None:
            if (a[what] is None) != (b[what] is None):
                errs.append(f"{tag}: {call} is refused by one session only")
            continue
        if what == "node":
            lose = (lambda r: dict(r, first_task=[u is not None for u in r["first_task"]])) if by_uid_only else dict
            errs += _diff_rows({n: lose(r) for n, r in a[what].items()}, {n: lose(r) for n, r in b[what].items()},
                               f"{tag}: node reasons")
        elif sorted(a[what]) != sorted(b[what]):
            errs.append(f"{tag}: {call} asked for {sorted(a[what])}, the fresh session for {sorted(b[what])}")
        else:
            for key in a[what]:
                errs += _diff_rows(a[what][key], b[what][key], f"{tag}: {call}, {key}")
    return errs


def _diff_rows(a, b, tag):
    if sorted(a) != sorted(b):
        return [f"{tag}: rows of {sorted(a)}, the fresh session's {sorted(b)}"]
    errs = []
    for k in a:
        if a[k] != b[k]:
            if isinstance(a[k], dict):
                bad = {f: (a[k][f], b[k][f]) for f in a[k] if a[k][f] != b[k][f]}
            else:
                bad = (a[k], b[k])
            errs.append(f"{tag}: {k}: {bad} (updated session, fresh session)")
    return errs


def call_action(s, name, buf, cap, n):
    code = getattr(_abi.lib(), ws.ENTRY[name])(s.handle, buf, cap, ctypes.byref(n))
    if code in (_abi.KBG_E_REF_PANIC, _abi.KBG_E_UNSUPPORTED):
        return _abi.STATUS_NAMES[code]
    _abi.check(code)
    return "ok"


def log_of(s, buf, n):
    return [(s.flat.task_objs[buf[i].task].uid, s.flat.node_names[buf[i].node],
             "allocate" if buf[i].kind == _abi.KIND_ALLOCATE else "pipeline") for i in range(n.value)]


def node_rows(s):
    out = []
    for i, name in enumerate(s.flat.node_names):
        st = s.node_state(i)
        out.append((name, [st.idle.milli_cpu, st.idle.memory, st.idle.milli_gpu],
                    [st.releasing.milli_cpu, st.releasing.memory, st.releasing.milli_gpu], st.num_tasks))
    return out


def check_rounds(fx0, rounds_of, opts=None, staged=False, probe=None, first_point=0):
    """`rounds_of`: one callable per update, (session or view, the fixture
    after the rounds before or None) -> change list. `staged`: the first batch
    is sent right after a cycle that ended in preempt and was not asked, with
    no reset before it (the staged deltas of its evictions are still to push).
    Returns a dict: errors, rows (compared), skipped (a refusal's text or
    None), rebuilds (per round), n_classes (at the warm-up and after each
    update), rows0 and s1 (named rows at the warm-up and after the last
    round's last action) and what the caller asserts from the counters. That
    the update is visible to the calls at all is not checked here: the task
    sets alone make rows0 and s1 differ; tests/test_query_update_ref.py shows
    it from the references. `probe`: () -> {counter: launches so far} (hostsim's); `launches`
    then sums the launches of the updated session's own calls after its
    updates, and `stage_mask` holds, per round, the stage-plane builds between
    the update and the end of its first calls. `round_launches` holds the
    same counters per round, `drain_plain_walk` whether a kbg_node_drain walk
    of the round held a pod without a host port, `rows_ref_by` the reference
    rows compared per later call ("fit", "node", "drain"), `pod_affinity` the
    fixture's flag per round, `first_asked` the call asked first after each
    update. `first_point`: the ordinal of the warm-up's
    point (module docstring)."""
    L = _abi.lib()
    probe = probe or (lambda: {})

    res = dict(errors=[], rows=0, rows_ref=0, skipped=None, rebuilds=[], by_uid_only=[], answered=[], launches={},
               stage_mask=[], host_only=[], evicted0=0, n_classes=[], rows_ref_by={}, round_launches=[],
               drain_plain_walk=[], pod_affinity=[], first_asked=[])

    def asked(s, uids, k, cordons, snaps, tag):
        """ask, and the three later calls' self-checks, with the launches counted."""
        c0 = probe()
        raw, got = ask(s, uids, k, cordons)
        if raw["fit"] is not None and raw["node"] is not None and raw["drain"] is not None:
            top = FIT_LIMITS[-1]
            switches = {name: os.environ.get(name) for name in HOST_SWITCHES}
            res["errors"] += ns.transpose(s, raw["node"], tag)[0]
            res["errors"] += js.invariants(s, snaps[0], raw["fit"][top], top, tag)
            res["errors"] += ds.invariants(s, snaps[1], raw["drain"][(top, ())], top, (), tag)
            for name, v in switches.items():  # (the self-checks set and clear their own call's switch)
                if v is not None:
                    os.environ[name] = v
        for name, v in probe().items():
            res["launches"][name] = res["launches"].get(name, 0) + v - c0[name]
            res["round_launches"][-1][name] = res["round_launches"][-1].get(name, 0) + v - c0[name]
        return raw, got

    errs = res["errors"]
    actions = qr.actions_of(fx0)
    ssn, _ = ws.open_with_reasons(fx0, opts)
    try:
        cap = 4 * len(ssn.flat.task_objs) + 64
        buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
        for name in actions:
            if (status := call_action(ssn, name, buf, cap, n)) != "ok":
                res["skipped"] = f"S0: {name} ends {status}"
                return res
        uids0 = [t.uid for t in ssn.flat.task_objs if t is not None]
        _, rows0 = ask(ssn, uids0, first_point)
        for what in ("fit", "node", "drain"):
            if rows0[what] is None:
                errs.append(f"S0: the call of {what!r} was refused")
        point = first_point + 1  # the ordinal of the session's next asked point: it sets the order of the seven calls
        ev, ne = (_abi.kbg_eviction * cap)(), ctypes.c_int32(0)
        _abi.check(L.kbg_evictions_get(ssn.handle, ev, cap, ctypes.byref(ne)))
        res["evicted0"] = ne.value
        res["rows0_pending"] = sum(r["valid"] for r in rows0["task"].values())
        if staged:
            _abi.check(L.kbg_session_reset(ssn.handle))
            for name in actions:
                if (status := call_action(ssn, name, buf, cap, n)) != "ok":
                    res["skipped"] = f"S0, the cycle that is not asked: {name} ends {status}"
                    return res
        res["n_classes"].append(ssn.stats().n_classes)
        done, rebuilt = [], 0
        for r, changes_of in enumerate(rounds_of):
            tag0 = f"round {r}"
            old_order = {"jobs": [j.uid for j in ssn.jobs], "nodes": list(ssn.flat.node_names),
                         "queues": [q.uid for q in ssn.queues]}
            fx_now = fixture_after(fx0, done) if done else fx0
            if fx_now is None:
                res["skipped"] = f"{tag0}: no fixture says the cache after the rounds before"
                return res
            if not (staged and r == 0):
                _abi.check(L.kbg_session_reset(ssn.handle))
            changes = changes_of(ssn, fx_now)
            built = probe().get("stage_mask", 0)
            try:
                ssn.update(changes)
            except ValueError as e:
                res["skipped"] = f"{tag0}: the update needs a re-open: {e}"
                return res
            except _abi.KbgError as e:
                if e.status not in ("unsupported", "ref_panic"):
                    raise
                res["skipped"] = f"{tag0}: the update was refused: {e}"
                return res
            done.append(changes)
            total = ssn.stats().update_rebuilds  # (counted since the session's open, read right after an update)
            res["rebuilds"].append(total - rebuilt)
            res["n_classes"].append(ssn.stats().n_classes)
            rebuilt = total
            order = {"jobs": [j.uid for j in ssn.jobs], "nodes": list(ssn.flat.node_names),
                     "queues": [q.uid for q in ssn.queues]}
            # what tests/test_query_update_ref.py takes for S1's numbering: the old order, the new names after it
            if qr.order_of(qr.view_of(replay(fx0, done), old_order, fx0)) != order:
                errs.append(f"{tag0}: the session's order {order} is not the cache's snapshot in the old order")
            fssn = open_session(_OrderedCache(replay(fx0, done), {"sessionOrder": order}), fixture_tiers(fx0),
                                dict(opts or {}), reasons=True)
            try:
                if [j.uid for j in fssn.jobs] != order["jobs"] or list(fssn.flat.node_names) != order["nodes"] or \
                        [q.uid for q in fssn.queues] != order["queues"]:
                    errs.append(f"{tag0}: the fresh session is not in the updated session's order")
                    return res
                live = [t.uid for t in fssn.flat.task_objs if t is not None]
                pending = {t.uid for t in fssn.flat.task_objs if t is not None and t.status == PENDING}
                same_numbers = [t.uid if t is not None else None for t in ssn.flat.task_objs] == \
                    [t.uid if t is not None else None for t in fssn.flat.task_objs]
                res["by_uid_only"].append(not same_numbers)
                mine = {t.uid for t in ssn.flat.task_objs if t is not None}
                if set(live) - mine:
                    errs.append(f"{tag0}: the updated session holds no task {sorted(set(live) - mine)[:5]}")
                    return res
                numbers = {t.uid: i for i, t in enumerate(ssn.flat.task_objs) if t is not None}
                fx1 = fixture_after(fx0, done)
                refs = None
                if fx1 is not None and not fx0.get("namespaces"):
                    refs = qr.reference_points(fx1, order, actions, task_numbers=numbers)
                    if qr.order_of(refs.view) != order:
                        errs.append(f"{tag0}: the session's order {order} is not the fixture's in the old order "
                                    f"{qr.order_of(refs.view)}")
                        refs = None
                aff = ts.has_pod_affinity(fx1 or fx0)
                res["pod_affinity"].append(aff)
                # the library answers on the host alone with host ports, pod affinity or a nil Node
                res["host_only"].append(fx1 is None or aff or ts.has_host_ports(fx1) or any(
                    p.get("nodeName") and p["nodeName"] not in order["nodes"] for p in fx1["pods"]))
                fbuf, fn = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
                # what the self-checks read of a session at open, from the fresh one (the updated session's Python
                # mirror is not kept task by task), with the tasks in the updated session's own numbering
                snaps = (js.Snap(fssn), ds.Snap(fssn))
                snaps[0].by_task = {numbers[v[0]]: v for v in snaps[0].by_task.values()}
                fresh_uid = {i: u for u, i in snaps[1].mirror.task_index.items()}
                snaps[1].task_job = {numbers[fresh_uid[t]]: j for t, j in snaps[1].task_job.items()}
                asks_room = {t.uid for t in fssn.flat.task_objs if t is not None and t.status == PENDING
                             and not ts.empty([float(v) for v in t.resreq.as_tuple()])}
                job_of = {t.uid: j.uid for j in fssn.jobs for t in j.tasks.values()}
                res["round_launches"].append({})
                res["first_asked"].append(call_order(point)[0])
                res["drain_plain_walk"].append(False)
                for k in range(len(actions) + 1):
                    when = "before the first action" if k == 0 else f"after {actions[k - 1]}"
                    tag = f"{tag0}, {when}"
                    n_errs = len(errs)
                    if k:
                        a, b = call_action(ssn, actions[k - 1], buf, cap, n), call_action(fssn, actions[k - 1], fbuf, cap, fn)
                        if a != b:
                            errs.append(f"{tag}: the action ends {a}, the fresh session's {b}")
                        if a != "ok" or b != "ok":
                            res["skipped"] = f"{tag}: the action ends {a}"
                            return res
                    cordons = None if refs is None or refs.points[k]["drain"] is None else list(refs.points[k]["drain"])
                    raw, got = asked(ssn, live, point, cordons, snaps, tag)
                    if k == 0:  # (the fresh session has not asked yet: these builds are the updated session's)
                        res["stage_mask"].append(probe().get("stage_mask", 0) - built)
                    refused = [what for what in ("fit", "node", "drain") if got[what] is None]
                    if refused:
                        errs.append(f"{tag}: the calls of {refused} were refused")
                        return res
                    fraw, want = ask(fssn, live, point, list(got["drain"]))
                    errs += diff_named(got, want, tag, not same_numbers)
                    if same_numbers and raw != fraw:
                        errs.append(f"{tag}: the rows of {[what for what in raw if raw[what] != fraw[what]]} differ "
                                    f"index by index from the fresh session's")
                    res["rows"] += n_rows(got)
                    if k == 0:
                        left = pending
                        if got["victim"] is not None:
                            errs.append(f"{tag}: kbg_victim_reasons answered before the cycle's first action")
                        if any(row[0] for row in got["job"].values()):
                            errs.append(f"{tag}: kbg_job_reasons is valid before the cycle's first action")
                    else:
                        left = pending - {d[0] for d in log_of(ssn, buf, n)}
                    answered = {u for u, row in got["task"].items() if row["valid"]}
                    res["answered"].append(len(answered))
                    for lim in LIMITS:
                        if {u for u, row in got["room"][lim].items() if row["valid"]} != answered:
                            errs.append(f"{tag}: kbg_task_headroom (limit {lim}) and kbg_task_reasons answer for "
                                        f"different tasks")
                    if answered != left:
                        errs.append(f"{tag}: rows for {sorted(answered)}, Pending {sorted(left)}")
                    # the three later calls answer for exactly what the cycle leaves: the jobs that hold a Pending
                    # task with a request, every live node
                    fit_left = sorted({job_of[u] for u in left & asks_room})
                    for lim in FIT_LIMITS:
                        if sorted(j for j, row in got["fit"][lim].items() if row["valid"]) != fit_left:
                            errs.append(f"{tag}: kbg_job_fit (limit {lim}) answers for "
                                        f"{sorted(j for j, row in got['fit'][lim].items() if row['valid'])}, the jobs "
                                        f"with a Pending task with a request are {fit_left}")
                    if [nm for nm, row in got["node"].items() if row["valid"]] != order["nodes"]:
                        errs.append(f"{tag}: kbg_node_reasons answers for "
                                    f"{[nm for nm, row in got['node'].items() if row['valid']]}, live {order['nodes']}")
                    for key, rows in got["drain"].items():
                        if [nm for nm, row in rows.items() if row["valid"]] != order["nodes"]:
                            errs.append(f"{tag}: kbg_node_drain {key} answers for "
                                        f"{[nm for nm, row in rows.items() if row['valid']]}, live {order['nodes']}")
                        # (the drain kernel takes a walk only where it holds a pod without a host port)
                        res["drain_plain_walk"][-1] |= any(not rr._ports(ssn.flat.task_objs[t].pod)
                                                           for row in raw["drain"][key] for t, _, _ in row["places"])
                    if refs is not None:
                        e, said = qr.compare_point(refs.points[k], valid_only(got), aff, tag, res["rows_ref_by"])
                        errs += e
                        res["rows_ref"] += said
                        if k and actions[k - 1] == "allocate" and not aff:
                            log = refs.points[k]["ref"]["decisions"]
                            for j, (v, t, before, vis, c, f) in got["job"].items():
                                if v:
                                    w = qr.job_reason_row(refs, log, t, before)
                                    if (vis, c, f) != tuple(w):
                                        errs.append(f"{tag}: kbg_job_reasons of {j}: {(vis, c, f)}, reference {w}")
                                    res["rows_ref"] += 1
                    if k == len(actions):
                        res["s1"] = got
                    if len(errs) > n_errs:
                        errs.append(f"{tag}: the seven calls were asked in the order {call_order(point)}")
                    point += 1
                # the cycle itself: the oracle's where a fixture says S1, else the fresh session's
                log = log_of(ssn, buf, n)
                if refs is not None:
                    ref = refs.points[-1]["ref"]
                    if log != [(d["task"], d["node"], d["kind"]) for d in ref["decisions"]]:
                        errs.append(f"{tag0}: the decision log differs from the oracle's")
                    by = {x["name"]: x for x in ref["nodes"]}
                    for name, idle, rel, nt in node_rows(ssn):
                        if (idle, rel, nt) != (by[name]["idle"], by[name]["releasing"], by[name]["ntasks"]):
                            errs.append(f"{tag0}: node {name} ends differently from the oracle's")
                if log != log_of(fssn, fbuf, fn) or node_rows(ssn) != node_rows(fssn):
                    errs.append(f"{tag0}: the cycle differs from the fresh session's")
            finally:
                fssn.close()
        res["rows0"] = rows0
        res["ref"] = refs is not None
    finally:
        ssn.close()
    return res


def check_queries_after_update(fx0, changes_of, opts=None):
    """check_rounds for one update (`changes_of`: session -> change list): the
    list of differences. A refused update and a comparison of no row are
    differences too: no committed case may be skipped."""
    res = check_rounds(fx0, [lambda s, fx: changes_of(s)], opts)
    errs = list(res["errors"])
    if res["skipped"]:
        errs.append(f"skipped: {res['skipped']}")
    elif not res["rows"]:
        errs.append("no row compared")
    return errs


def host_paths():
    """HOST_SWITCHES for the block's calls (read per call)."""
    class _Env:
        def __enter__(self):
            for name in HOST_SWITCHES:
                os.environ[name] = "1"

        def __exit__(self, *exc):
            for name in HOST_SWITCHES:
                del os.environ[name]
    return _Env()
