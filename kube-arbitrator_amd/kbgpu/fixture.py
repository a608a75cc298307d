"""Runs a JSON fixture (the schema the kbref oracle reads) through the device
path and reports the same fields the oracle prints, for parity checks."""
from . import _abi, actions
from .api import RefPanic
from .cache import FakeBinder, cache_from_fixture
from .conf import tiers_from_list, load_scheduler_conf
from .framework import get_action, open_session


def fixture_tiers(fx):
    if fx.get("tiers") is None:
        return load_scheduler_conf()[1]
    return tiers_from_list(fx["tiers"])


def session_order(ssn, fx):
    """Applies an explicit `sessionOrder` before marshaling."""
    so = fx.get("sessionOrder") or {}

    def reorder(items, keys, key):
        if not keys:
            return items
        pos = {k: i for i, k in enumerate(keys)}
        first = [x for x in sorted(items, key=lambda x: pos.get(key(x), 1 << 30)) if key(x) in pos]
        return first + [x for x in items if key(x) not in pos]

    return (reorder(ssn.nodes, so.get("nodes"), lambda n: n.name),
            reorder(ssn.jobs, so.get("jobs"), lambda j: j.uid),
            reorder(ssn.queues, so.get("queues"), lambda q: q.uid))


class _OrderedCache:
    """Wraps a SchedulerCache so snapshot() honours the fixture's sessionOrder."""

    def __init__(self, cache, fx):
        self._c = cache
        self._fx = fx

    def __getattr__(self, k):
        return getattr(self._c, k)

    def snapshot(self):
        s = self._c.snapshot()
        s.nodes, s.jobs, s.queues = session_order(s, self._fx)
        return s


def fit_error(nodes, cpu, memory, gpu):
    """JobInfo.FitError (job_info.go:329-358) from NodesFitDelta counts."""
    if nodes == 0:
        return "0 nodes are available"
    reasons = [f"{v} insufficient {k}" for k, v in (("cpu", cpu), ("memory", memory), ("GPU", gpu)) if v > 0]
    return f"0/{nodes} nodes are available, {', '.join(sorted(reasons))}."


# The predicates plugin's error per stage (predicates.go:125-198), without the
# names it formats in, in kbg_job_reasons.count order.
STAGE_TEXTS = ("can not allow more task running on it", "didn't match node selector",
               "didn't have available host ports", "set to unschedulable", "does not tolerate node taints",
               "affinity/anti-affinity failed")


def unschedulable_message(reasons, fit=None):
    """One line, kube-scheduler style, for a job that did not get ready: the
    nodes its last evaluated task visited by the predicate stage that turned
    them away (kbg_job_reasons), then FitError's resource parts for the nodes
    that passed them all (kbg_job_state). Each group is sorted as FitError
    sorts its own (sort.Strings of the "<n> <text>" parts)."""
    if not reasons.valid or reasons.visited == 0:
        return "0 nodes are available"
    parts = sorted(f"{n} {text}" for n, text in zip(reasons.count, STAGE_TEXTS) if n > 0)
    if fit is not None and fit.fit_valid:
        parts += sorted(f"{v} insufficient {k}" for k, v in (("cpu", fit.fit_cpu), ("memory", fit.fit_memory),
                                                            ("GPU", fit.fit_gpu)) if v > 0)
    if not parts:
        return f"0/{reasons.visited} nodes are available."
    return f"0/{reasons.visited} nodes are available: {', '.join(parts)}."


def pending_message(row):
    """One line, kube-scheduler style, for a Pending task (a Session.
    task_reasons row): the nodes that would take it now when there are any,
    else the live nodes by the predicate stage that turns them away and
    FitError's resource parts over the nodes that pass every stage but lack
    Idle resources, each group sorted as unschedulable_message sorts its own."""
    if not row["valid"]:
        return "not pending"
    count, total = row["count"], row["visited"]
    if total == 0:
        return "0 nodes are available"
    fits = count[_abi.TWHY_FITS_IDLE] + count[_abi.TWHY_FITS_RELEASING]
    tail = " (its queue is overused)" if row["queue_overused"] else ""
    if fits:
        rel = count[_abi.TWHY_FITS_RELEASING]
        return f"{fits}/{total} nodes are available" + (f", {rel} of them once resources are released" if rel else "") \
            + f".{tail}"
    parts = sorted(f"{n} {text}" for n, text in zip(count, STAGE_TEXTS) if n > 0)
    if count[_abi.TWHY_PANIC]:
        parts.append(f"{count[_abi.TWHY_PANIC]} have no Node object")
    parts += sorted(f"{v} insufficient {k}" for k, v in zip(("cpu", "memory", "GPU"), row["idle_short"]) if v > 0)
    if not parts:
        return f"0/{total} nodes are available.{tail}"
    return f"0/{total} nodes are available: {', '.join(parts)}.{tail}"


def headroom_message(row, needed):
    """One line for a job that still needs `needed` members (a Session.
    task_headroom row of one of its Pending tasks): how many of them have room
    now, how many more on resources that are being released, on how many
    nodes; "lower bound" where the call's limit cut a node's count."""
    if not row["valid"]:
        return "not pending"
    nodes = row["nodes_idle"] + row["nodes_releasing_only"]
    tail = ", lower bound" if row["limit_hit"] else ""
    tail += " (pod affinity as it is now)" if row["affinity_now"] else ""
    tail += " (its queue is overused)" if row["queue_overused"] else ""
    return (f"needs {needed} more; room for {row['copies_idle']} now, {row['copies_releasing']} more on releasing "
            f"resources ({nodes} nodes){tail}")


def job_fit_message(row):
    """One line for a job that is not ready (a Session.job_fit row): how many
    of its next pending pods fit now, from Idle and from resources that are
    being released, on how many nodes, and either the pod after which the gang
    has enough or the first task without room."""
    if not row["valid"]:
        return "nothing pending"
    needed = max(0, row["min_available"] - row["ready_num"])
    placed = row["placed_idle"] + row["placed_releasing"]
    if row["ready_after"] >= 0:
        end = f"enough after pod {row['ready_after']}"
    elif row["first_unplaced"] >= 0:
        end = f"not enough, first without room: task {row['first_unplaced']}"
    else:
        end = "not enough"
    tail = f", {row['pending'] - row['walked']} not walked" if row["pending"] > row["walked"] else ""
    tail += " (pod affinity as it is now)" if row["affinity_now"] else ""
    tail += " (its queue is overused)" if row["queue_overused"] else ""
    return (f"needs {needed} more; {placed} of its next {row['walked']} pending pods fit now "
            f"({row['placed_idle']} on idle, {row['placed_releasing']} on releasing resources, "
            f"{row['nodes_used']} nodes): {end}{tail}")


def node_message(row):
    """One line for a node (a Session.node_reasons row): how many of the
    pending pods it would take now and once resources are released, then the
    pods it turns away by predicate stage and FitError's resource parts over
    the pods that pass every stage but find too little Idle here, each group
    sorted as pending_message sorts its own."""
    if not row["valid"]:
        return "not a live node"
    count, total = row["count"], row["pending"]
    if total == 0:
        return "no pods are pending"
    idle, rel = count[_abi.TWHY_FITS_IDLE], count[_abi.TWHY_FITS_RELEASING]
    head = f"takes {idle} of {total} pending pods now"
    if idle:
        head += f" ({row['open_idle']} in queues that are not overused, {row['idle_best_effort']} best-effort)"
    if rel:
        head += f", {rel} more once resources are released"
    parts = sorted(f"{n} {text}" for n, text in zip(count, STAGE_TEXTS) if n > 0)
    if count[_abi.TWHY_PANIC]:
        parts.append(f"{count[_abi.TWHY_PANIC]} no Node object")
    if count[_abi.TWHY_SHORT]:
        parts += sorted(f"{v} insufficient {k}" for k, v in zip(("cpu", "memory", "GPU"), row["idle_short"]) if v > 0)
    return head + (f"; turned away: {', '.join(parts)}" if parts else "")


def drain_message(row):
    """One line for a node an operator wants to drain (a Session.node_drain
    row): how many of the pods it holds find room elsewhere now, from Idle and
    from resources that are being released, on how many nodes, the first pod
    that does not, and the gangs that would lose their minimum."""
    if not row["valid"]:
        return "not a live node"
    if row["tasks"] == 0:
        tail = f" ({row['other_pods']} other pods stay out of the walk)" if row["other_pods"] else ""
        return "no pods to move" + tail
    placed = row["placed_idle"] + row["placed_releasing"]
    msg = (f"{placed} of {row['walked']} pods find room ({row['placed_releasing']} on releasing resources, "
           f"{row['nodes_used']} nodes)")
    if row["unplaced"]:
        msg += f"; {row['unplaced']} do not, first task {row['first_unplaced']}"
    if row["jobs_short"]:
        msg += f"; breaks {row['jobs_short']} gang" + ("s" if row["jobs_short"] > 1 else "")
    msg += f"; {row['tasks'] - row['walked']} not walked" if row["tasks"] > row["walked"] else ""
    msg += " (pod affinity as it is now)" if row["affinity_now"] else ""
    return msg


def reasons_row(st):
    """A kbg_job_reasons as the output rows carry it."""
    return {"task": st.task, "before": st.before, "visited": st.visited, "count": list(st.count),
            "first_node": list(st.first_node)}


def run_fixture(fx, options=None):
    """Returns (result dict in the oracle's output schema, session)."""
    opts = dict(options or {})
    if (fx.get("options") or {}).get("heapDownRule") == "go1.13":
        opts["heap_rule"] = 1
    binder = FakeBinder()
    try:
        cache = _OrderedCache(cache_from_fixture(fx, binder), fx)
        ssn = open_session(cache, fixture_tiers(fx), opts)
    except RefPanic as e:  # Resource.Sub underflow while building the cache/snapshot
        return {"status": "ref_panic", "error": str(e)}, None
    except _abi.KbgError as e:
        return {"status": e.status, "error": str(e)}, None
    status = "ok"
    try:
        for name in fx.get("actions") or ["allocate"]:  # conf "actions" (util.go:30-61)
            action = get_action(name)
            if action is None:
                return {"status": "bad_input", "error": f"unsupported action {name}"}, ssn
            status = action.execute(ssn).status
    except _abi.KbgError as e:
        if e.status == "unsupported":
            return {"status": "unsupported", "error": str(e)}, ssn
        if e.status != "ref_panic":
            raise
        return {"status": "ref_panic", "error": str(e)}, ssn
    return session_output(ssn, binder.binds, status), ssn


def session_output(ssn, binds, status="ok"):
    """The session's outputs in the oracle's output schema, after its actions
    have been replayed through it (actions.replay): the decision log, the
    binds the fake binder recorded, evictions, job / queue / node states (the
    latter three read from the library)."""
    tasks, names = ssn.flat.task_objs, ssn.flat.node_names
    out = {"status": status, "decisions": [], "binds": dict(binds), "jobs": [], "queues": [], "nodes": [],
           "evictions": [{"task": t.uid, "by": by.uid, "action": act} for t, by, act in ssn.evictions]}
    for (t, nd, kind, disp), act in zip(ssn.decisions, ssn.action_of):
        d = {"task": tasks[t].uid, "job": tasks[t].job, "node": names[nd],
             "kind": "allocate" if kind == _abi.KIND_ALLOCATE else "pipeline", "dispatched_at": disp}
        if act != "allocate":
            d["action"] = act
        out["decisions"].append(d)
    has_drf = any(p.name == "drf" for t in ssn.tiers for p in t.plugins)
    for j, job in enumerate(ssn.jobs):
        st = ssn.job_state(j)
        row = {"uid": job.uid, "queue": job.queue, "ready_num": st.ready_num, "min_available": job.min_available,
               "ready": bool(st.ready), "allocated": list(job.allocated.as_tuple())}
        if has_drf:
            row["drf_share"] = st.drf_share
        if st.fit_valid:
            row["fit_error"] = fit_error(st.fit_nodes, st.fit_cpu, st.fit_memory, st.fit_gpu)
        if getattr(ssn, "reasons", False):  # only sessions opened with reasons: every other output is as before
            why = ssn.job_reasons(j)
            if why.valid:
                row["reasons"] = dict(reasons_row(why), message=unschedulable_message(why, st))
        out["jobs"].append(row)
    for q, queue in enumerate(ssn.queues):
        st = ssn.queue_state(q)
        if st.has_attr:
            out["queues"].append({"uid": queue.uid, "share": st.share,
                                  "deserved": [st.deserved.milli_cpu, st.deserved.memory, st.deserved.milli_gpu],
                                  "allocated": [st.allocated.milli_cpu, st.allocated.memory, st.allocated.milli_gpu],
                                  "request": [st.request.milli_cpu, st.request.memory, st.request.milli_gpu]})
    for i, n in enumerate(ssn.nodes):
        st = ssn.node_state(i)
        out["nodes"].append({"name": n.name, "idle": [st.idle.milli_cpu, st.idle.memory, st.idle.milli_gpu],
                             "releasing": [st.releasing.milli_cpu, st.releasing.memory, st.releasing.milli_gpu],
                             "ntasks": st.num_tasks})
    return out
