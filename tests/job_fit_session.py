"""Session-level checks of kbg_job_fit, shared by the hostsim tests
(tests/test_hostsim_job_fit.py, through tests/job_fit_worker.py) and the
device tests (tests/test_job_fit_gpu.py).

`check_fixture` opens a session with reasons and, for each action prefix of
tests/task_why_session.py, runs the prefix and asks for the rows of every job.
The expected places are built as tests/headroom_session.py builds its rows,
without the library: node Idle, Releasing and pod counts from the ORACLE's
output of the same prefix, the Pending tasks and the pods a node holds from
the mirror at open plus the oracle's decisions, the stages from
reasons_ref.first_failing_stage against the job's own view (its placements'
pods join the node's), the walk in plain Python. reasons_ref has no inter-pod
affinity stage: sessions with pod affinity are held to the invariants alone;
tests/golden/kat_job_fit.json holds hand-derived host-port and pod-affinity
walks. Seeds whose cycle discards a statement after evicting get no expected
rows on sessions with host ports (tests/task_why_session.py: the same rule).

Against the other calls on the same session, whatever it holds:
  the first walked task is placed iff its kbg_task_reasons row has
  count[FITS_IDLE] + count[FITS_RELEASING] > 0, on the lower of the two
  first_nodes, an Allocate iff that one is FITS_IDLE's;
  a job whose walked tasks are copies of one pod, against kbg_task_headroom at
  limit 1024 with limit_hit == 0: placed == min(walked, copies), and when the
  walk took them all the two sums and the node count are headroom's;
  the places at limit L are the first L at limit 512; a subset of jobs asked
  by index equals their rows of the whole call; KBG_HOST_JOB_FIT=1 gives the
  same rows.

`check_allocate` is independent of all that: for a job J of a fixture without
pod affinity every other job's Pending pods are deleted, `proportion` is
stripped from the tiers and the ORACLE runs allocate alone: its decisions for
J, in order, are the call's placed entries, and J's Pending pods with a
request that it leaves undecided are the entries with node -1."""
import json
import os

import job_fit_ref as jr
import reasons_ref as rr
import task_why_ref as tr
import task_why_session as ts
import victim_why_session as ws
from helpers import run_oracle
from kbgpu import _abi
from kbgpu.api import PENDING
from kbgpu.fixture import job_fit_message

PREFIXES, REST = ts.PREFIXES, ts.REST
KINDS = {"allocate": jr.ALLOCATE, "pipeline": jr.PIPELINE}
BIG = _abi.FIT_MAX_LIMIT
DERIVED = ("walked", "placed_idle", "placed_releasing", "first_unplaced", "nodes_used", "ready_after")


class Snap(ts.OpenSnap):
    """OpenSnap, and per job its Pending tasks at open as (task index, uid, priority)."""

    def __init__(self, ssn):
        super().__init__(ssn)
        self.job_uids = [j.uid for j in ssn.jobs]
        self.job_min = [j.min_available for j in ssn.jobs]
        jidx = {u: i for i, u in enumerate(self.job_uids)}
        self.by_task = {t: (uid, req, pod, queue) for t, uid, req, pod, queue in self.pending}
        self.job_tasks = [[] for _ in ssn.jobs]
        for t, obj in enumerate(ssn.flat.task_objs):
            if obj is not None and obj.status == PENDING:
                self.job_tasks[jidx[obj.job]].append((t, obj.uid, obj.priority))


def walk_order(tasks, task_prio):
    """TaskOrderFn: the priority plugin's order, then the UID's bytes."""
    return sorted(tasks, key=lambda x: ((-x[2] if task_prio else 0), x[1].encode()))


def expected_rows(snap, fx, ref, rules, limit):
    """{job index: row} of every job with a Pending task with a request after
    the oracle's prefix (ref: its output; snap.state: no action yet: ready_num
    and queue_overused are None there, not compared)."""
    pods = {p["uid"]: p for p in fx["pods"]}
    decided = {d["task"] for d in ref["decisions"]}
    by_name = {n["name"]: n for n in ref["nodes"]}
    held0 = [dict(h) for h in snap.held]
    index = {name: i for i, (name, _, _) in enumerate(snap.nodes)}
    for d in ref["decisions"]:
        held0[index[d["node"]]].setdefault(rr.pod_key(pods[d["task"]]), pods[d["task"]])
    queues = {q["uid"]: q for q in ref["queues"] or []}
    ready = {j["uid"]: j["ready_num"] for j in ref.get("jobs") or []}
    panic = sum(1 for _, node, _ in snap.nodes if node is None) if rules["predicates"] else 0
    out = {}
    for j, tasks in enumerate(snap.job_tasks):
        todo = [x for x in walk_order(tasks, rules["task_prio"])
                if x[1] not in decided and not ts.empty(snap.by_task[x[0]][1])]
        if not todo:
            continue
        view = {}  # node index -> [idle, releasing, ntasks, held]
        places = []
        for t, uid, _ in todo[:limit]:
            _, req, pod, _ = snap.by_task[t]
            at, kind = -1, jr.ALLOCATE
            for i, (name, node, max_task_num) in enumerate(snap.nodes):
                st = view.get(i)
                if st is None:
                    o = by_name[name]
                    st = [[float(v) for v in o["idle"]], [float(v) for v in o["releasing"]], o["ntasks"], held0[i]]
                if rules["predicates"]:
                    if node is None or max_task_num <= st[2]:
                        continue
                    if rr.first_failing_stage(pod, node, 1 << 30, st[3]) >= 0:
                        continue
                if jr.less_equal(req, st[0]):
                    at, kind = i, jr.ALLOCATE
                elif jr.less_equal(req, st[1]):
                    at, kind = i, jr.PIPELINE
                else:
                    continue
                if rr.pod_key(pod) not in st[3]:  # else AddTask's error: the node is unchanged (node_info.go:101-106)
                    st = [list(st[0]), list(st[1]), st[2] + 1, dict(st[3])]
                    if node is not None:
                        st[kind] = [st[kind][d] - req[d] for d in range(3)]
                    st[3][rr.pod_key(pod)] = pod
                    view[i] = st
                break
            places.append((t, at, kind))
        queue = snap.by_task[todo[0][0]][3]
        q = queues.get(queue)
        rn = ready.get(snap.job_uids[j]) if ref.get("jobs") else None
        row = dict(job=j, pending=len(todo), places=places, min_available=snap.job_min[j], ready_num=rn,
                   panic_nodes=panic,
                   queue_overused=None if ref["queues"] is None else bool(
                       rules["proportion"] and q is not None and
                       tr.less_equal([float(v) for v in q["deserved"]], [float(v) for v in q["allocated"]])))
        row.update(jr.rows_of(places, rn if rn is not None else 0, snap.job_min[j]))
        out[j] = row
    return out


def compare_rows(want, got, tag):
    errs = []
    valid = sorted(r["job"] for r in got if r["valid"])
    if sorted(want) != valid:
        return [f"{tag}: rows of jobs {valid}, reference {sorted(want)}"]
    for g in got:
        if not g["valid"]:
            continue
        w = want[g["job"]]
        keys = ["pending", "places", "min_available", "panic_nodes"] + [k for k in DERIVED if k != "ready_after"]
        if w["ready_num"] is not None:
            keys += ["ready_num", "ready_after"]
        if w["queue_overused"] is not None:
            keys.append("queue_overused")
        errs += [f"{tag}: job {g['job']}: {k} is {g[k]}, reference {w[k]}" for k in keys if g[k] != w[k]]
    return errs


def host_rows(ssn, jobs=None, limit=BIG):
    os.environ["KBG_HOST_JOB_FIT"] = "1"
    try:
        return ssn.job_fit(jobs, limit)
    finally:
        del os.environ["KBG_HOST_JOB_FIT"]


def copy_key(pod):
    """Equal for pods that differ in nothing but their identity."""
    return json.dumps({k: v for k, v in pod.items() if k not in ("uid", "name")}, sort_keys=True)


def invariants(ssn, snap, rows, limit, tag):
    """The rows against themselves, kbg_task_reasons, kbg_task_headroom, the other limit, the host path."""
    errs = []
    live = [r for r in rows if r["valid"]]
    firsts = [r["places"][0][0] for r in live]
    why = {w["task"]: w for w in ssn.task_reasons(firsts)} if firsts else {}
    for r in live:
        j = r["job"]
        derived = jr.rows_of(r["places"], r["ready_num"], r["min_available"])
        errs += [f"{tag}: job {j}: {k} is {r[k]}, its places give {v}" for k, v in derived.items() if r[k] != v]
        if r["walked"] != min(r["pending"], limit) or len(r["places"]) != r["walked"]:
            errs.append(f"{tag}: job {j}: walked {r['walked']} of {r['pending']} at limit {limit}")
        t0, n0, k0 = r["places"][0]
        c, f = why[t0]["count"], why[t0]["first_node"]
        cands = [(f[tr.FITS_IDLE], jr.ALLOCATE), (f[tr.FITS_RELEASING], jr.PIPELINE)]
        cands = sorted(x for x in cands if x[0] >= 0)
        want = cands[0] if c[tr.FITS_IDLE] + c[tr.FITS_RELEASING] > 0 else (-1, 0)
        if (n0, k0) != want:
            errs.append(f"{tag}: job {j}: its first task {t0} goes to {(n0, k0)}, kbg_task_reasons gives {want}")
        if r["queue_overused"] != why[t0]["queue_overused"] or r["panic_nodes"] != c[tr.PANIC]:
            errs.append(f"{tag}: job {j}: queue_overused {r['queue_overused']}, panic_nodes {r['panic_nodes']}; "
                        f"kbg_task_reasons {why[t0]['queue_overused']}, {c[tr.PANIC]}")
        msg = job_fit_message(r)
        placed = r["placed_idle"] + r["placed_releasing"]
        if not msg.startswith(f"needs {max(0, r['min_available'] - r['ready_num'])} more; {placed} of its next "
                              f"{r['walked']} pending pods fit now ({r['placed_idle']} on idle") or \
                ("not walked" in msg) != (r["pending"] > r["walked"]) or \
                ("enough after pod" in msg) != (r["ready_after"] >= 0):
            errs.append(f"{tag}: job {j}: message {msg!r}")
        # copies of one pod, no key met twice: kbg_task_headroom's per-node counts, taken in node order
        pods = [snap.by_task[t][2] for t, _, _ in r["places"] if t in snap.by_task]
        keys = {rr.pod_key(p) for p in pods}
        if len(pods) == r["walked"] and len({copy_key(p) for p in pods}) == 1 and len(keys) == len(pods) and \
                not any(k in h for k in keys for h in snap.held):
            (room,) = ssn.task_headroom([t0], 1024)
            total = room["copies_idle"] + room["copies_releasing"]
            if room["limit_hit"] == 0:
                if placed != min(r["walked"], total):
                    errs.append(f"{tag}: job {j}: {placed} of {r['walked']} copies placed, kbg_task_headroom has room "
                                f"for {total}")
                if r["walked"] >= total and (r["placed_idle"], r["placed_releasing"], r["nodes_used"]) != \
                        (room["copies_idle"], room["copies_releasing"],
                         room["nodes_idle"] + room["nodes_releasing_only"]):
                    errs.append(f"{tag}: job {j}: {r['placed_idle']} + {r['placed_releasing']} on {r['nodes_used']} "
                                f"nodes, kbg_task_headroom {room}")
    host = host_rows(ssn, None, limit)
    if host != rows:
        bad = [(a, b) for a, b in zip(rows, host) if a != b][:2]
        errs.append(f"{tag}: the device-shaped path differs from KBG_HOST_JOB_FIT=1: {bad}")
    return errs


def limits_and_subsets(ssn, rows, tag):
    errs = []
    short = ssn.job_fit(limit=2)
    for a, b in zip(rows, short):
        if a["valid"] != b["valid"] or b["places"] != a["places"][:2] or a["pending"] != b["pending"]:
            errs.append(f"{tag}: job {a['job']}: the places at limit 2 are {b['places']}, at 512 {a['places'][:3]}")
    if rows:
        pick = [len(rows) - 1, 0, len(rows) // 2]
        if ssn.job_fit(pick, BIG) != [rows[p] for p in pick]:
            errs.append(f"{tag}: jobs {pick} asked by index differ from their rows of the whole call")
    return errs


def features(rows, snap, fx=None):
    """What a set of expected rows shows (the ..._say_something tests)."""
    seen = set()
    for r in rows:
        pl = r["places"]
        placed = [p for p in pl if p[1] >= 0]
        if len({copy_key(snap.by_task[t][2]) for t, _, _ in pl}) > 1:
            seen.add("two_shapes")
        if len({p[1] for p in placed}) < len(placed):
            seen.add("two_on_one_node")
        if any(p[2] == jr.PIPELINE for p in placed):
            seen.add("pipeline")
        if any(a[1] < 0 <= b[1] for i, a in enumerate(pl) for b in pl[i + 1:]):
            seen.add("unplaced_then_placed")
        if r["ready_num"] is not None and r["ready_num"] < r["min_available"]:
            seen.add("ready_within" if r["ready_after"] > 0 else "not_ready_within")
        ported = [p for p in placed if rr._ports(snap.by_task[p[0]][2])]
        for i, a in enumerate(ported):
            for b in ported[i + 1:]:
                if a[1] != b[1] and set(rr._ports(snap.by_task[a[0]][2])) & set(rr._ports(snap.by_task[b[0]][2])):
                    seen.add("port_pair_on_two_nodes")
    return seen


def check_fixture(fx, opts=None):
    """Every check of one fixture over the three prefixes: (errors, seen,
    skipped); `seen` lists the features() of the expected rows. The session is
    asked at limit 2 between the actions and at 512 after the prefix, then
    runs the actions of REST: its logs must equal those of a session that ran
    the same actions without a call."""
    errs, seen, skipped = [], set(), False
    aff = ts.has_pod_affinity(fx)
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
            snap = Snap(ssn)
            rules = ws.plugin_rules(ssn.tiers)
            if prefix is PREFIXES[0] and not aff:  # before the first action: the snapshot
                errs += compare_rows(expected_rows(snap, fx, snap.state, rules, 7), ssn.job_fit(limit=7), "at open")
            for k, name in enumerate(prefix):
                if ts.run_actions(ssn, [name]) == "ref_panic":
                    errs.append(f"{tag}: {name} ends ref_panic where the oracle ends ok")
                if k + 1 < len(prefix):
                    errs += invariants(ssn, snap, ssn.job_fit(limit=2), 2, f"{tag}, after {name}")
            rows = ssn.job_fit(limit=BIG)
            errs += invariants(ssn, snap, rows, BIG, tag)
            errs += limits_and_subsets(ssn, rows, tag)
            if aff or (ts.has_host_ports(fx) and not ws.discard_free(snap.mirror, ref)):
                skipped = True
            else:
                want = expected_rows(snap, fx, ref, rules, BIG)
                errs += compare_rows(want, rows, tag)
                seen |= features(want.values(), snap)
            with_calls = (ts.run_actions(ssn, rest), ts.log_of(ssn))
        finally:
            ssn.close()
        plain, _ = ws.open_with_reasons(fxp, opts)
        try:
            if (ts.run_actions(plain, list(prefix) + rest), ts.log_of(plain)) != with_calls:
                errs.append(f"{tag}: the logs of {list(prefix) + rest} differ with the calls in between")
        finally:
            plain.close()
    return errs, sorted(seen), skipped


def check_refusals(fx):
    """No reasons; limit 0, -1, 513; job index -1 and n_jobs; places_cap one
    short (KBG_E_CAPACITY with the need reported); a job with nothing Pending
    gives valid == 0."""
    import ctypes
    from kbgpu.fixture import run_fixture
    errs = []

    def refused(ssn, what, *args):
        try:
            ssn.job_fit(*args)
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
        L, nj = _abi.lib(), len(ssn.jobs)
        for limit in (0, -1, 513):
            refused(ssn, f"limit {limit}", None, limit)
        for bad in (-1, nj):
            refused(ssn, f"job index {bad}", [bad], 4)
        rows = ssn.job_fit()
        need = sum(r["walked"] for r in rows)
        if need < 2:
            errs.append("the fixture walks fewer than two tasks")
        out, n = (_abi.kbg_job_fit * nj)(), ctypes.c_int32(-7)
        places = (_abi.kbg_fit_place * need)()
        st = L.kbg_job_fit(ssn.handle, None, nj, BIG, out, places, need - 1, ctypes.byref(n))
        if st != _abi.KBG_E_CAPACITY or n.value != need:
            errs.append(f"places_cap one short: status {st}, n_places {n.value}, need {need}")
        if L.kbg_job_fit(ssn.handle, None, nj, BIG, out, places, need, ctypes.byref(n)) != _abi.KBG_OK:
            errs.append("places_cap exact: the call failed")
        if L.kbg_job_fit(ssn.handle, None, nj, BIG, out, None, 0, ctypes.byref(n)) != _abi.KBG_OK or \
                n.value != need or any(o.valid and o.place_off != -1 for o in out):
            errs.append("places == NULL: the rows alone, place_off -1, n_places the need")
        if L.kbg_job_fit(ssn.handle, None, nj - 1 if nj > 1 else 2, BIG, out, None, 0, None) != _abi.KBG_E_INVALID:
            errs.append("jobs == NULL with another n_jobs: the call did not return KBG_E_INVALID")
        ts.run_actions(ssn, ["allocate", "backfill"])
        after = ssn.job_fit()
        pending = {t.job for t in ssn.flat.task_objs if t is not None and t.status == PENDING}
        idle_jobs = [r for r, job in zip(after, ssn.jobs) if job.uid not in pending]
        if not idle_jobs:
            errs.append("every job has a Pending task after allocate: pick another fixture")
        for r in idle_jobs:
            if r["valid"] or r["places"] or any(v for k, v in r.items() if k not in ("valid", "places")):
                errs.append(f"a job with nothing Pending has the row {r}")
    finally:
        ssn.close()
    return errs


def check_resident(fx0, seed, rounds, opts=None, limits=(2, BIG), chain=None):
    """A resident session (kbg_session_reset, kbg_session_update) over
    helpers.churn_chain (or `chain`: [(fixture, changes)]): before the round's
    first action and after its actions, at both limits, its rows against a
    fresh session's on the round's fixture, task by uid and node by name.
    Returns (errors, rows compared)."""
    import ctypes
    errs, said = [], 0
    ssn = None
    L = _abi.lib()

    def named(s, rows):
        names, tasks = s.flat.node_names, s.flat.task_objs
        out = []
        for r in rows:
            if r["valid"]:
                d = {k: v for k, v in r.items() if k not in ("job", "places", "first_unplaced")}
                d["first_unplaced"] = tasks[r["first_unplaced"]].uid if r["first_unplaced"] >= 0 else None
                d["places"] = [(tasks[t].uid, names[n] if n >= 0 else None, k) for t, n, k in r["places"]]
                out.append((s.jobs[r["job"]].uid, sorted(d.items())))
        return sorted(out)

    try:
        rounds_ = chain if chain is not None else [(fx, ch) for fx, ch, _ in ws.resident_rounds(fx0, seed, rounds)]
        for r, (fx, changes) in enumerate(rounds_):
            actions = fx.get("actions") or ["allocate"]
            if ssn is None:
                ssn, _ = ws.open_with_reasons(fx, opts)
            else:
                _abi.check(L.kbg_session_reset(ssn.handle))
                ssn.update(changes)
            fresh, _ = ws.open_with_reasons(fx, opts)
            try:
                for when in ("before", "after"):
                    if when == "after":
                        cap = max(1, len(ssn.flat.task_objs))
                        buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
                        for name in actions:
                            _abi.check(getattr(L, ws.ENTRY[name])(ssn.handle, buf, cap, ctypes.byref(n)))
                        ts.run_actions(fresh, actions)
                    for limit in limits:
                        want, got = named(fresh, fresh.job_fit(limit=limit)), named(ssn, ssn.job_fit(limit=limit))
                        if want != got:
                            bad = [(a, b) for a, b in zip(want, got) if a != b][:1]
                            errs.append(f"round {r}, {when} the actions, limit {limit}: the resident session's rows "
                                        f"differ from a fresh session's: {bad}")
                        said += len(want)
            finally:
                fresh.close()
    finally:
        if ssn is not None:
            ssn.close()
    if not said:
        errs.append("no round held a Pending task: the case says nothing")
    return errs, said


def check_kat(fx):
    """The hand-derived walks of tests/golden/kat_job_fit.json, at open, on both paths."""
    ssn, _ = ws.open_with_reasons(fx)
    errs = []
    try:
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        jobs = {j.uid: i for i, j in enumerate(ssn.jobs)}
        kind = {jr.ALLOCATE: "allocate", jr.PIPELINE: "pipeline"}
        for exp in fx["expected"]["job_fit"]:
            for rows_of in (ssn.job_fit, lambda jobs_, limit: host_rows(ssn, jobs_, limit)):
                (g,) = rows_of([jobs[exp["job"]]], exp.get("limit", BIG))
                got = dict(g, job=exp["job"], limit=exp.get("limit", BIG), message=job_fit_message(g),
                           first_unplaced=tasks[g["first_unplaced"]].uid if g["first_unplaced"] >= 0 else None,
                           places=[[tasks[t].uid, names[n] if n >= 0 else None, kind[k] if n >= 0 else None]
                                   for t, n, k in g["places"]])
                want = dict(exp, valid=True)
                errs += [f"{exp['job']}: {k} is {got[k]}, hand-derived {want[k]}" for k in want if got[k] != want[k]]
    finally:
        ssn.close()
    return errs


# ------------------------------------------------- against the oracle's allocate
def job_alone(fx, group):
    """The fixture with every other job's Pending pods deleted, without
    `proportion` (the walk does not consult the queue), allocate alone."""
    def of(p):
        return (p.get("annotations") or {}).get("scheduling.k8s.io/group-name"), p.get("namespace")
    pods = [p for p in fx["pods"] if p["phase"] != "Pending" or of(p) == group]
    tiers = [[pl for pl in t if pl["name"] != "proportion"] for t in fx["tiers"]]
    return dict(fx, pods=pods, tiers=[t for t in tiers if t], actions=["allocate"])


def allocate_jobs(fx, most=3):
    """(group key, the oracle's output of job_alone) for the first `most`
    groups with a Pending pod with a request; None in place of the output when
    the oracle ends ref_panic."""
    out = []
    for p in fx["pods"]:
        g = ((p.get("annotations") or {}).get("scheduling.k8s.io/group-name"), p.get("namespace"))
        if p["phase"] == "Pending" and g[0] and g not in [x[0] for x in out] and len(out) < most:
            ref = run_oracle(job_alone(fx, g))
            out.append((g, ref if ref["status"] == "ok" else None))
    return out


def check_allocate(fx, picked=None):
    """(errors, the reference rows as features() reads them) of one fixture."""
    errs, shown = [], []
    ssn, _ = ws.open_with_reasons(dict(fx, actions=["allocate"]))
    try:
        snap = Snap(ssn)
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        pods = {p["uid"]: p for p in fx["pods"]}
        for group, ref in picked if picked is not None else allocate_jobs(fx):
            if ref is None:
                continue
            uid = f"{group[1]}/{group[0]}"
            if uid not in snap.job_uids:  # (pods naming a PodGroup the cache does not hold)
                continue
            j = snap.job_uids.index(uid)
            mine = {t for t, _, _ in snap.job_tasks[j]}
            dec = [(d["task"], d["node"], KINDS[d["kind"]]) for d in ref["decisions"] if pods[d["task"]]["phase"] == "Pending"]
            decided = {d[0] for d in dec}
            for rows_of in (ssn.job_fit, lambda jobs, limit: host_rows(ssn, jobs, limit)):
                (g,) = rows_of([j], BIG)
                if not g["valid"]:
                    if dec:
                        errs.append(f"{fx['name']}: job {uid}: no row, the oracle's allocate decides {dec[:3]}")
                    continue
                got = [(tasks[t].uid, names[n], k) for t, n, k in g["places"] if n >= 0]
                if got != dec:
                    bad = next((i for i, (a, b) in enumerate(zip(got, dec)) if a != b), min(len(got), len(dec)))
                    errs.append(f"{fx['name']}: job {uid}: placed entries differ from the oracle's allocate at {bad}: "
                                f"{got[bad:bad + 2]} against {dec[bad:bad + 2]}")
                nowhere = sorted(tasks[t].uid for t, n, _ in g["places"] if n < 0)
                left = sorted(tasks[t].uid for t in mine if tasks[t].uid not in decided
                              and not ts.empty(snap.by_task[t][1]))
                if g["pending"] <= BIG and nowhere != left:
                    errs.append(f"{fx['name']}: job {uid}: entries with node -1 {nowhere}, the oracle leaves {left}")
            order = {d[0]: i for i, d in enumerate(dec)}
            index = {n: i for i, n in enumerate(names)}
            walked = [(t, uid_) for t, uid_, _ in walk_order(snap.job_tasks[j], ws.plugin_rules(ssn.tiers)["task_prio"])
                      if not ts.empty(snap.by_task[t][1])]
            places = [(t, index[dec[order[u]][1]], dec[order[u]][2]) if u in order else (t, -1, 0) for t, u in walked]
            rn = next((x["ready_num"] for x in ref["jobs"] if x["uid"] == uid), 0) - len(dec)
            shown.append(dict(places=places, min_available=snap.job_min[j], ready_num=rn,
                              **jr.rows_of(places, rn, snap.job_min[j])))
        return errs, shown, snap
    finally:
        ssn.close()


def gang_fixture(ports=True):
    """A hand-built cluster (ports=False: without job H, so that the device kernel answers). Nodes c00 4000m (x000 1500m Running, x001 1500m
    being deleted: Idle 1000m, Releasing 1500m), c01 2000m, c02 1000m, all empty
    of other pods. Job G (MinMember 4), in UID order:
      g0-big 3000m     fits nowhere                         -> nowhere
      g1-driver 2000m  c00 Idle 1000m no, Releasing no; c01 -> c01 Allocate
      g2-w 1000m       c00 Idle 1000m                       -> c00 Allocate
      g3-w 1000m       c00 Idle 0, Releasing 1500m          -> c00 Pipeline
      g4-w 1000m       c00 500m left, c01 0; c02            -> c02 Allocate (the fourth: ready after step 5)
      g5-w 1000m       nothing left                         -> nowhere
    Job N (MinMember 5) holds two pods of 3000m: none fits, never ready. Job H
    (MinMember 2) holds two pods of 100m with host port 8080: the first goes to
    c00, the second finds the port taken there in the job's own view -> c01."""
    def pod(uid, group, cpu, mem, node_name="", ports=None, **kw):
        c = {"requests": {"cpu": f"{cpu}m", "memory": f"{mem}Mi"}}
        if ports:
            c["ports"] = ports
        return dict({"uid": uid, "namespace": "ns", "name": uid, "phase": "Running" if node_name else "Pending",
                     "nodeName": node_name, "annotations": {"scheduling.k8s.io/group-name": group},
                     "containers": [c]}, **kw)
    nodes = [{"name": f"c{i:02d}", "allocatable": {"cpu": f"{c}m", "memory": "8192Mi", "pods": "110"}, "labels": {}}
             for i, c in enumerate((4000, 2000, 1000))]
    pods = [pod("x000", "X", 1500, 1024, "c00"),
            pod("x001", "X", 1500, 1024, "c00", deletionTimestamp="2026-01-01T00:00:00Z"),
            pod("g0-big", "G", 3000, 512), pod("g1-driver", "G", 2000, 1024)] + \
           [pod(f"g{i}-w", "G", 1000, 512) for i in (2, 3, 4, 5)] + \
           [pod("n0", "N", 3000, 512), pod("n1", "N", 3000, 512)] + \
           [pod(f"h{i}", "H", 100, 64, ports=[{"hostPort": 8080, "protocol": "TCP"}]) for i in (0, 1) if ports]
    groups = [{"namespace": "ns", "name": g, "minMember": m, "queue": "q", "creationTimestamp": t * 10 ** 9}
              for g, m, t in (("G", 4, 100), ("N", 5, 200), ("H", 2, 300), ("X", 1, 1)) if ports or g != "H"]
    tiers = [[{"name": "priority"}, {"name": "gang"}], [{"name": "drf"}, {"name": "predicates"}, {"name": "proportion"}]]
    return {"name": "gang-hand" if ports else "gang-dev", "actions": ["allocate"], "tiers": tiers, "nodes": nodes,
            "queues": [{"name": "q", "weight": 1}], "podGroups": groups, "pods": pods}


GANG_CLAIMS = {"ns/G": [("g0-big", None, 0), ("g1-driver", "c01", jr.ALLOCATE), ("g2-w", "c00", jr.ALLOCATE),
                        ("g3-w", "c00", jr.PIPELINE), ("g4-w", "c02", jr.ALLOCATE), ("g5-w", None, 0)],
               "ns/N": [("n0", None, 0), ("n1", None, 0)],
               "ns/H": [("h0", "c00", jr.ALLOCATE), ("h1", "c01", jr.ALLOCATE)]}

# seeds of synth.random_fixture at open (picked on the CPU with the oracle and the hostsim run, see
# tests/test_hostsim_job_fit.py: those the oracle ends in ref_panic, and those with pod affinity, are left out)
ALLOCATE_SEEDS = tuple(range(1, 13))


def allocate_fixtures():
    from kbgpu import synth
    out = {"hand": gang_fixture(), "dev": gang_fixture(ports=False)}
    out.update({f"seed{s}": synth.random_fixture(s) for s in ALLOCATE_SEEDS})
    return out


def allocate_picks(fx):
    """None when the fixture is left out (pod affinity, or the oracle ends
    some job's allocate in ref_panic), else allocate_jobs(fx)."""
    if ts.has_pod_affinity(fx):
        return None
    picks = allocate_jobs(fx)
    return None if any(ref is None for _, ref in picks) else picks


def check_structural(case=None):
    """One structural batch of tests/query_update_cases.py on a session that
    ran its actions and was asked (every buffer sized for the old session),
    then reset and updated: held to a fresh session on the fixture after the
    events, at limits 2 and 512, before and after the actions."""
    import query_update_cases as qc
    from update_events import fixture_after
    fx0, rounds_of, _ = (case or qc.pod_group_add_new_class)()
    fx0 = dict(fx0, actions=list(fx0.get("actions") or qc.ACTIONS))
    changes = rounds_of[0](None, fx0)
    fx1 = fixture_after(fx0, [changes])
    assert fx1 is not None, "no fixture says the cache after the batch"
    return check_resident(None, 0, 0, chain=[(fx0, []), (dict(fx1, actions=fx0["actions"]), changes)])
