"""Session-level checks of kbg_node_drain, shared by the hostsim tests
(tests/test_hostsim_drain.py, through tests/drain_worker.py) and the device
tests (tests/test_drain_gpu.py).

`check_fixture` opens a session with reasons and, for each action prefix of
tests/task_why_session.py, runs the prefix and asks for the rows of every
node. The expected places are built as tests/job_fit_session.py builds its
rows, without the library: node Idle, Releasing and pod counts from the
ORACLE's output of the same prefix, the pods a node holds and their order
(NodeInfo.Tasks) from the mirror at open plus the oracle's decisions, the moved
tasks those of them in an AllocatedStatus at open that the oracle's prefix did
not evict and then the oracle's Allocate decisions onto the node in the order
of its log (its Pipeline decisions join the other pods), the stages from reasons_ref.first_failing_stage against the row's
own view (its placements' pods join the node's), the walk in plain Python with
the drained node and the cordon left out and backfill's rule for a pod with an
empty request.

reasons_ref has no inter-pod affinity stage: sessions with pod affinity are
held to the invariants (affinity_now among them), to kbg_task_reasons through
Pending twins (`check_twin`) and to the oracle's own allocate of one Pending
twin at a time (`check_twin_oracle`: the verdict of now, the moved pod still
counted where it is); tests/golden/kat_drain.json holds a hand-derived walk
under pod affinity. Seeds whose cycle discards a statement after evicting get
no expected rows on sessions with host ports (tests/task_why_session.py: the
same rule).

Against itself and the other calls on the same session, whatever it holds:
  placed_idle + placed_releasing + unplaced == walked == min(tasks, limit),
  every derived field follows from the places (drain_ref.row_of);
  no place is the drained node or a cordoned one;
  the places at limit L are the first L at limit 512; nodes asked by index,
  out of order and twice, equal their rows of the whole call;
  KBG_HOST_NODE_DRAIN=1 gives the same rows.
`check_twin` holds a walk of one requesting task to kbg_task_reasons through a
Pending twin of the moved pod, and `check_headroom` a walk of k copies with one
target node to kbg_task_headroom's per-node bound."""
import os

import drain_ref as dr
import reasons_ref as rr
import task_why_ref as tr
import task_why_session as ts
import victim_why_session as ws
from helpers import run_oracle
from kbgpu import _abi
from kbgpu import api
from kbgpu.fixture import drain_message

PREFIXES, REST = ts.PREFIXES, ts.REST
BIG = _abi.FIT_MAX_LIMIT
MOVABLE = (api.ALLOCATED, api.BINDING, api.BOUND, api.RUNNING)  # AllocatedStatus, api/helpers.go:63-70
DERIVED = ("walked", "placed_idle", "placed_releasing", "unplaced", "first_unplaced", "nodes_used", "jobs_moved")


class Snap(ts.OpenSnap):
    """OpenSnap, and per node the pods it holds at open in NodeInfo.Tasks
    order as (task index or None for a pod outside the session jobs, uid,
    status, request, pod)."""

    def __init__(self, ssn):
        super().__init__(ssn)
        m = self.mirror
        self.job_min = m.job_min
        self.task_job = {m.task_index[u]: j for u, j in m.task_job.items() if u in m.task_index}
        self.order = [[(m.task_index.get(t.uid) if t.uid in m.task_job else None, t.uid, t.status,
                        [float(v) for v in t.resreq.as_tuple()], t.pod) for t in n.tasks.values()] for n in ssn.nodes]


def expected_rows(snap, fx, ref, rules, limit, cordon=()):
    """{node index: row} of every node after the oracle's prefix (ref: its
    output; snap.state: no action yet: jobs_short is None there, not compared)."""
    pods = {p["uid"]: p for p in fx["pods"]}
    by_name = {n["name"]: n for n in ref["nodes"]}
    held0 = [dict(h) for h in snap.held]
    index = {name: i for i, (name, _, _) in enumerate(snap.nodes)}
    for d in ref["decisions"]:
        held0[index[d["node"]]].setdefault(rr.pod_key(pods[d["task"]]), pods[d["task"]])
    evicted = {e["task"] for e in ref.get("evictions") or []}
    ready = {j["uid"]: j["ready_num"] for j in ref.get("jobs") or []}
    ready_num = {j: ready.get(u, 0) for j, u in enumerate(snap.mirror.job_uids)} if ref.get("jobs") else None
    panic = sum(1 for _, node, _ in snap.nodes if node is None) if rules["predicates"] else 0
    out = {}
    pend = {uid: (t, uid, api.ALLOCATED, req, pod) for t, uid, req, pod, _ in snap.pending}
    placed, piped = [[] for _ in snap.nodes], [0] * len(snap.nodes)
    done = set()
    for d in ref["decisions"]:  # (a decision whose PodKey the node held left the node as it was)
        i, key = index[d["node"]], rr.pod_key(pods[d["task"]])
        if d["task"] in pend and d["task"] not in done and key not in snap.held[i] and \
                key not in {rr.pod_key(e[4]) for e in placed[i]}:
            done.add(d["task"])
            if d["kind"] == "allocate":
                placed[i].append(pend[d["task"]])
            else:
                piped[i] += 1
    for x, tasks in enumerate(snap.order):
        move = [e for e in tasks if e[0] is not None and e[2] in MOVABLE and e[1] not in evicted] + placed[x]
        gone = set(cordon) | {x}
        view = {}  # node index -> [idle, releasing, ntasks, held]
        places = []
        for t, uid, _, req, pod in move[:limit]:
            beff = ts.empty(req)
            at, kind = -1, dr.ALLOCATE
            for i, (name, node, max_task_num) in enumerate(snap.nodes):
                if i in gone:
                    continue
                st = view.get(i)
                if st is None:
                    o = by_name[name]
                    st = [[float(v) for v in o["idle"]], [float(v) for v in o["releasing"]], o["ntasks"], held0[i]]
                if rules["predicates"]:
                    if node is None or max_task_num <= st[2]:
                        continue
                    if rr.first_failing_stage(pod, node, 1 << 30, st[3]) >= 0:
                        continue
                if beff or dr.less_equal(req, st[0]):  # backfill.go:47-64: no resource test
                    at, kind = i, dr.ALLOCATE
                elif dr.less_equal(req, st[1]):
                    at, kind = i, dr.PIPELINE
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
        row = dict(node=x, tasks=len(move), other_pods=len(tasks) - len(move) + len(placed[x]) + piped[x],
                   places=places, panic_nodes=panic)
        row.update(dr.row_of(places, snap.task_job, ready_num or {j: 0 for j in range(len(snap.job_min))},
                             dict(enumerate(snap.job_min))))
        if ready_num is None:
            row["jobs_short"] = None
        out[x] = row
    return out


def compare_rows(want, got, tag):
    errs = []
    valid = sorted(r["node"] for r in got if r["valid"])
    if sorted(want) != valid:
        return [f"{tag}: rows of nodes {valid}, reference {sorted(want)}"]
    for g in got:
        w = want[g["node"]]
        keys = ["tasks", "other_pods", "places", "panic_nodes"] + list(DERIVED)
        if w["jobs_short"] is not None:
            keys.append("jobs_short")
        errs += [f"{tag}: node {g['node']}: {k} is {g[k]}, reference {w[k]}" for k in keys if g[k] != w[k]]
    return errs


def host_rows(ssn, nodes=None, cordon=(), limit=BIG):
    os.environ["KBG_HOST_NODE_DRAIN"] = "1"
    try:
        return ssn.node_drain(nodes, cordon, limit)
    finally:
        del os.environ["KBG_HOST_NODE_DRAIN"]


def invariants(ssn, snap, rows, limit, cordon, tag):
    """The rows against themselves and the host path."""
    errs = []
    for r in rows:
        if not r["valid"]:
            errs.append(f"{tag}: node {r['node']}: not valid")
            continue
        x = r["node"]
        if r["placed_idle"] + r["placed_releasing"] + r["unplaced"] != r["walked"] or \
                r["walked"] != min(r["tasks"], limit) or len(r["places"]) != r["walked"]:
            errs.append(f"{tag}: node {x}: {r['placed_idle']} + {r['placed_releasing']} + {r['unplaced']} of "
                        f"{r['walked']} walked, {r['tasks']} tasks at limit {limit}")
        bad = [p for p in r["places"] if p[1] == x or p[1] in cordon]
        if bad:
            errs.append(f"{tag}: node {x}: places {bad} on the drained node or the cordon {sorted(cordon)}")
        if any(t not in snap.task_job for t, _, _ in r["places"]):
            errs.append(f"{tag}: node {x}: a walked task outside the session jobs")
            continue
        # jobs_short needs the gangs' numbers: drain_ref.row_of against the session's own job_fit-free fields
        derived = dr.row_of(r["places"], snap.task_job, {j: 0 for j in set(snap.task_job.values())},
                            {j: 1 for j in set(snap.task_job.values())})
        errs += [f"{tag}: node {x}: {k} is {r[k]}, its places give {derived[k]}" for k in DERIVED if r[k] != derived[k]]
        if r["jobs_short"] > r["jobs_moved"] or (r["unplaced"] == 0 and r["jobs_short"]):
            errs.append(f"{tag}: node {x}: jobs_short {r['jobs_short']} of {r['jobs_moved']} moved, {r['unplaced']} unplaced")
        msg = drain_message(r)
        placed = r["placed_idle"] + r["placed_releasing"]
        if r["tasks"] and (not msg.startswith(f"{placed} of {r['walked']} pods find room ({r['placed_releasing']} on "
                                              f"releasing resources, {r['nodes_used']} nodes)") or
                           ("do not, first task" in msg) != (r["unplaced"] > 0) or
                           ("breaks" in msg) != (r["jobs_short"] > 0) or
                           ("not walked" in msg) != (r["tasks"] > r["walked"])):
            errs.append(f"{tag}: node {x}: message {msg!r}")
        if not r["tasks"] and not msg.startswith("no pods to move"):
            errs.append(f"{tag}: node {x}: message {msg!r}")
    host = host_rows(ssn, None, cordon, limit)
    if host != rows:
        bad = [(a, b) for a, b in zip(rows, host) if a != b][:2]
        errs.append(f"{tag}: the device-shaped path differs from KBG_HOST_NODE_DRAIN=1: {bad}")
    return errs


def limits_and_subsets(ssn, rows, cordon, tag):
    errs = []
    for limit in (1, 2):
        short = ssn.node_drain(None, cordon, limit)
        for a, b in zip(rows, short):
            if a["valid"] != b["valid"] or b["places"] != a["places"][:limit] or a["tasks"] != b["tasks"] or \
                    a["other_pods"] != b["other_pods"]:
                errs.append(f"{tag}: node {a['node']}: the places at limit {limit} are {b['places']}, at 512 "
                            f"{a['places'][:3]}")
    if rows:
        pick = [len(rows) - 1, 0, len(rows) // 2, len(rows) - 1]  # out of order, one twice
        if ssn.node_drain(pick, cordon, BIG) != [rows[p] for p in pick]:
            errs.append(f"{tag}: nodes {pick} asked by index differ from their rows of the whole call")
    return errs


def features(rows, snap, plain=None):
    """What a set of expected rows shows (the ..._say_something tests);
    `plain`: the rows of the same nodes without the cordon."""
    seen = set()
    req = {e[0]: e[3] for tasks in snap.order for e in tasks if e[0] is not None}
    req.update({t: r for t, _, r, _, _ in snap.pending})  # (what the prefix allocated is moved too)
    pod_of = {e[0]: e[4] for tasks in snap.order for e in tasks if e[0] is not None}
    pod_of.update({t: pod for t, _, _, pod, _ in snap.pending})
    for r in rows:
        pl = r["places"]
        placed = [p for p in pl if p[1] >= 0]
        if len({tuple(req[t]) for t, _, _ in pl}) > 1:
            seen.add("two_shapes")
        if len({p[1] for p in placed}) < len(placed):
            seen.add("two_on_one_node")
        if any(p[2] == dr.PIPELINE for p in placed):
            seen.add("pipeline")
        if any(a[1] < 0 <= b[1] for i, a in enumerate(pl) for b in pl[i + 1:]):
            seen.add("unplaced_then_placed")
        if any(ts.empty(req[t]) for t, _, _ in placed):
            seen.add("best_effort")
        if r["jobs_short"] is not None and pl:
            seen.add("jobs_short" if r["jobs_short"] > 0 else "jobs_not_short")
        if plain is not None and plain[r["node"]]["places"] != pl:
            seen.add("cordon_changed_a_place")
        ported = [p for p in placed if rr._ports(pod_of[p[0]])]
        for i, u in enumerate(ported):
            for w in ported[i + 1:]:
                if u[1] != w[1] and set(rr._ports(pod_of[u[0]])) & set(rr._ports(pod_of[w[0]])):
                    seen.add("port_pair_on_two_nodes")
    return seen


def pick_cordon(want):
    """The nodes most rows of `want` place on: cordoning them changes places."""
    count = {}
    for r in want.values():
        for _, n, _ in r["places"]:
            if n >= 0:
                count[n] = count.get(n, 0) + 1
    return tuple(sorted(sorted(count, key=lambda n: (-count[n], n))[:2]))


def check_fixture(fx, opts=None):
    """Every check of one fixture over the three prefixes: (errors, seen,
    skipped); `seen` lists the features() of the expected rows. The session is
    asked at limit 2 between the actions and at 512 after the prefix, without
    and with a cordon, then runs the actions of REST: its logs must equal those
    of a session that ran the same actions without a call."""
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
                errs += compare_rows(expected_rows(snap, fx, snap.state, rules, 7), ssn.node_drain(limit=7), "at open")
            for k, name in enumerate(prefix):
                if ts.run_actions(ssn, [name]) == "ref_panic":
                    errs.append(f"{tag}: {name} ends ref_panic where the oracle ends ok")
                if k + 1 < len(prefix):
                    errs += invariants(ssn, snap, ssn.node_drain(limit=2), 2, (), f"{tag}, after {name}")
            rows = ssn.node_drain(limit=BIG)
            want_aff = bool(aff and rules["predicates"])
            if any(r["affinity_now"] != want_aff for r in rows):
                errs.append(f"{tag}: affinity_now is not {want_aff} in every row")
            errs += invariants(ssn, snap, rows, BIG, (), tag)
            errs += limits_and_subsets(ssn, rows, (), tag)
            if aff or (ts.has_host_ports(fx) and not ws.discard_free(snap.mirror, ref)):
                skipped = True
                cordon = pick_cordon({r["node"]: r for r in rows})
            else:
                want = expected_rows(snap, fx, ref, rules, BIG)
                errs += compare_rows(want, rows, tag)
                cordon = pick_cordon(want)
                fenced = expected_rows(snap, fx, ref, rules, BIG, cordon)
                errs += compare_rows(fenced, ssn.node_drain(None, cordon + cordon[:1], BIG), f"{tag}, cordon {cordon}")
                seen |= features(want.values(), snap) | features(fenced.values(), snap, want)
            fenced_rows = ssn.node_drain(None, cordon, BIG)
            errs += invariants(ssn, snap, fenced_rows, BIG, cordon, f"{tag}, cordon {cordon}")
            errs += limits_and_subsets(ssn, fenced_rows, cordon, f"{tag}, cordon {cordon}")
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
    """No reasons; limit 0, -1, 513; node index -1 and n_nodes; cordon index
    -1 and n_nodes; places_cap one short (KBG_E_CAPACITY with the need
    reported); places == NULL; nodes == NULL with another count."""
    import ctypes
    from kbgpu.fixture import run_fixture
    errs = []

    def refused(ssn, what, *args):
        try:
            ssn.node_drain(*args)
            errs.append(f"{what}: the call did not fail")
        except _abi.KbgError as e:
            if e.status != "invalid":
                errs.append(f"{what}: {e}")

    _, ssn = run_fixture(dict(fx, actions=["allocate"]), {})
    try:
        refused(ssn, "reasons = 0", [0], (), 4)
    finally:
        ssn.close()
    ssn, _ = ws.open_with_reasons(fx)
    try:
        L, nn = _abi.lib(), len(ssn.flat.node_names)
        for limit in (0, -1, 513):
            refused(ssn, f"limit {limit}", None, (), limit)
        for bad in (-1, nn):
            refused(ssn, f"node index {bad}", [bad], (), 4)
            refused(ssn, f"cordon index {bad}", [0], (bad,), 4)
        rows = ssn.node_drain()
        need = sum(r["walked"] for r in rows)
        if need < 2:
            errs.append("the fixture walks fewer than two tasks")
        out, n = (_abi.kbg_node_drain * nn)(), ctypes.c_int32(-7)
        places = (_abi.kbg_fit_place * need)()
        st = L.kbg_node_drain(ssn.handle, None, nn, None, 0, BIG, out, places, need - 1, ctypes.byref(n))
        if st != _abi.KBG_E_CAPACITY or n.value != need:
            errs.append(f"places_cap one short: status {st}, n_places {n.value}, need {need}")
        if L.kbg_node_drain(ssn.handle, None, nn, None, 0, BIG, out, places, need, ctypes.byref(n)) != _abi.KBG_OK:
            errs.append("places_cap exact: the call failed")
        if L.kbg_node_drain(ssn.handle, None, nn, None, 0, BIG, out, None, 0, ctypes.byref(n)) != _abi.KBG_OK or \
                n.value != need or any(o.valid and o.place_off != -1 for o in out):
            errs.append("places == NULL: the rows alone, place_off -1, n_places the need")
        if L.kbg_node_drain(ssn.handle, None, nn + 1, None, 0, BIG, out, None, 0, None) != _abi.KBG_E_INVALID:
            errs.append("nodes == NULL with another n_nodes: the call did not return KBG_E_INVALID")
        if L.kbg_node_drain(ssn.handle, None, nn, None, 1, BIG, out, None, 0, None) != _abi.KBG_E_INVALID:
            errs.append("cordon == NULL with a count: the call did not return KBG_E_INVALID")
        if L.kbg_node_drain(ssn.handle, None, nn, None, 0, BIG, out, None, 3, None) != _abi.KBG_E_INVALID:
            errs.append("places == NULL with a capacity: the call did not return KBG_E_INVALID")
    finally:
        ssn.close()
    return errs


def check_resident(fx0, seed, rounds, opts=None, limits=(2, BIG), chain=None):
    """A resident session (kbg_session_reset, kbg_session_update) over
    helpers.churn_chain (or `chain`: [(fixture, changes)]): before the round's
    first action and after its actions, at both limits, with node 0 cordoned,
    its rows against a fresh session's on the round's fixture, task by uid and
    node by name. Returns (errors, rows compared)."""
    import ctypes
    errs, said = [], 0
    ssn = None
    L = _abi.lib()

    def named(s, rows):
        names, tasks = s.flat.node_names, s.flat.task_objs
        out = []
        for r in rows:
            if r["valid"]:
                d = {k: v for k, v in r.items() if k not in ("node", "places", "first_unplaced")}
                d["first_unplaced"] = tasks[r["first_unplaced"]].uid if r["first_unplaced"] >= 0 else None
                d["places"] = [(tasks[t].uid, names[n] if n >= 0 else None, k) for t, n, k in r["places"]]
                out.append((names[r["node"]], sorted(d.items())))
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
                        def cordon(s):
                            return (s.flat.node_names.index(fresh.flat.node_names[0]),)
                        want = named(fresh, fresh.node_drain(None, cordon(fresh), limit))
                        got = named(ssn, ssn.node_drain(None, cordon(ssn), limit))
                        if want != got:
                            bad = [(a, b) for a, b in zip(want, got) if a != b][:1]
                            errs.append(f"round {r}, {when} the actions, limit {limit}: the resident session's rows "
                                        f"differ from a fresh session's: {bad}")
                        said += sum(1 for _, d in want if dict(d)["walked"])
            finally:
                fresh.close()
    finally:
        if ssn is not None:
            ssn.close()
    if not said:
        errs.append("no round moved a task: the case says nothing")
    return errs, said


def check_structural(case=None):
    """One structural batch of tests/query_update_cases.py (job_fit_session.check_structural's)."""
    import query_update_cases as qc
    from update_events import fixture_after
    fx0, rounds_of, _ = (case or qc.pod_group_add_new_class)()
    fx0 = dict(fx0, actions=list(fx0.get("actions") or qc.ACTIONS))
    changes = rounds_of[0](None, fx0)
    fx1 = fixture_after(fx0, [changes])
    assert fx1 is not None, "no fixture says the cache after the batch"
    return check_resident(None, 0, 0, chain=[(fx0, []), (dict(fx1, actions=fx0["actions"]), changes)])


# ------------------------------------------------------------ hand-built
def drain_fixture(ports=True):
    """A hand-built cluster (ports=False: without job P, so that the device
    kernel answers). Nodes d00..d03 of 4000m / 8192Mi / 110 pods, every pod
    with 64Mi:
      d00: a0 1000m, a1 1000m (job A, MinMember 2), e0 without a request (job E), and with ports p0, p1 of 100m
           with host port 8080 (job P, MinMember 1)               -> Idle 1800m (2000m without job P)
      d01: x0 3500m                                               -> Idle 500m
      d02: y0 1800m, y1 1500m being deleted                       -> Idle 700m, Releasing 1500m
      d03: z0 3000m (job Z, MinMember 1)                          -> Idle 1000m
    Draining d00, in NodeInfo.Tasks order a0, a1, e0, p0, p1:
      a0 1000m   d01 500m no; d02 Idle 700m no, Releasing 1500m       -> d02 Pipeline
      a1 1000m   d01 no; d02 Idle 700m, Releasing 500m no; d03 1000m  -> d03 Allocate
      e0 empty   no resource test: the first node past the stages    -> d01 Allocate
      p0 100m    d01 Idle 500m                                        -> d01 Allocate
      p1 100m    d01 holds port 8080 in the row's view; d02 Idle 700m -> d02 Allocate
    Draining d02: y1 is Releasing and stays out (other_pods 1); y0 1800m finds d00's Idle. Draining d03: z0 3000m
    fits nowhere, and job Z (ready 1, MinMember 1) loses its minimum: jobs_short 1. With d02 cordoned, draining
    d00: a0 takes d03's 1000m, a1 finds nothing: job A (ready 2, MinMember 2) breaks; e0 and p0 go to d01 as
    before, p1 finds port 8080 taken on d01, d02 cordoned and d03 empty: nowhere, and job P (ready 2, MinMember 1)
    keeps its minimum: jobs_short 1."""
    def pod(uid, group, cpu, node_name, ports=None, **kw):
        c = {"requests": {"cpu": f"{cpu}m", "memory": "64Mi"}} if cpu else {}
        if ports:
            c["ports"] = ports
        return dict({"uid": uid, "namespace": "ns", "name": uid, "phase": "Running", "nodeName": node_name,
                     "annotations": {"scheduling.k8s.io/group-name": group}, "containers": [c]}, **kw)
    nodes = [{"name": f"d{i:02d}", "allocatable": {"cpu": "4000m", "memory": "8192Mi", "pods": "110"}, "labels": {}}
             for i in range(4)]
    pods = [pod("a0", "A", 1000, "d00"), pod("a1", "A", 1000, "d00"), pod("e0", "E", 0, "d00")] + \
           [pod(f"p{i}", "P", 100, "d00", ports=[{"hostPort": 8080, "protocol": "TCP"}]) for i in (0, 1) if ports] + \
           [pod("x0", "X", 3500, "d01"), pod("y0", "Y", 1800, "d02"),
            pod("y1", "Y", 1500, "d02", deletionTimestamp="2026-01-01T00:00:00Z"), pod("z0", "Z", 3000, "d03")]
    groups = [{"namespace": "ns", "name": g, "minMember": m, "queue": "q", "creationTimestamp": t * 10 ** 9}
              for t, (g, m) in enumerate((("A", 2), ("E", 1), ("P", 1), ("X", 1), ("Y", 1), ("Z", 1)), 1)
              if ports or g != "P"]
    tiers = [[{"name": "priority"}, {"name": "gang"}], [{"name": "drf"}, {"name": "predicates"}, {"name": "proportion"}]]
    return {"name": "drain-hand" if ports else "drain-dev", "actions": ["allocate"], "tiers": tiers, "nodes": nodes,
            "queues": [{"name": "q", "weight": 1}], "podGroups": groups, "pods": pods}


A_, P_ = dr.ALLOCATE, dr.PIPELINE
# (cordon, node) -> (places, fields)
DRAIN_CLAIMS = {
    ((), "d00"): ([("a0", "d02", P_), ("a1", "d03", A_), ("e0", "d01", A_), ("p0", "d01", A_), ("p1", "d02", A_)],
                  dict(tasks=5, other_pods=0, jobs_moved=3, jobs_short=0, unplaced=0)),
    ((), "d02"): ([("y0", "d00", A_)], dict(tasks=1, other_pods=1, jobs_moved=1, jobs_short=0, unplaced=0)),
    ((), "d03"): ([("z0", None, 0)], dict(tasks=1, other_pods=0, jobs_moved=1, jobs_short=1, unplaced=1)),
    (("d02",), "d00"): ([("a0", "d03", A_), ("a1", None, 0), ("e0", "d01", A_), ("p0", "d01", A_), ("p1", None, 0)],
                        dict(tasks=5, other_pods=0, jobs_moved=3, jobs_short=1, unplaced=2)),
}


def check_hand(ports=True):
    """The hand-worked walks of drain_fixture, at open, on both paths."""
    ssn, _ = ws.open_with_reasons(drain_fixture(ports))
    errs = []
    try:
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        for (cordon, node), (places, fields) in DRAIN_CLAIMS.items():
            if not ports:
                places = [p for p in places if not p[0].startswith("p")]
                fields = dict(fields, tasks=len(places), jobs_moved=fields["jobs_moved"] - (node == "d00"),
                              unplaced=sum(1 for p in places if p[1] is None))
            for rows_of in (ssn.node_drain, lambda n, c, lim: host_rows(ssn, n, c, lim)):
                (g,) = rows_of([names.index(node)], [names.index(c) for c in cordon], BIG)
                got = [(tasks[t].uid, names[n] if n >= 0 else None, k) for t, n, k in g["places"]]
                if got != places:
                    errs.append(f"drain {node}, cordon {cordon}: walk {got}, hand-worked {places}")
                errs += [f"drain {node}, cordon {cordon}: {k} is {g[k]}, hand-worked {v}" for k, v in fields.items()
                         if g[k] != v]
    finally:
        ssn.close()
    return errs


def check_twin(fx, opts=None):
    """A walk of one requesting task lands on the lowest non-excluded node that
    kbg_task_reasons puts under FITS_IDLE or FITS_RELEASING for a Pending twin
    of the moved pod (the same spec under another name and uid, in a PodGroup
    of its own): (errors, walks compared)."""
    import copy
    errs, said = [], 0
    fx = dict(fx, actions=["allocate"])
    ssn, _ = ws.open_with_reasons(fx, opts)
    try:
        snap = Snap(ssn)
        firsts = {}
        for x, tasks in enumerate(snap.order):
            e = next((e for e in tasks if e[0] is not None and e[2] in MOVABLE), None)
            if e is not None and not ts.empty(e[3]):
                firsts[x] = e
        rows = {r["node"]: r for r in ssn.node_drain(sorted(firsts), (), 1)}
    finally:
        ssn.close()
    twins, pods = {}, list(fx["pods"])
    groups = list(fx["podGroups"])
    for x, e in firsts.items():
        p = copy.deepcopy(e[4])
        p.update(uid=f"twin-{e[1]}", name=f"twin-{e[1]}", phase="Pending", nodeName="")
        p.pop("deletionTimestamp", None)
        p.setdefault("annotations", {})["scheduling.k8s.io/group-name"] = f"twin-{x}"
        src = next((g for g in groups if g["name"] == (e[4].get("annotations") or {}).get(
            "scheduling.k8s.io/group-name") and g.get("namespace") == p.get("namespace")), None)
        groups.append(dict(src or {"queue": fx["queues"][0]["name"]}, namespace=p.get("namespace"), name=f"twin-{x}",
                           minMember=1, creationTimestamp=10 ** 15 + x))
        pods.append(p)
        twins[x] = p["uid"]
    ssn, _ = ws.open_with_reasons(dict(fx, pods=pods, podGroups=groups), opts)
    try:
        index = {t.uid: i for i, t in enumerate(ssn.flat.task_objs) if t is not None}
        for x, uid in twins.items():
            (w,) = ssn.task_reasons([index[uid]])
            # the drained node is the only exclusion: the lowest node of the two causes that is not it, found by
            # asking again for the nodes after it is what first_node cannot say; so only rows where it decides
            f = w["first_node"]
            cands = sorted(c for c in ((f[tr.FITS_IDLE], dr.ALLOCATE), (f[tr.FITS_RELEASING], dr.PIPELINE)) if c[0] >= 0)
            if cands and cands[0][0] == x:
                continue  # (the twin's first fit is the drained node itself: the row below it is not in first_node)
            want = cands[0] if cands else (-1, 0)
            t, n, k = rows[x]["places"][0]
            if (n, k) != want:
                errs.append(f"drain {x}: its first task goes to {(n, k)}, kbg_task_reasons of its twin gives {want}")
            said += 1
    finally:
        ssn.close()
    return errs, said


def headroom_fixture():
    """One target node. h00 holds c0..c5 of 600m (Idle 400m: no copy fits
    there); h01 holds w0 1500m and w1 1000m being deleted (Idle 1500m,
    Releasing 1000m): two copies from Idle, one from Releasing, three nowhere.
    c-twin is a Pending copy of the moved pods in a PodGroup of its own."""
    def pod(uid, group, cpu, node_name, **kw):
        return dict({"uid": uid, "namespace": "ns", "name": uid, "phase": "Running" if node_name else "Pending",
                     "nodeName": node_name, "annotations": {"scheduling.k8s.io/group-name": group},
                     "containers": [{"requests": {"cpu": f"{cpu}m", "memory": "64Mi"}}]}, **kw)
    nodes = [{"name": f"h{i:02d}", "allocatable": {"cpu": "4000m", "memory": "8192Mi", "pods": "110"}, "labels": {}}
             for i in range(2)]
    pods = [pod(f"c{i}", "C", 600, "h00") for i in range(6)] + \
           [pod("w0", "W", 1500, "h01"), pod("w1", "W", 1000, "h01", deletionTimestamp="2026-01-01T00:00:00Z"),
            pod("c-twin", "T", 600, "")]
    groups = [{"namespace": "ns", "name": g, "minMember": 1, "queue": "q", "creationTimestamp": t * 10 ** 9}
              for t, g in enumerate("CWT", 1)]
    tiers = [[{"name": "priority"}, {"name": "gang"}], [{"name": "drf"}, {"name": "predicates"}, {"name": "proportion"}]]
    return {"name": "drain-headroom", "actions": ["allocate"], "tiers": tiers, "nodes": nodes,
            "queues": [{"name": "q", "weight": 1}], "podGroups": groups, "pods": pods}


def check_headroom():
    """A walk of k identical tasks with one target node against
    kbg_task_headroom's per-node bound for a Pending copy, on both paths."""
    ssn, _ = ws.open_with_reasons(headroom_fixture())
    errs = []
    try:
        names = ssn.flat.node_names
        twin = next(i for i, t in enumerate(ssn.flat.task_objs) if t is not None and t.uid == "c-twin")
        (room,) = ssn.task_headroom([twin], 1024)
        if (room["copies_idle"], room["copies_releasing"], room["nodes_idle"], room["limit_hit"]) != (2, 1, 1, 0):
            errs.append(f"kbg_task_headroom of the copy: {room}, hand-worked 2 + 1 on one node")
        for rows_of in (ssn.node_drain, lambda n, c, lim: host_rows(ssn, n, c, lim)):
            (g,) = rows_of([names.index("h00")], (), BIG)
            got = (g["tasks"], g["placed_idle"], g["placed_releasing"], g["unplaced"], g["nodes_used"])
            want = (6, room["copies_idle"], room["copies_releasing"], 6 - room["copies_idle"] - room["copies_releasing"],
                    1)
            if got != want or {n for _, n, _ in g["places"] if n >= 0} != {room["first_node"]}:
                errs.append(f"drain h00: (tasks, idle, releasing, unplaced, nodes) {got}, kbg_task_headroom gives {want} "
                            f"on node {room['first_node']}")
    finally:
        ssn.close()
    return errs


# ------------------------------------------------- against the oracle's allocate
ALLOCATE_SEEDS = {"random": (1, 5, 7, 8), "contended": (6, 7, 19, 21), "ports": (0, 1, 13, 19)}


def drained_alone(fx, node, cordon, walked):
    """The fixture in which the oracle's own allocate has to make the walk:
    the drained node and the cordon unschedulable, the walked pods Pending
    without a node in one new PodGroup with pod priorities descending in walk
    order (TaskOrderFn under the priority plugin reproduces the walk), every
    other Pending pod deleted, the queue not consulted (no proportion, no drf),
    allocate alone."""
    import copy
    rank = {uid: i for i, uid in enumerate(walked)}
    nodes = [dict(n, unschedulable=True) if n["name"] in (node,) + tuple(cordon) else n for n in fx["nodes"]]
    pods = []
    for p in fx["pods"]:
        if p["uid"] in rank:
            q = copy.deepcopy(p)
            q.update(phase="Pending", nodeName="", namespace="drain", priority=len(walked) - rank[p["uid"]])
            q["annotations"] = dict(q.get("annotations") or {}, **{"scheduling.k8s.io/group-name": "moved"})
            pods.append(q)
        elif p["phase"] != "Pending":
            pods.append(p)
    groups = list(fx["podGroups"]) + [{"namespace": "drain", "name": "moved", "minMember": 1,
                                       "queue": fx["queues"][0]["name"], "creationTimestamp": 1}]
    tiers = [[{"name": "priority"}, {"name": "gang"}], [{"name": "predicates"}]]
    return dict(fx, nodes=nodes, pods=pods, podGroups=groups, tiers=tiers, actions=["allocate"])


def check_allocate(fx, most=3):
    """(errors, nodes compared, left out) of one fixture at open: for the first
    `most` nodes with a pod to move, without a cordon and with the node the
    first pod went to cordoned, the oracle's decisions for the moved pods, in
    its order, are the call's placed entries, and the moved pods it leaves
    undecided are the entries with node -1, on both paths. Left out (None):
    fixtures without the predicates plugin (an unschedulable node takes pods
    there) or with pod affinity; per node: a walk with a BestEffort pod
    (backfill's, after allocate) or whose pods' namespaces carry meaning the
    move would change; an oracle run that ends in ref_panic."""
    ssn, _ = ws.open_with_reasons(dict(fx, actions=["allocate"]))
    errs, said, left = [], 0, 0
    try:
        rules = ws.plugin_rules(ssn.tiers)
        if not rules["predicates"] or ts.has_pod_affinity(fx):
            return [], 0, None
        snap = Snap(ssn)
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        picked = [x for x, ts_ in enumerate(snap.order) if any(e[0] is not None and e[2] in MOVABLE for e in ts_)][:most]
        for x in picked:
            move = [e for e in snap.order[x] if e[0] is not None and e[2] in MOVABLE]
            if any(ts.empty(e[3]) for e in move):
                left += 1
                continue
            (plain,) = ssn.node_drain([x], (), BIG)
            first = next((n for _, n, _ in plain["places"] if n >= 0), None)
            for cordon in ((),) + (((first,),) if first is not None else ()):
                ref = run_oracle(drained_alone(fx, names[x], [names[c] for c in cordon], [e[1] for e in move]))
                if ref["status"] != "ok":
                    left += 1
                    continue
                moved = {e[1] for e in move}
                kinds = {"allocate": dr.ALLOCATE, "pipeline": dr.PIPELINE}
                dec = [(d["task"], d["node"], kinds[d["kind"]]) for d in ref["decisions"] if d["task"] in moved]
                for rows_of in (ssn.node_drain, lambda n, c, lim: host_rows(ssn, n, c, lim)):
                    (g,) = rows_of([x], cordon, BIG)
                    got = [(tasks[t].uid, names[n], k) for t, n, k in g["places"] if n >= 0]
                    if got != dec:
                        bad = next((i for i, (a, b) in enumerate(zip(got, dec)) if a != b), min(len(got), len(dec)))
                        errs.append(f"{fx['name']}: drain {names[x]}, cordon {cordon}: placed entries differ from the "
                                    f"oracle's allocate at {bad}: {got[bad:bad + 2]} against {dec[bad:bad + 2]}")
                    nowhere = sorted(tasks[t].uid for t, n, _ in g["places"] if n < 0)
                    if nowhere != sorted(moved - {d[0] for d in dec}):
                        errs.append(f"{fx['name']}: drain {names[x]}, cordon {cordon}: entries with node -1 {nowhere}, "
                                    f"the oracle leaves {sorted(moved - {d[0] for d in dec})}")
                said += 1
        return errs, said, left
    finally:
        ssn.close()


def check_kat(fx):
    """The hand-derived walks of tests/golden/kat_drain.json (host ports, a
    BestEffort pod, a cordon, a nil Node, a gang that breaks and gangs that do
    not), at open, on both paths."""
    ssn, _ = ws.open_with_reasons(fx)
    errs = []
    try:
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        kind = {dr.ALLOCATE: "allocate", dr.PIPELINE: "pipeline"}
        for exp in fx["expected"]["drain"]:
            for rows_of in (ssn.node_drain, lambda n, c, lim: host_rows(ssn, n, c, lim)):
                (g,) = rows_of([names.index(exp["node"])], [names.index(c) for c in exp["cordon"]], BIG)
                uid = tasks[g["first_unplaced"]].uid if g["first_unplaced"] >= 0 else None
                got = dict(g, node=exp["node"], cordon=exp["cordon"], first_unplaced=uid,
                           message=drain_message(dict(g, first_unplaced=uid)),
                           places=[[tasks[t].uid, names[n] if n >= 0 else None, kind[k] if n >= 0 else None]
                                   for t, n, k in g["places"]])
                want = dict(exp, valid=True)
                errs += [f"drain {exp['node']!r}, cordon {exp['cordon']}: {k} is {got[k]}, hand-derived {want[k]}"
                         for k in want if got[k] != want[k]]
    finally:
        ssn.close()
    return errs


def check_twin_oracle(fx, most=4):
    """The verdict of now under the oracle: for the first `most` nodes whose
    first movable pod has a request, a Pending twin of that pod (its spec,
    labels and affinity under another name and uid, in a PodGroup of its own)
    is the only Pending pod of the fixture, the drained node is unschedulable,
    and kbref runs allocate alone without the queue plugins. The moved pod still
    runs where it is, as the call counts it. The oracle's decision for the twin
    (node, kind), or none, is the place of the one-step walk, on both paths.
    (errors, walks compared); fixtures without the predicates plugin compare
    nothing (an unschedulable node takes pods there)."""
    import copy
    errs, said = [], 0
    ssn, _ = ws.open_with_reasons(dict(fx, actions=["allocate"]))
    try:
        if not ws.plugin_rules(ssn.tiers)["predicates"]:
            return [], 0
        snap = Snap(ssn)
        names = ssn.flat.node_names
        firsts = {}
        for x, tasks in enumerate(snap.order):
            e = next((e for e in tasks if e[0] is not None and e[2] in MOVABLE), None)
            if e is not None and not ts.empty(e[3]) and len(firsts) < most:
                firsts[x] = e
        for x, e in firsts.items():
            twin = copy.deepcopy(e[4])
            twin.update(uid="twin", name="twin", phase="Pending", nodeName="")
            twin.pop("deletionTimestamp", None)
            twin["annotations"] = dict(twin.get("annotations") or {}, **{"scheduling.k8s.io/group-name": "twin"})
            alone = dict(fx, actions=["allocate"],
                         tiers=[[{"name": "priority"}, {"name": "gang"}], [{"name": "predicates"}]],
                         nodes=[dict(n, unschedulable=True) if n["name"] == names[x] else n for n in fx["nodes"]],
                         pods=[p for p in fx["pods"] if p["phase"] != "Pending"] + [twin],
                         podGroups=list(fx["podGroups"]) + [{"namespace": twin.get("namespace"), "name": "twin",
                                                             "minMember": 1, "queue": fx["queues"][0]["name"],
                                                             "creationTimestamp": 1}])
            ref = run_oracle(alone)
            if ref["status"] != "ok":
                continue
            kinds = {"allocate": dr.ALLOCATE, "pipeline": dr.PIPELINE}
            want = next(((d["node"], kinds[d["kind"]]) for d in ref["decisions"] if d["task"] == "twin"), (None, 0))
            for rows_of in (ssn.node_drain, lambda n, c, lim: host_rows(ssn, n, c, lim)):
                (g,) = rows_of([x], (), 1)
                t, n, k = g["places"][0]
                got = (names[n] if n >= 0 else None, k)
                if got != want:
                    errs.append(f"{fx['name']}: drain {names[x]}: its first pod {e[1]} goes to {got}, the oracle's "
                                f"allocate puts its Pending twin on {want}")
            said += 1
        return errs, said
    finally:
        ssn.close()


def check_allocate_after(fx, most=3):
    """check_allocate for the tasks a cycle's own allocate put on a node: the
    session runs allocate and is asked; the oracle's allocate of the same
    fixture says which pods went where and in which order (its decision log),
    those pods are written into the fixture as Running pods of their nodes, and
    the oracle then allocates the moved pods of a node (those it held at open,
    then the decided ones in log order) as in check_allocate. Only nodes with a
    decision onto them are drained. (errors, walks compared, left out); left
    out: a first run that is not ok or pipelines (Releasing cannot be written as
    a pod), and per node what check_allocate leaves out."""
    ref0 = run_oracle(dict(fx, actions=["allocate"]))
    if ref0["status"] != "ok" or any(d["kind"] != "allocate" for d in ref0["decisions"]):
        return [], 0, None
    ssn, _ = ws.open_with_reasons(dict(fx, actions=["allocate"]))
    errs, said, left = [], 0, 0
    try:
        rules = ws.plugin_rules(ssn.tiers)
        if not rules["predicates"] or ts.has_pod_affinity(fx):
            return [], 0, None
        snap = Snap(ssn)
        if ts.run_actions(ssn, ["allocate"]) != "ok":
            return [], 0, None
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        where = {d["task"]: d["node"] for d in ref0["decisions"]}
        fx1 = dict(fx, pods=[dict(p, phase="Running", nodeName=where[p["uid"]]) if p["uid"] in where else p
                             for p in fx["pods"]])
        pend = {uid: req for _, uid, req, _, _ in snap.pending}
        for x in [i for i, nm in enumerate(names) if nm in where.values()][:most]:
            moved = [e[1] for e in snap.order[x] if e[0] is not None and e[2] in MOVABLE]
            reqs = [e[3] for e in snap.order[x] if e[0] is not None and e[2] in MOVABLE]
            tail = [d["task"] for d in ref0["decisions"] if d["node"] == names[x]]
            if any(ts.empty(r) for r in reqs + [pend[u] for u in tail]):
                left += 1
                continue
            moved += tail
            ref = run_oracle(drained_alone(fx1, names[x], (), moved))
            if ref["status"] != "ok":
                left += 1
                continue
            kinds = {"allocate": dr.ALLOCATE, "pipeline": dr.PIPELINE}
            dec = [(d["task"], d["node"], kinds[d["kind"]]) for d in ref["decisions"] if d["task"] in set(moved)]
            for rows_of in (ssn.node_drain, lambda n, c, lim: host_rows(ssn, n, c, lim)):
                (g,) = rows_of([x], (), BIG)
                if [tasks[t].uid for t, _, _ in g["places"]] != moved:
                    errs.append(f"{fx['name']}: drain {names[x]} after allocate: walks {[tasks[t].uid for t, _, _ in g['places']]}, "
                                f"the node's pods at open then the oracle's log give {moved}")
                got = [(tasks[t].uid, names[n], k) for t, n, k in g["places"] if n >= 0]
                if got != dec:
                    errs.append(f"{fx['name']}: drain {names[x]} after allocate: placed entries {got[:3]}, the oracle's "
                                f"allocate {dec[:3]}")
            said += 1
        return errs, said, left
    finally:
        ssn.close()


def dup_fixture():
    """A colliding pod key (node_info.go:101-106). Nodes k00..k02 of 4000m. k00
    holds m0 (named `dup`) and m1, 1000m each; k01 holds h0, 3000m, also named
    `dup` in the same namespace (Idle 1000m); k02 holds w0 4000m (Idle 0); c0,
    Pending, is a third `dup`, so the session tracks the key. Draining k00:
      m0 1000m  k01 Idle 1000m: an Allocate, but k01 already holds ns/dup:
                AddTask fails, the decision is reported and the view stays
      m1 1000m  k01 Idle is still 1000m                      -> k01 Allocate
    Without the rule m1 would find nothing."""
    def pod(uid, group, cpu, node_name, name=None):
        return {"uid": uid, "namespace": "ns", "name": name or uid, "phase": "Running" if node_name else "Pending",
                "nodeName": node_name, "annotations": {"scheduling.k8s.io/group-name": group},
                "containers": [{"requests": {"cpu": f"{cpu}m", "memory": "64Mi"}}]}
    nodes = [{"name": f"k{i:02d}", "allocatable": {"cpu": "4000m", "memory": "8192Mi", "pods": "110"}, "labels": {}}
             for i in range(3)]
    pods = [pod("m0", "M", 1000, "k00", "dup"), pod("m1", "M", 1000, "k00"), pod("h0", "H", 3000, "k01", "dup"),
            pod("w0", "W", 4000, "k02"), pod("c0", "C", 500, "", "dup")]
    groups = [{"namespace": "ns", "name": g, "minMember": 1, "queue": "q", "creationTimestamp": t * 10 ** 9}
              for t, g in enumerate("MHWC", 1)]
    tiers = [[{"name": "priority"}, {"name": "gang"}], [{"name": "drf"}, {"name": "predicates"}, {"name": "proportion"}]]
    return {"name": "drain-dup", "actions": ["allocate"], "tiers": tiers, "nodes": nodes,
            "queues": [{"name": "q", "weight": 1}], "podGroups": groups, "pods": pods}


def check_dup():
    """The hand-worked walk of dup_fixture, at open, on both paths (the host's: the key collides)."""
    ssn, _ = ws.open_with_reasons(dup_fixture())
    errs = []
    try:
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        want = [("m0", "k01", dr.ALLOCATE), ("m1", "k01", dr.ALLOCATE)]
        for rows_of in (ssn.node_drain, lambda n, c, lim: host_rows(ssn, n, c, lim)):
            (g,) = rows_of([names.index("k00")], (), BIG)
            got = [(tasks[t].uid, names[n] if n >= 0 else None, k) for t, n, k in g["places"]]
            if got != want or (g["placed_idle"], g["nodes_used"], g["unplaced"]) != (2, 1, 0):
                errs.append(f"drain k00: walk {got}, hand-worked {want}; row {g}")
    finally:
        ssn.close()
    return errs
