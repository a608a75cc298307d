"""Plain reference of kbg_victim_reasons' per-node rule: under which cause a
live node goes for one query (a reclaimer or preemptor with its mode, class,
tiers, request and drf share), restated per node on lists and dicts. Nothing
of the kernels' chunks, lanes, masks or buffers is in it; the tables are those
of tests/victim_ref.py (its `state`), the stage planes are lists of booleans
per node.

The order (preempt.go:181-202, reclaim.go:112-150, session_plugins.go:59-140):
  a node that is not live is not visited;
  a nil Node under the predicates plugin                       -> PANIC;
  with the predicates plugin on (cap_check), the first failing stage in the
  plugin's order: pod cap (0), selector (1), unschedulable (3), taints (4);
  no Running task passes the mode's filter                      -> NO_PREEMPTEES;
  tier by tier, every enabled fn over the whole preemptee list, intersected: a
  Resource.Sub underflow in a tier the walk reaches -> PANIC; the first tier
  with a non-empty intersection decides; none (or no tier)      -> NO_VICTIMS;
  the victims' sum Less than the request                        -> NOT_ENOUGH;
  otherwise                                                     -> VICTIMS.
fn_empty[f] counts the NO_VICTIMS nodes where fn f is enabled in some tier and
keeps nobody of the whole preemptee list by itself.

`defect` selects one deliberately wrong variant (DEFECTS); the tests use them
to show that the cases and the comparator would notice a kernel, a launcher or
a fan-out that is wrong in that way."""
from victim_ref import is_preemptee, less, less_equal, share, state  # noqa: F401  (state: re-exported)

VP_GANG, VP_DRF, VP_PROP = 1, 2, 4
POD_CAP, SELECTOR, HOST_PORTS, UNSCHEDULABLE, TAINTS, POD_AFFINITY = range(6)
NO_PREEMPTEES, NO_VICTIMS, NOT_ENOUGH, VICTIMS, PANIC, N_CAUSES = range(6, 12)
CAUSE_NAMES = ("pod_cap", "selector", "host_ports", "unschedulable", "taints", "pod_affinity", "no_preemptees",
               "no_victims", "not_enough", "victims", "panic")
MAX_NODE_CANDIDATES = 1024

DEFECTS = ("cap_after_selector", "unsched_before_selector", "dead_counted", "no_preemptees_merged",
           "fn_empty_intersection", "first_node_last", "big_counted_twice", "row_not_cleared",
           "not_enough_preemptees", "last_lane_lost", "panic_dropped", "fanout_second_empty")


class _Underflow(Exception):
    pass


def cause(c, s, q, n, defect=None):
    """(cause, fn_empty) of live node n for query q; fn_empty is a set of fn
    bits and is empty unless the cause is NO_VICTIMS."""
    row = n - c.p["node_lo"]
    if c.panic_node[n] and defect != "panic_dropped":  # predicates.go:122-123
        return PANIC, set()
    if q["cap_check"]:
        capped = s.ntasks[row] >= s.maxtasks[row]
        sel, uns, tol = c.sel_ok[q["cls"]][n], c.unsched[n], c.taint_ok[q["cls"]][n]
        if defect == "cap_after_selector":
            order = ((not sel, SELECTOR), (capped, POD_CAP), (uns, UNSCHEDULABLE), (not tol, TAINTS))
        elif defect == "unsched_before_selector":
            order = ((capped, POD_CAP), (uns, UNSCHEDULABLE), (not sel, SELECTOR), (not tol, TAINTS))
        else:
            order = ((capped, POD_CAP), (not sel, SELECTOR), (uns, UNSCHEDULABLE), (not tol, TAINTS))
        for failed, code in order:
            if failed:
                return code, set()
    off, L = int(c.nt_off[n]), int(c.nt_off[n + 1] - c.nt_off[n])
    job = lambda k: int(c.c_jq[off + k][0])
    queue = lambda k: int(c.c_jq[off + k][1])
    req = lambda k: s.c_req[off + k]
    pre = [k for k in range(L) if s.c_run[off + k] and is_preemptee(q, job(k), queue(k))
           and not (defect == "last_lane_lost" and k % 64 == 63)]
    if not pre:
        return (NO_VICTIMS if defect == "no_preemptees_merged" else NO_PREEMPTEES), set()

    def sub(a, r):  # Resource.Sub (resource_info.go:100-110)
        if not less_equal(r, a, s.kmin) and defect != "panic_dropped":
            raise _Underflow()
        for d in range(3):
            a[d] = a[d] - r[d]

    def gang():  # gang.go:104-124
        return {k for k in pre if int(c.j_min[job(k)]) <= s.j_ready[job(k)] - 1}

    def drf():  # drf.go:80-105
        keep, alloc = set(), {}
        for k in pre:
            a = alloc.setdefault(job(k), list(s.j_alloc[job(k)]))
            sub(a, req(k))
            rs = share(a, s.total)
            if q["ls"] < rs or abs(q["ls"] - rs) <= s.share_delta:
                keep.add(k)
        return keep

    def prop():  # proportion.go:161-186
        keep, alloc = set(), {}
        for k in pre:
            a = alloc.setdefault(queue(k), list(s.q_alloc[queue(k)]))
            if less(a, req(k)):
                continue
            sub(a, req(k))
            if less_equal(s.q_deserved[queue(k)], a, s.kmin):
                keep.add(k)
        return keep

    empty = set()
    for fns in q["tier_fns"][:q["n_tiers"]]:
        try:
            own = {f: fn() for f, fn in ((VP_GANG, gang), (VP_DRF, drf), (VP_PROP, prop)) if fns & f}
        except _Underflow:
            return PANIC, set()
        victims = [k for k in pre if all(k in keep for keep in own.values())]
        if defect == "fn_empty_intersection":
            empty |= {f for f in own if not victims}
        else:
            empty |= {f for f, keep in own.items() if not keep}
        if victims:
            total = [0, 0, 0]  # validateVictims (preempt.go:242-253)
            for k in (pre if defect == "not_enough_preemptees" else victims):
                for d in range(3):
                    total[d] = total[d] + req(k)[d]
            return (NOT_ENOUGH if less(total, [float(v) for v in q["req"]]) else VICTIMS), set()
    return NO_VICTIMS, empty


def empty_row():
    return dict(count=[0] * N_CAUSES, first_node=[-1] * N_CAUSES, fn_empty=[0, 0, 0])


def rows(c, defect=None, huge=True):
    """One row per query of c.queries: count, first_node, fn_empty over the
    live nodes of [node_lo, node_lo + node_n). huge=False leaves out the nodes
    holding more than MAX_NODE_CANDIDATES candidates (the launchers do; the
    session adds them on the host)."""
    s = state(c, prep=False)
    lo, nn = c.p["node_lo"], c.p["node_n"]
    out = []
    for qi, q in enumerate(c.queries):
        if defect == "fanout_second_empty" and any(q == p for p in c.queries[:qi]):
            out.append(empty_row())
            continue
        r = empty_row()
        if defect == "row_not_cleared" and qi:
            r = dict(count=list(out[-1]["count"]), first_node=list(out[-1]["first_node"]),
                     fn_empty=list(out[-1]["fn_empty"]))
        for n in range(lo, lo + nn):
            L = int(c.nt_off[n + 1] - c.nt_off[n])
            if not c.live[n] and defect != "dead_counted":
                continue
            if L > MAX_NODE_CANDIDATES and not huge:
                continue
            k, fn = cause(c, s, q, n, defect)
            for _ in range(2 if defect == "big_counted_twice" and 128 < L <= MAX_NODE_CANDIDATES else 1):
                r["count"][k] += 1
                for f in range(3):
                    r["fn_empty"][f] += (1 << f) in fn
            if r["first_node"][k] < 0 or n < r["first_node"][k] or defect == "first_node_last":
                r["first_node"][k] = n
        out.append(r)
    return out


def compare(c, want, got):
    """Readable differences between two lists of rows (reference first)."""
    errs = []
    for qi, (w, g) in enumerate(zip(want, got)):
        q = c.queries[qi]
        tag = f"query {qi} (mode {q['mode']}, cls {q['cls']}, job {q['job']}, tiers {q['tier_fns'][:q['n_tiers']]})"
        for k in range(N_CAUSES):
            if w["count"][k] != g["count"][k]:
                errs.append(f"{tag}: count[{CAUSE_NAMES[k]}] is {g['count'][k]}, reference {w['count'][k]}")
            if w["first_node"][k] != g["first_node"][k]:
                errs.append(f"{tag}: first_node[{CAUSE_NAMES[k]}] is {g['first_node'][k]}, "
                            f"reference {w['first_node'][k]}")
        for f, name in enumerate(("gang", "drf", "proportion")):
            if w["fn_empty"][f] != g["fn_empty"][f]:
                errs.append(f"{tag}: fn_empty[{name}] is {g['fn_empty'][f]}, reference {w['fn_empty'][f]}")
    if len(want) != len(got):
        errs.append(f"{len(got)} rows, reference {len(want)}")
    return errs
