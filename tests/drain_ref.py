"""Plain reference of the node drain walk (kbg_node_drain; the contract of
kbg_drain_kernel in kube-arbitrator_amd/csrc/kbg_device.hpp): per walk, on
lists and Python floats (the same IEEE doubles), its steps in order, each to
the first node that takes it against a view private to the walk, in which the
walk's drained node and the launch's cordon take nothing (allocate.go:119-162,
backfill.go:47-64, node_info.go:101-129). A plain loop per walk, no cursor:
every step looks at every node from the table's first.

A case `c` holds what a case of tests/task_why_ref.py holds, and
  c.shapes    dicts cls, best_effort, req [3] (best_effort: no resource test)
  c.walks     one list of shape indices per walk
  c.drain     per walk the global node that takes nothing in it, or -1; a node
              outside the table range [tab_lo, tab_lo + tab_n) excludes nothing
  c.cordon    the global nodes that take nothing in any walk
`walks(c)` gives per walk one (node, kind) per step, node -1 (and kind 0) for a
step no node takes. `walks(c, defect)` restates one of DEFECTS, a mistake a
kernel could make; the comparator must report each (tests/test_drain_ref.py).
The defect `guard_written` changes no walk: tests/drain_cases.py writes it
into the raw bytes."""

MIN = (10.0, 10.0 * 1024.0 * 1024.0, 10.0)  # resource_info.go:54-56
MAX_STEPS = 512
ALLOCATE, PIPELINE = 0, 1
DEFECTS = ("drained_not_excluded", "cordon_ignored", "exclusion_leaks", "best_effort_resource_test",
           "best_effort_not_counted", "cursor_across_walks", "idle_everywhere_first", "no_overlay",
           "guard_written", "drained_row_as_node", "exclusion_needs_cap_check", "stops_at_unplaced")


def less_equal(r, a):
    """Resource.LessEqual (resource_info.go:142-146): per dimension r < a || |a - r| < min."""
    return all(r[d] < a[d] or abs(a[d] - r[d]) < MIN[d] for d in range(3))


def links(c, walk_):
    """The `prev` of each step of a walk: the previous step of the same shape,
    -1 for the first and for a shape with a negative request dimension. A
    BestEffort shape keeps its links."""
    last, out = {}, []
    for i, s in enumerate(walk_):
        ok = all(v >= 0 for v in c.shapes[s]["req"])
        out.append(last.get(s, -1) if ok else -1)
        last[s] = i
    return out


def walk(c, j, defect=None, carried=None):
    """Walk j of the case: [(node, kind)] per step. `carried` is the state the
    defects that leak from walk to walk keep (a dict, shared by the caller)."""
    lo, nn = c.p["tab_lo"], c.p["tab_n"]
    carried = {} if carried is None else carried
    steps = c.walks[j]
    gone = set(c.cordon)
    if defect == "cordon_ignored" or (defect == "exclusion_needs_cap_check" and not c.p["cap_check"]):
        gone = set()
    x = c.drain[j]
    if defect == "drained_row_as_node" and x >= 0:
        x = x - lo  # (the walk's table row taken for a global node: the exclusion moves down by tab_lo)
    if x >= 0 and defect != "drained_not_excluded" and not (defect == "exclusion_needs_cap_check"
                                                            and not c.p["cap_check"]):
        gone.add(x)
    if defect == "exclusion_leaks":
        gone |= carried.setdefault("gone", set())
        if c.drain[j] >= 0:
            carried["gone"].add(c.drain[j])
    view = {}  # row -> [idle, rel, ntasks]
    out, stopped = [], False
    for s in steps:
        sh = c.shapes[s]
        req, cls, beff = sh["req"], sh["cls"], sh["best_effort"]
        if defect == "best_effort_resource_test":
            beff = False
        start = 0
        if defect == "cursor_across_walks":
            start = carried.setdefault("land", {}).get(s, 0)

        def state(row):
            seen = row in view and defect != "no_overlay"
            return view[row] if seen else [list(c.idle[row]), list(c.rel[row]), c.ntasks[row]]

        def passes(row, st):
            n = lo + row
            if not c.live[n] or n in gone:
                return False
            if not c.p["cap_check"]:
                return True
            return st[2] < c.maxtasks[row] and c.sel_ok[cls][n] and not c.unsched[n] and c.taint_ok[cls][n]

        def take(row, st):
            if beff or less_equal(req, st[0]):
                return ALLOCATE
            if less_equal(req, st[1]):
                return PIPELINE
            return None

        at, kind = -1, ALLOCATE
        if not stopped:
            if defect == "idle_everywhere_first" and not beff:
                for k in (ALLOCATE, PIPELINE):
                    for row in range(start, nn):
                        st = state(row)
                        if passes(row, st) and less_equal(req, st[k]):
                            at, kind = row, k
                            break
                    if at >= 0:
                        break
            else:
                for row in range(start, nn):
                    st = state(row)
                    if not passes(row, st):
                        continue
                    k = take(row, st)
                    if k is None:
                        continue
                    at, kind = row, k
                    break
        if at >= 0:
            st = state(at)
            st[kind] = [st[kind][d] - req[d] for d in range(3)]  # Resource.Sub, plain fp64 per dimension
            if not (sh["best_effort"] and defect == "best_effort_not_counted"):
                st[2] += 1
            view[at] = st
        elif defect == "stops_at_unplaced":
            stopped = True
        if defect == "cursor_across_walks":
            carried["land"][s] = at if at >= 0 else nn
        out.append((-1 if at < 0 else lo + at, kind if at >= 0 else 0))
    return out


def walks(c, defect=None):
    carried = {}
    return [walk(c, j, defect, carried) for j in range(len(c.walks))]


def compare(c, want, got):
    """Readable differences between two lists of walks (reference first)."""
    errs = []
    for j, (w, g) in enumerate(zip(want, got)):
        for i, (a, b) in enumerate(zip(w, g)):
            if tuple(a) != tuple(b):
                s = c.shapes[c.walks[j][i]]
                errs.append(f"walk {j} (drains {c.drain[j]}) step {i} (shape {c.walks[j][i]}: cls {s['cls']}, "
                            f"req {s['req']}, best effort {s['best_effort']}): (node, kind) is {tuple(b)}, "
                            f"reference {tuple(a)}")
        if len(w) != len(g):
            errs.append(f"walk {j}: {len(g)} steps, reference {len(w)}")
    if len(want) != len(got):
        errs.append(f"{len(got)} walks, reference {len(want)}")
    return errs


def row_of(places, task_job, ready_num, min_available):
    """The call's derived row fields from one node's (task, node, kind)
    places: task_job maps a task to its job, ready_num and min_available a job
    to its gang's numbers now (gang.go:44-78)."""
    placed = [p for p in places if p[1] >= 0]
    lost = {}
    for p in places:
        if p[1] < 0:
            lost[task_job[p[0]]] = lost.get(task_job[p[0]], 0) + 1
    short = sum(1 for j, k in lost.items() if ready_num[j] >= min_available[j] > ready_num[j] - k)
    return dict(walked=len(places), placed_idle=sum(p[2] == ALLOCATE for p in placed),
                placed_releasing=sum(p[2] == PIPELINE for p in placed), unplaced=len(places) - len(placed),
                first_unplaced=next((p[0] for p in places if p[1] < 0), -1), nodes_used=len({p[1] for p in placed}),
                jobs_moved=len({task_job[p[0]] for p in places}), jobs_short=short)
