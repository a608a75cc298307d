"""Plain reference of the job fit walk (kbg_job_fit; the contract of
kbg_job_fit_kernel in kube-arbitrator_amd/csrc/kbg_device.hpp): per job, on
lists and Python floats (the same IEEE doubles), its steps in order, each to
the first node that takes it against a view private to the job
(allocate.go:119-162, node_info.go:101-129). No cursor: every step looks at
every node from the table's first.

A case `c` holds what a case of tests/task_why_ref.py holds, and c.jobs:
  c.p         n_nodes, W, tab_lo, tab_n, stride, classes, n_shapes, cap_check
  c.idle, c.rel      [stride][3] rows of the node table (row = node - tab_lo)
  c.ntasks, c.maxtasks   [stride]
  c.live, c.unsched  [n_nodes] by global node; c.sel_ok, c.taint_ok [classes][n_nodes]
  c.shapes    dicts cls, best_effort (never set here), req [3]
  c.jobs      one list of shape indices per job: its walk
`walks(c)` gives per job one (node, kind) per step, node -1 (and kind 0) for a
step no node takes. `walks(c, defect)` restates one of DEFECTS, a mistake a
kernel could make; the comparator must report each (tests/test_job_fit_ref.py)."""

MIN = (10.0, 10.0 * 1024.0 * 1024.0, 10.0)  # resource_info.go:54-56
MAX_STEPS = 512
ALLOCATE, PIPELINE = 0, 1
DEFECTS = ("no_overlay", "touched_lost", "rel_not_subtracted", "pods_not_counted", "idle_everywhere_first",
           "one_cursor", "exclusive_cursor", "stops_at_unplaced", "kinds_swapped", "local_nodes", "dead_takes",
           "ragged_counted")


def less_equal(r, a):
    """Resource.LessEqual (resource_info.go:142-146): per dimension r < a || |a - r| < min."""
    return all(r[d] < a[d] or abs(a[d] - r[d]) < MIN[d] for d in range(3))


def links(c, job):
    """The `prev` of each step of a walk: the previous step of the same shape,
    -1 for the first and for a shape with a negative request dimension."""
    last, out = {}, []
    for i, s in enumerate(job):
        ok = all(v >= 0 for v in c.shapes[s]["req"])
        out.append(last.get(s, -1) if ok else -1)
        last[s] = i
    return out


def walk(c, job, defect=None):
    """One job's walk: [(node, kind)] per step."""
    lo, nn, N = c.p["tab_lo"], c.p["tab_n"], c.p["n_nodes"]
    view = {}  # row -> [idle, rel, ntasks]
    first_word = None  # (touched_lost: the only word whose overlay is read)
    end = (nn + 63) // 64 * 64 if defect == "ragged_counted" else nn
    out, land, stopped = [], [], False
    prev = links(c, job)
    for i, s in enumerate(job):
        sh = c.shapes[s]
        req, cls = sh["req"], sh["cls"]
        start = 0
        if defect == "one_cursor" and i > 0:
            start = land[i - 1] if land[i - 1] >= 0 else nn
        if defect == "exclusive_cursor" and prev[i] >= 0:
            start = land[prev[i]] + 1 if land[prev[i]] >= 0 else nn

        def state(row):
            src = min(row, nn - 1)  # (a lane past the table reads its last row, never the overlay)
            seen = row in view and row < nn and defect != "no_overlay"
            if defect == "touched_lost" and row // 64 != first_word:
                seen = False
            return view[row] if seen else [list(c.idle[src]), list(c.rel[src]), c.ntasks[src]]

        def passes(row, st):
            n = lo + row
            if n >= N:  # the planes hold ones there
                return not c.p["cap_check"]
            if not c.live[n] and defect != "dead_takes":
                return False
            if not c.p["cap_check"]:
                return True
            src = min(row, nn - 1)
            return st[2] < c.maxtasks[src] and c.sel_ok[cls][n] and not c.unsched[n] and c.taint_ok[cls][n]

        at, kind = -1, ALLOCATE
        if not stopped:
            if defect == "idle_everywhere_first":
                for k, which in ((ALLOCATE, 0), (PIPELINE, 1)):
                    for row in range(start, end):
                        st = state(row)
                        if passes(row, st) and less_equal(req, st[which]):
                            at, kind = row, k
                            break
                    if at >= 0:
                        break
            else:
                for row in range(start, end):
                    st = state(row)
                    if not passes(row, st):
                        continue
                    if less_equal(req, st[0]):
                        at, kind = row, ALLOCATE
                    elif less_equal(req, st[1]):
                        at, kind = row, PIPELINE
                    else:
                        continue
                    break
        if at >= 0:
            st = state(at)
            if not (kind == PIPELINE and defect == "rel_not_subtracted"):
                st[kind] = [st[kind][d] - req[d] for d in range(3)]  # Resource.Sub, plain fp64 per dimension
            if defect != "pods_not_counted":
                st[2] += 1
            view[at] = st
            if first_word is None:
                first_word = at // 64
        elif defect == "stops_at_unplaced":
            stopped = True
        land.append(at)
        node = -1 if at < 0 else (at if defect == "local_nodes" else lo + at)
        shown = kind if at >= 0 else 0
        if defect == "kinds_swapped" and at >= 0:
            shown = 1 - kind
        out.append((node, shown))
    return out


def walks(c, defect=None):
    return [walk(c, job, defect) for job in c.jobs]


def compare(c, want, got):
    """Readable differences between two lists of walks (reference first)."""
    errs = []
    for j, (w, g) in enumerate(zip(want, got)):
        for i, (a, b) in enumerate(zip(w, g)):
            if tuple(a) != tuple(b):
                s = c.shapes[c.jobs[j][i]]
                errs.append(f"job {j} step {i} (shape {c.jobs[j][i]}: cls {s['cls']}, req {s['req']}): "
                            f"(node, kind) is {tuple(b)}, reference {tuple(a)}")
        if len(w) != len(g):
            errs.append(f"job {j}: {len(g)} steps, reference {len(w)}")
    if len(want) != len(got):
        errs.append(f"{len(got)} jobs, reference {len(want)}")
    return errs


def rows_of(places, ready_num, min_available):
    """The call's derived row fields from one job's (task, node, kind) places."""
    placed = [p for p in places if p[1] >= 0]
    ready_after = 0 if ready_num >= min_available else -1
    k = 0
    for i, p in enumerate(places):
        k += p[1] >= 0
        if ready_after < 0 and p[1] >= 0 and ready_num + k >= min_available:
            ready_after = i + 1
    return dict(walked=len(places), placed_idle=sum(p[2] == ALLOCATE for p in placed),
                placed_releasing=sum(p[2] == PIPELINE for p in placed),
                first_unplaced=next((p[0] for p in places if p[1] < 0), -1),
                nodes_used=len({p[1] for p in placed}), ready_after=ready_after)
