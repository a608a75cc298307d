"""Plain reference of the pending-task reasons (kbg_task_reasons; the contract
of kbg_task_why_kernel in kube-arbitrator_amd/csrc/kbg_device.hpp): per shape
and per node, on lists and Python floats, in the order of allocate.go:119-162,
backfill.go:50-64 and predicates.go:125-183.

A case `c` holds
  c.p         n_nodes, W, tab_lo, tab_n, stride, classes, n_shapes, cap_check
  c.idle, c.rel      [stride][3] rows of the node table (row = node - tab_lo)
  c.ntasks, c.maxtasks   [stride]
  c.live, c.unsched  [n_nodes] by global node; c.sel_ok, c.taint_ok [classes][n_nodes]
  c.shapes    dicts cls, best_effort, req [3]
`rows(c)` gives one row per shape: count[10], first_node[10], idle_short[3].
`rows(c, defect)` restates one of DEFECTS, a mistake a kernel could make; the
comparator must report each (tests/test_task_why_ref.py)."""

MIN = (10.0, 10.0 * 1024.0 * 1024.0, 10.0)  # resource_info.go:54-56
N_CAUSES = 10
POD_CAP, SELECTOR, HOST_PORTS, UNSCHEDULABLE, TAINTS, POD_AFFINITY, FITS_IDLE, FITS_RELEASING, SHORT, PANIC = range(10)
CAUSE_NAMES = ("pod_cap", "selector", "host_ports", "unschedulable", "taints", "pod_affinity", "fits_idle",
               "fits_releasing", "short", "panic")
DEFECTS = ("stage_swap", "cap_gt", "no_tolerance", "releasing_first", "short_on_idle", "zero_dim_short", "be_tested",
           "garbage_counted", "dead_counted", "first_node_last", "offset_dropped")


def less_equal(r, a, defect=None):
    """Resource.LessEqual (resource_info.go:142-146): per dimension r < a || |a - r| < min."""
    if defect == "no_tolerance":
        return all(r[d] <= a[d] for d in range(3))
    return all(r[d] < a[d] or abs(a[d] - r[d]) < MIN[d] for d in range(3))


def fit_delta_negative(idle, req, defect=None):
    """Idle.FitDelta(req) (resource_info.go:116-129): the dimensions left negative."""
    out = []
    for d in range(3):
        v = idle[d]
        if req[d] > 0 or defect == "zero_dim_short":
            v = v - (req[d] + MIN[d])
        out.append(v < 0)
    return out


def cause(c, shape, row, n, defect=None):
    """(cause, [cpu, memory, GPU short]) of table row `row`, global node n."""
    cls = shape["cls"]
    none = [False] * 3
    if c.p["cap_check"]:
        capped = c.ntasks[row] > c.maxtasks[row] if defect == "cap_gt" else c.ntasks[row] >= c.maxtasks[row]
        if capped:
            return POD_CAP, none
        if not c.sel_ok[cls][n]:
            return SELECTOR, none
        stages = ((TAINTS, not c.taint_ok[cls][n]), (UNSCHEDULABLE, c.unsched[n]))
        for code, fails in (stages if defect == "stage_swap" else stages[::-1]):
            if fails:
                return code, none
    idle, rel, req = c.idle[row], c.rel[row], shape["req"]
    if shape["best_effort"] and defect != "be_tested":
        return FITS_IDLE, none
    fi, fr = less_equal(req, idle, defect), less_equal(req, rel, defect)
    if defect == "releasing_first" and fr:
        return FITS_RELEASING, fit_delta_negative(idle, req)
    if fi:
        return FITS_IDLE, (fit_delta_negative(idle, req) if defect == "short_on_idle" else none)
    return (FITS_RELEASING if fr else SHORT), fit_delta_negative(idle, req, defect)


def empty_row():
    return dict(count=[0] * N_CAUSES, first_node=[-1] * N_CAUSES, idle_short=[0, 0, 0])


def rows(c, defect=None):
    lo, nn, N = c.p["tab_lo"], c.p["tab_n"], c.p["n_nodes"]
    out = []
    for shape in c.shapes:
        r = empty_row()
        end = nn
        if defect == "garbage_counted":  # the bits of the last word past the table's end, as a clamped lane sees them
            end = (nn + 63) // 64 * 64
        for row in range(end):
            n = lo + row
            if row >= nn:  # (the planes hold ones there; the lane reads the table's last row)
                k, short = cause(c, shape, nn - 1, min(n, N - 1), defect)
            else:
                pn = row if defect == "offset_dropped" else n
                if not c.live[pn] and defect != "dead_counted":
                    continue
                k, short = cause(c, shape, row, pn, defect)
                n = pn
            r["count"][k] += 1
            if r["first_node"][k] < 0 or n < r["first_node"][k] or defect == "first_node_last":
                r["first_node"][k] = n
            for d in range(3):
                r["idle_short"][d] += bool(short[d])
        out.append(r)
    return out


def compare(c, want, got):
    """Readable differences between two lists of rows (reference first)."""
    errs = []
    for si, (w, g) in enumerate(zip(want, got)):
        s = c.shapes[si]
        tag = f"shape {si} (cls {s['cls']}, best_effort {s['best_effort']}, req {s['req']})"
        for k in range(N_CAUSES):
            if w["count"][k] != g["count"][k]:
                errs.append(f"{tag}: count[{CAUSE_NAMES[k]}] is {g['count'][k]}, reference {w['count'][k]}")
            if w["first_node"][k] != g["first_node"][k]:
                errs.append(f"{tag}: first_node[{CAUSE_NAMES[k]}] is {g['first_node'][k]}, "
                            f"reference {w['first_node'][k]}")
        for d, name in enumerate(("cpu", "memory", "GPU")):
            if w["idle_short"][d] != g["idle_short"][d]:
                errs.append(f"{tag}: idle_short[{name}] is {g['idle_short'][d]}, reference {w['idle_short'][d]}")
    if len(want) != len(got):
        errs.append(f"{len(got)} rows, reference {len(want)}")
    return errs
