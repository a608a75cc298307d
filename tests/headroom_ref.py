"""Plain reference of the pending-task headroom (kbg_task_headroom; the
contract of kbg_task_headroom_kernel in kube-arbitrator_amd/csrc/
kbg_device.hpp): per shape and per node, on lists and Python floats (the same
IEEE doubles), the copies allocate would put on the node one after the other
(allocate.go:119-162, node_info.go:101-129, resource_info.go:100-110,142-146)
under the pod cap of predicates.go:125-127.

A case `c` holds what a case of tests/task_why_ref.py holds, and c.p["limit"]:
  c.p         n_nodes, W, tab_lo, tab_n, stride, classes, n_shapes, cap_check, limit
  c.idle, c.rel      [stride][3] rows of the node table (row = node - tab_lo)
  c.ntasks, c.maxtasks   [stride]
  c.live, c.unsched  [n_nodes] by global node; c.sel_ok, c.taint_ok [classes][n_nodes]
  c.shapes    dicts cls, best_effort, req [3]
`node_copies` gives one node's (passes, k_idle, k_rel, cut); `rows(c)` one row
per shape with the keys of KEYS, the order of the device row's words.
`rows(c, defect)` restates one of DEFECTS, a mistake a kernel could make; the
comparator must report each (tests/test_headroom_ref.py)."""

MIN = (10.0, 10.0 * 1024.0 * 1024.0, 10.0)  # resource_info.go:54-56
INT32_MAX = 2 ** 31 - 1
MAX_LIMIT = 1024
KEYS = ("copies_idle", "copies_releasing", "nodes_idle", "nodes_releasing_only", "first_node", "max_node_copies",
        "nodes_pass", "limit_hit")
DEFECTS = ("rel_restart", "room_ignored", "limit_ignored", "division", "no_tolerance", "last_lane_lost",
           "ragged_counted", "first_node_local", "max_idle_only", "limit_hit_eq", "be_tested", "wrong_class")


def less_equal(r, a, defect=None):
    """Resource.LessEqual (resource_info.go:142-146): per dimension r < a || |a - r| < min."""
    if defect == "no_tolerance":
        return all(r[d] <= a[d] for d in range(3))
    return all(r[d] < a[d] or abs(a[d] - r[d]) < MIN[d] for d in range(3))


def passes(c, cls, row, n):
    """The static stages of predicates.go:125-183; none with cap_check 0."""
    if not c.p["cap_check"]:
        return True
    return c.ntasks[row] < c.maxtasks[row] and c.sel_ok[cls][n] and not c.unsched[n] and c.taint_ok[cls][n]


def take(req, have, i, bound, defect=None):
    """Copies i, i + 1, ... below `bound` taken from `have` one at a time: the count after the last that fits."""
    if defect == "division":  # a closed form in place of the iteration
        ks = [int(have[d] // req[d]) for d in range(3) if req[d] > 0]
        return max(i, min(bound, i + max(0, min(ks)))) if ks else bound
    a = list(have)
    while i < bound and less_equal(req, a, defect):
        a = [a[d] - req[d] for d in range(3)]  # Resource.Sub, plain fp64 per dimension
        i += 1
    return i


def node_copies(c, shape, row, n, defect=None):
    """(passes, k_idle, k_rel, cut) of table row `row`, global node n."""
    cls = shape["cls"]
    if defect == "wrong_class":
        cls = (cls + 1) % c.p["classes"]
    if not passes(c, cls, row, n):
        return False, 0, 0, False
    limit = c.p["limit"]
    room = c.maxtasks[row] - c.ntasks[row] if c.p["cap_check"] else INT32_MAX
    bound = min(limit, room)
    if defect == "room_ignored":
        bound = limit
    if defect == "limit_ignored":
        bound = room
    if shape["best_effort"] and defect != "be_tested":  # backfill.go:47-60
        k_idle = k = bound
    else:
        k_idle = take(shape["req"], c.idle[row], 0, bound, defect)
        if defect == "rel_restart":
            k = k_idle + take(shape["req"], c.rel[row], 0, bound, defect)
        else:
            k = take(shape["req"], c.rel[row], k_idle, bound, defect)
    cut = k == limit and (limit <= room if defect == "limit_hit_eq" else limit < room)
    return True, k_idle, k - k_idle, cut


def copies(req, idle, rel, room, limit, best_effort):
    """(k_idle, k_rel, cut) of one node past the stages, from plain values (the session checks)."""
    bound = min(limit, room)
    k_idle = bound if best_effort else take(req, idle, 0, bound)
    k = k_idle if best_effort else take(req, rel, k_idle, bound)
    return k_idle, k - k_idle, k == limit and limit < room


def empty_row():
    return dict(copies_idle=0, copies_releasing=0, nodes_idle=0, nodes_releasing_only=0, first_node=-1,
                max_node_copies=0, nodes_pass=0, limit_hit=0)


def add_node(r, n, k_idle, k_rel, cut, defect=None, row=None):
    """One node past the stages into its shape's row."""
    r["nodes_pass"] += 1
    r["copies_idle"] += k_idle
    r["copies_releasing"] += k_rel
    r["nodes_idle"] += k_idle > 0
    r["nodes_releasing_only"] += k_idle == 0 and k_rel > 0
    if k_idle + k_rel > 0:
        at = row if defect == "first_node_local" else n
        if r["first_node"] < 0 or at < r["first_node"]:
            r["first_node"] = at
    r["max_node_copies"] = max(r["max_node_copies"], k_idle if defect == "max_idle_only" else k_idle + k_rel)
    r["limit_hit"] += bool(cut)


def rows(c, defect=None):
    lo, nn, N = c.p["tab_lo"], c.p["tab_n"], c.p["n_nodes"]
    out = []
    for shape in c.shapes:
        r = empty_row()
        end = nn
        if defect == "ragged_counted":  # the bits of the last word past the table's end, as a clamped lane sees them
            end = (nn + 63) // 64 * 64
        for row in range(end):
            n = lo + row
            if defect == "last_lane_lost" and n % 64 == 63:
                continue
            if row >= nn:  # (the planes hold ones there; the lane reads the table's last row)
                ok, ki, kr, cut = node_copies(c, shape, nn - 1, min(n, N - 1), defect)
            else:
                if not c.live[n]:
                    continue
                ok, ki, kr, cut = node_copies(c, shape, row, n, defect)
            if ok:
                add_node(r, n, ki, kr, cut, defect, row)
        out.append(r)
    return out


def compare(c, want, got):
    """Readable differences between two lists of rows (reference first)."""
    errs = []
    for si, (w, g) in enumerate(zip(want, got)):
        s = c.shapes[si]
        tag = f"shape {si} (cls {s['cls']}, best_effort {s['best_effort']}, req {s['req']}, limit {c.p['limit']})"
        errs += [f"{tag}: {k} is {g[k]}, reference {w[k]}" for k in KEYS if w[k] != g[k]]
    if len(want) != len(got):
        errs.append(f"{len(got)} rows, reference {len(want)}")
    return errs
