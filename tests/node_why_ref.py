"""Plain reference of the node reasons (kbg_node_reasons; the contract of
kbg_node_why_kernel in kube-arbitrator_amd/csrc/kbg_device.hpp): per named node
and per Pending task, on lists and Python ints. A shape record stands for
`weight` tasks of one key, `weight_open` of them in a queue that is not
overused, the lowest of them task `first_task`. The cause of a (node, task)
pair is task_why_ref.cause, the per-pair function of the pending-task reference;
the walk and the sums here are this file's own (node-major, a dict per node).

A case `c` is a case of tests/task_why_ref.py with
  c.shapes    dicts cls, best_effort, req [3], weight, weight_open, first_task
  c.words     the listed words of the table (ascending, no repeats)
  c.p         also n_words and ostride (words of an output plane)
`rows(c)` gives {slot: row}: slot 64 * i + l is lane l of list entry i, present
for the live nodes inside the table only; a row holds count[10], first_task[10],
idle_short[3], open_idle, open_releasing, idle_best_effort.
`rows(c, defect)` restates one of DEFECTS, a mistake a kernel could make; the
comparator must report each (tests/test_node_why_ref.py)."""
import task_why_ref as tr

GROUP = 32  # kNodeWhyGroup
N_CAUSES = tr.N_CAUSES
DEFECTS = ("weight_ignored", "open_for_count", "min_over_shape_index", "dead_row", "ragged_counted", "last_group_only",
           "stage_swap", "releasing_first", "short_on_idle", "be_tested", "cap_without_check", "unnamed_word_written")
# the defects that are task_why_ref.cause's own
PAIR_DEFECTS = ("stage_swap", "releasing_first", "short_on_idle", "be_tested")


def empty_row():
    return dict(count=[0] * N_CAUSES, first_task=[-1] * N_CAUSES, idle_short=[0, 0, 0], open_idle=0, open_releasing=0,
                idle_best_effort=0)


def pair(c, shape, row, n, defect=None):
    """(cause, [cpu, memory, GPU short]) of one task of `shape` on table row `row`, global node n."""
    if defect == "cap_without_check" and not c.p["cap_check"] and c.ntasks[row] >= c.maxtasks[row]:
        return tr.POD_CAP, [False] * 3
    return tr.cause(c, shape, row, n, defect if defect in PAIR_DEFECTS else None)


def node_row(c, row, n, defect=None):
    """The row of one node: every shape's tasks under their cause."""
    r = empty_row()
    shapes = list(enumerate(c.shapes))
    if defect == "last_group_only":
        shapes = shapes[(len(shapes) - 1) // GROUP * GROUP:]
    for si, s in shapes:
        k, short = pair(c, s, row, n, defect)
        tasks = 1 if defect == "weight_ignored" else s["weight_open"] if defect == "open_for_count" else s["weight"]
        first = si if defect == "min_over_shape_index" else s["first_task"]
        r["count"][k] += tasks
        if r["first_task"][k] < 0 or first < r["first_task"][k]:
            r["first_task"][k] = first
        for d in range(3):
            if short[d]:
                r["idle_short"][d] += s["weight"]
        if k == tr.FITS_IDLE:
            r["open_idle"] += s["weight_open"]
            if s["best_effort"]:
                r["idle_best_effort"] += s["weight"]
        elif k == tr.FITS_RELEASING:
            r["open_releasing"] += s["weight_open"]
    return r


def rows(c, defect=None):
    lo, nn, N = c.p["tab_lo"], c.p["tab_n"], c.p["n_nodes"]
    out = {}
    entries = list(enumerate(c.words))
    if defect == "unnamed_word_written":  # every word of the table, at the slots of its word number
        entries = [(w, w) for w in range((nn + 63) // 64)]
    for i, w in entries:
        for lane in range(64):
            row, slot = 64 * w + lane, 64 * i + lane
            if slot >= c.p["ostride"]:
                continue
            n = lo + row
            if row >= nn:  # (the planes hold ones there; the lane reads the table's last row)
                if defect == "ragged_counted":
                    out[slot] = node_row(c, nn - 1, min(n, N - 1), defect)
                continue
            if not c.live[n] and defect != "dead_row":
                continue
            out[slot] = node_row(c, row, n, defect)
    return out


def compare(c, want, got):
    """Readable differences between two {slot: row} (reference first)."""
    errs = []
    for slot in sorted(set(want) | set(got)):
        tag = f"slot {slot}"
        if slot // 64 < len(c.words):
            tag += f" (node {c.p['tab_lo'] + 64 * c.words[slot // 64] + slot % 64})"
        if slot not in want or slot not in got:
            errs.append(f"{tag}: a row {'is missing' if slot in want else 'was written where the reference has none'}")
            continue
        w, g = want[slot], got[slot]
        for k in range(N_CAUSES):
            for f in ("count", "first_task"):
                if w[f][k] != g[f][k]:
                    errs.append(f"{tag}: {f}[{tr.CAUSE_NAMES[k]}] is {g[f][k]}, reference {w[f][k]}")
        for d, name in enumerate(("cpu", "memory", "GPU")):
            if w["idle_short"][d] != g["idle_short"][d]:
                errs.append(f"{tag}: idle_short[{name}] is {g['idle_short'][d]}, reference {w['idle_short'][d]}")
        for f in ("open_idle", "open_releasing", "idle_best_effort"):
            if w[f] != g[f]:
                errs.append(f"{tag}: {f} is {g[f]}, reference {w[f]}")
    return errs
