"""Seeded and hand-made cases of kbg_drain_kernel and their flat layout for the
probe (kbg_tool_probe_drain), at the smallest sizes where the kernel can go
wrong: tables of 1, 63, 64, 65, 130, 257 and 600 nodes (a lane per node of a
64-node word), shards of 93 of 200 nodes from node 64 and of 1 of 300 from node
128, launches of 1, 2, 5 and 70 walks (a wave and a workgroup per walk), walks
of 1, 2, 7, 64, 65 and 512 steps (the overlay is looked through 64 entries at
a time and holds 512), the drained node at lane 0, at lane 63, at lane 0 of
word 1, in the ragged last word, the only node of the table and outside the
table range, cordons that are empty, one bit in another word, a whole word and
the node the first fit would have been, cap_check 0 and 1, dead nodes and rows
past tab_n holding garbage, garbage plane bits past the last node, BestEffort
steps, and hand-worked walks (`claims`: walk -> [(node, kind)], written by
hand).

The table block, the planes and the shape records are laid out as
tests/task_why_cases.py lays them out (the kernels read the same data); the
steps as tests/job_fit_cases.py lays them out."""
import functools

import numpy as np

import drain_ref as dr
from headroom_cases import BIG, garbage, multiple
from job_fit_cases import STEP
from kernel_ref import GUARD_BYTES, SENTINEL
from task_why_cases import CPU, GPU, MEM, MI, blank as _blank, planes_words, shape, shape_records, table_block

FIELDS = ("n_nodes", "W", "tab_lo", "tab_n", "stride", "classes", "n_shapes", "cap_check", "n_walks", "n_steps")
G = 1024.0 * MI
A, P = dr.ALLOCATE, dr.PIPELINE
NOWHERE = (-1, 0)


def blank(name, n_nodes, **kw):
    c = _blank(name, n_nodes, **kw)
    c.walks, c.drain, c.cordon, c.claims = [], [], set(), {}
    return c


def drain(c, node, steps, claim=None):
    """One walk: `node` (global, -1 none) takes nothing in it."""
    c.walks.append([int(s) for s in steps])
    c.drain.append(int(node))
    if claim is not None:
        c.claims[len(c.walks) - 1] = list(claim)


def random_case(name, seed, n_nodes, walk_lens, drains, cordon=(), n_shapes=6, tab_lo=0, tab_n=None, cap_check=1,
                classes=3):
    """`drains`: the drained node of each walk (global; None: a random live node of the table)."""
    rng = np.random.default_rng(seed)
    c = blank(name, n_nodes, tab_lo=tab_lo, tab_n=tab_n, classes=classes, cap_check=cap_check)
    c.live = (rng.random(n_nodes) >= 0.1).tolist()
    nn = c.p["tab_n"]
    named = {d for d in drains if d is not None and tab_lo <= d < tab_lo + nn}
    for d in named:
        c.live[d] = True
    for row in range(c.p["stride"]):
        c.idle[row] = [multiple(rng, CPU, 0), multiple(rng, MEM, 1), multiple(rng, GPU, 2)]
        if rng.random() < 0.4:
            c.rel[row] = [multiple(rng, CPU, 0), multiple(rng, MEM, 1), multiple(rng, GPU, 2)]
        c.maxtasks[row] = int(rng.choice((2, 8, 110)))
        c.ntasks[row] = int(rng.choice((0, 1, c.maxtasks[row] - 1, c.maxtasks[row], c.maxtasks[row] + 1),
                                       p=(0.3, 0.3, 0.15, 0.15, 0.1)))
        if rng.random() < 0.15:  # an Idle that drifted below zero: only a BestEffort pod, which gets no test, lands
            c.idle[row][0] = -25.0
        n = tab_lo + row
        if row >= nn or (n < n_nodes and not c.live[n]):  # values no lane may use
            c.idle[row], c.rel[row] = garbage(rng), garbage(rng)
            c.ntasks[row], c.maxtasks[row] = int(rng.integers(-2 ** 31, 2 ** 31)), int(rng.integers(-2 ** 31, 2 ** 31))
    c.unsched = (rng.random(n_nodes) < 0.1).tolist()
    c.sel_ok = (rng.random((classes, n_nodes)) < 0.8).tolist()
    c.taint_ok = (rng.random((classes, n_nodes)) < 0.85).tolist()
    for d in named:  # a drained node is a good node: leaving it in shows
        r = d - tab_lo
        c.idle[r], c.ntasks[r], c.maxtasks[r], c.unsched[d] = [64000.0, 512 * G, 16000.0], 1, 3, False
        for k in range(classes):
            c.sel_ok[k][d] = c.taint_ok[k][d] = True
    for i in range(n_shapes):  # shape 1 BestEffort, shape 2 without a GPU request
        if i == 1:
            shape(c, rng.integers(0, classes), (0.0, 0.0, 0.0), best_effort=True)
        else:
            shape(c, rng.integers(0, classes), (rng.choice(CPU), rng.choice(MEM), 0.0 if i == 2 else rng.choice(GPU)))
    c.cordon = set(int(n) for n in cordon)
    live = [n for n in range(tab_lo, tab_lo + nn) if c.live[n]]
    for ln, d in zip(walk_lens, drains):  # the pods of a node: of any mix of shapes
        if d is None:
            d = int(rng.choice(live)) if live else -1
        drain(c, d, [int(rng.integers(0, n_shapes)) for _ in range(ln)])
    return c


def empty(name, n_nodes, **kw):
    """Every node with nothing Idle or Releasing and a pod room no walk fills."""
    c = blank(name, n_nodes, **kw)
    for row in range(c.p["stride"]):
        c.idle[row], c.rel[row], c.ntasks[row], c.maxtasks[row] = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0, BIG
    return c


def hand_cases():
    """The hand-worked walks. R asks for 1000m / 1Gi, H for 500m / 512Mi, B is BestEffort."""
    R, H, B = [1000.0, G, 0.0], [500.0, G / 2, 0.0], [0.0, 0.0, 0.0]
    big = [9000.0, 64 * G, 0.0]
    out = []

    c = empty("drained-is-the-lowest-fit", 3, classes=1)
    c.idle[0], c.idle[1], c.idle[2] = list(big), list(R), list(big)
    shape(c, 0, R)
    drain(c, 0, [0, 0], [(1, A), (2, A)])  # node 0 would take both
    out.append(c)

    c = empty("releasing-before-the-next-node", 4, classes=1)
    c.idle[0], c.idle[1], c.rel[1], c.idle[2] = list(big), list(R), list(R), [5000.0, 8 * G, 0.0]
    shape(c, 0, R)
    drain(c, 0, [0, 0, 0], [(1, A), (1, P), (2, A)])  # node 1's Releasing before node 2's Idle
    out.append(c)

    c = empty("best-effort-where-a-request-cannot", 4, classes=1)
    c.idle[0], c.idle[3] = list(big), list(R)  # node 2 has nothing
    c.idle[1] = [-20.0, 0.0, 0.0]  # below zero by more than LessEqual's tolerance: even an empty request fails it
    shape(c, 0, R)
    shape(c, 0, B, best_effort=True)
    drain(c, 0, [1, 0, 1], [(1, A), (3, A), (1, A)])  # no resource test for B: the first node past the stages
    out.append(c)

    c = empty("best-effort-fills-the-last-pod-slot", 3, classes=1)
    c.idle[0], c.idle[1], c.idle[2] = list(big), list(big), list(big)
    c.ntasks[1], c.maxtasks[1] = 109, 110
    shape(c, 0, R)
    shape(c, 0, B, best_effort=True)
    drain(c, 0, [1, 1, 0], [(1, A), (2, A), (2, A)])  # B takes node 1's last slot: the next B and R go past it
    out.append(c)

    c = empty("unplaced-then-smaller", 3, classes=1)
    c.idle[0], c.idle[1] = list(big), [500.0, G, 0.0]
    shape(c, 0, R)
    shape(c, 0, H)
    drain(c, 0, [0, 1, 0], [NOWHERE, (1, A), NOWHERE])  # the walk goes on; R's prev landed nowhere, so does R
    out.append(c)

    c = empty("back-to-a-touched-word", 130, classes=1)
    c.idle[0], c.idle[5], c.idle[70] = list(big), [1500.0, 2 * G, 0.0], list(R)
    shape(c, 0, R)
    shape(c, 0, H)
    drain(c, 0, [0, 1, 0], [(5, A), (5, A), (70, A)])  # H leaves node 5 at 0m / 512Mi: R's cursor node no longer fits
    out.append(c)

    c = empty("tolerance-once", 3, classes=1, cap_check=0)
    c.idle[0], c.idle[1] = list(big), [3.0, 8192.0 * MI, 0.0]
    shape(c, 0, [8.0, 64.0 * MI, 0.0])
    drain(c, 0, [0, 0], [(1, A), NOWHERE])  # |3 - 8| < 10 fits and leaves -5; |-5 - 8| = 13 does not
    out.append(c)

    c = empty("cordon-takes-the-first-fit", 70, classes=1)
    c.idle[0], c.idle[1], c.idle[65] = list(big), list(big), list(R)
    c.cordon = {1}
    shape(c, 0, R)
    drain(c, 0, [0, 0], [(65, A), NOWHERE])  # node 1 would take both; the next fit is in the other word
    out.append(c)

    c = empty("exclusion-is-per-walk", 3, classes=1)
    c.idle[0], c.idle[1], c.idle[2] = list(R), list(R), list(R)
    shape(c, 0, R)
    drain(c, 0, [0, 0], [(1, A), (2, A)])
    drain(c, 1, [0, 0], [(0, A), (2, A)])  # node 0 is back, and node 1's and 2's Idle with it
    out.append(c)

    c = empty("cursor-is-per-walk", 4, classes=1)
    c.idle[0], c.idle[2], c.idle[3] = list(R), list(R), list(R)
    shape(c, 0, R)
    drain(c, 0, [0], [(2, A)])
    drain(c, 2, [0, 0], [(0, A), (3, A)])  # from the table's first node again
    out.append(c)

    c = empty("shard-70-of-200", 200, tab_lo=64, tab_n=70, classes=1, stride=70)
    c.idle[3], c.idle[6], c.idle[69] = list(R), list(R), list(R)  # nodes 67, 70 and 133, the table's last row
    shape(c, 0, R)
    drain(c, 67, [0, 0, 0], [(70, A), (133, A), NOWHERE])  # global indices; row 3 takes nothing
    drain(c, 3, [0, 0, 0], [(67, A), (70, A), (133, A)])   # node 3 is below the range: nothing is excluded
    drain(c, 150, [0, 0], [(67, A), (70, A)])              # node 150 is above it
    drain(c, -1, [0], [(67, A)])
    out.append(c)

    c = empty("cap-check-off-still-excludes", 4, classes=1, cap_check=0)
    c.idle[0], c.idle[1], c.idle[2] = list(big), list(big), list(R)
    c.cordon = {1}
    shape(c, 0, R)
    shape(c, 0, B, best_effort=True)
    drain(c, 0, [0, 1, 0], [(2, A), (2, A), NOWHERE])  # B: the first live node that is not excluded
    out.append(c)

    c = empty("the-only-node", 1, classes=1)
    c.idle[0] = list(big)
    shape(c, 0, R)
    shape(c, 0, B, best_effort=True)
    drain(c, 0, [0, 1, 0], [NOWHERE, NOWHERE, NOWHERE])
    out.append(c)

    c = empty("whole-word-cordoned", 130, classes=1)
    for n in range(130):
        c.idle[n] = list(R)
    c.cordon = set(range(64, 128))
    shape(c, 0, R)
    drain(c, 63, [0] * 66, [(n, A) for n in list(range(63)) + [128, 129]] + [NOWHERE])
    out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [random_case("n1-w1", 12001, 1, (3,), (0,)),
          random_case("n63-w2", 12063, 63, (2, 7), (0, 62)),
          random_case("n64-w5", 12064, 64, (7,) * 5, (0, 63, None, None, 63)),
          random_case("n65-w2", 12065, 65, (64, 65), (64, 63), cordon=(0,)),
          random_case("n130-w5", 12130, 130, (1, 2, 7, 64, 65), (0, 63, 64, 129, 128), cordon=(70,)),
          random_case("n257-w70", 12257, 257, (7,) * 70, (None,) * 68 + (256, 0), cordon=range(64, 128)),
          random_case("n600-w2", 12600, 600, (512, 65), (0, 599), cordon=(1, 2, 64, 599)),
          random_case("n200-w5-cap0", 12301, 200, (7, 64, 2, 65, 1), (0, 63, 64, 199, None), cordon=(5, 130),
                      cap_check=0),
          random_case("shard64-93of200", 12303, 200, (64, 7, 7, 7), (64, 156, 10, 180), cordon=(3, 65, 190),
                      tab_lo=64, tab_n=93),
          random_case("shard128-1of300", 12315, 300, (2, 1), (128, 5), tab_lo=128, tab_n=1)]
    return {c.name: c for c in cs + hand_cases()}


def case(name):
    return _cases()[name]


NAMES = list(_cases())
HAND = [c.name for c in hand_cases()]
SEEDED = [n for n in NAMES if n not in HAND]


# ------------------------------------------------------------------ layout
def step_records(c):
    recs = np.zeros(sum(len(w) for w in c.walks), dtype=STEP)
    k = 0
    for w in c.walks:
        for s, p in zip(w, dr.links(c, w)):
            recs[k] = (s, p)
            k += 1
    return recs


def walk_offsets(c):
    return np.cumsum([0] + [len(w) for w in c.walks]).astype("<i4")


def walk_rows(c):
    """Per walk the table row of its drained node; -1 for none and for a node below the table."""
    return np.array([max(-1, d - c.p["tab_lo"]) if d >= 0 else -1 for d in c.drain], dtype="<i4")


def excl_words(c):
    """The cordon as one plane of W words; the bits past n_nodes are garbage (ones)."""
    n, W = c.p["n_nodes"], c.p["W"]
    bits = np.ones(W * 64, dtype=bool)
    bits[:n] = False
    for x in c.cordon:
        bits[x] = True
    return np.packbits(bits.reshape(W, 64), axis=1, bitorder="little").view("<u8").reshape(-1).copy()


def out_bytes(walks_, defect=None):
    """The probe's raw output for these walks, then the guard region still holding the sentinel."""
    w = np.array([v for wk in walks_ for pl in wk for v in pl], dtype=np.int32)
    guard = np.full(GUARD_BYTES, SENTINEL, dtype=np.uint8)
    if defect == "guard_written":
        guard[:8] = 0  # one step too many
    return np.concatenate([np.frombuffer(w.tobytes(), dtype=np.uint8), guard])


def walks_of(c, raw):
    """(walks, guard untouched) of a probe's raw output."""
    n = sum(len(w) for w in c.walks)
    w = np.frombuffer(raw[:n * 8].tobytes(), dtype=np.int32).reshape(n, 2).tolist()
    out, k = [], 0
    for wk in c.walks:
        out.append([tuple(p) for p in w[k:k + len(wk)]])
        k += len(wk)
    return out, bool((raw[n * 8:] == SENTINEL).all())


def compare_raw(c, raw):
    """Differences between a probe's raw output and the reference: the walks, then every byte."""
    got, clean = walks_of(c, raw)
    want = dr.walks(c)
    errs = dr.compare(c, want, got)
    if not clean:
        errs.append("the guard region after the places was overwritten")
    if not errs and not (raw == out_bytes(want)).all():
        errs.append("raw output differs from the reference's bytes")
    return errs


def run_probe(lib, c, ptr, params, p_over=None, mutate=None):
    """One kbg_tool_probe_drain call on copies of the case's arrays: (rc, arrays as left, raw output)."""
    import ctypes
    lib.kbg_tool_probe_drain.restype = ctypes.c_int32
    a = dict(block=table_block(c), planes=planes_words(c), shapes=shape_records(c), steps=step_records(c),
             off=walk_offsets(c), excl=excl_words(c), rows=walk_rows(c))
    if mutate:
        mutate(a)
    p = {**c.p, "n_walks": len(a["off"]) - 1, "n_steps": len(a["steps"]), **(p_over or {})}
    raw = np.full(len(a["steps"]) * 8 + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    opt = lambda x: ptr(x) if x is not None else None  # noqa: E731
    rc = lib.kbg_tool_probe_drain(params(FIELDS, p), ptr(a["block"]), opt(a["planes"]), ptr(a["shapes"]),
                                  ptr(a["steps"]), ptr(a["off"]), opt(a["excl"]), ptr(a["rows"]), ptr(raw))
    return rc, a, raw


def check_probe(lib, c, ptr, params):
    rc, a, raw = run_probe(lib, c, ptr, params)
    if rc != 0:
        return [f"probe returned {rc}: {lib.kbg_tool_probe_error()}"]
    errs = compare_raw(c, raw)
    if not (a["block"] == table_block(c)).all():
        errs.append("node table block changed")
    if not (a["planes"] == planes_words(c)).all():
        errs.append("stage planes changed")
    return errs


def illegal_launches():
    """(id, parameter overrides, mutation, what the message names) of launches kbg_node_drain never makes."""
    def shape_index(a):
        a["steps"]["shape"][3] = len(a["shapes"])

    def prev_later(a):
        a["steps"]["prev"][2] = 2

    def prev_other_shape(a):
        s = a["steps"]
        k = next(i for i in range(1, 64) if s["shape"][i] != s["shape"][0])
        s["prev"][k] = 0

    def prev_other_walk(a):  # the second walk's first step naming a step of the first
        a["steps"]["prev"][64] = 3

    def steps_513(a):
        a["steps"] = np.zeros(513, dtype=STEP)
        a["steps"]["prev"] = -1
        a["off"] = np.array([0, 513], dtype="<i4")
        a["rows"] = np.array([0], dtype="<i4")

    def row_below(a):
        a["rows"][1] = -2

    def no_planes(a):
        a["planes"] = None

    def no_excl(a):
        a["excl"] = None
    return [("tab_lo", dict(tab_lo=32), None, "tab_lo"), ("range", dict(tab_n=0), None, "node range"),
            ("past-n", dict(tab_n=10 ** 6), None, "node range"), ("stride", dict(stride=5), None, "table block"),
            ("planes", None, no_planes, "null planes"), ("excl", None, no_excl, "null argument"),
            ("shape-index", None, shape_index, "shape index"), ("prev-later", None, prev_later, "prev"),
            ("prev-other-shape", None, prev_other_shape, "prev"), ("prev-other-walk", None, prev_other_walk, "prev"),
            ("steps-513", None, steps_513, "more than 512 steps"), ("row-below", None, row_below, "drained row"),
            ("walks", dict(n_walks=(1 << 20) + 1), None, "n_walks"),
            # 2^20 + 1 nodes in the table: one word more than the bitmap holds (refused before any array is read)
            ("bitmap", dict(n_nodes=(1 << 20) + 64, W=(1 << 14) + 1, tab_lo=0, tab_n=(1 << 20) + 1,
                            stride=(1 << 20) + 1), None, "bitmap")]


def check_illegal(lib, ptr, params, ident):
    _, over, mutate, what = next(x for x in illegal_launches() if x[0] == ident)
    rc, a, raw = run_probe(lib, case("shard64-93of200"), ptr, params, over, mutate)
    msg = lib.kbg_tool_probe_error().decode()
    errs = []
    if rc != -2 or what not in msg:
        errs.append(f"expected -2 naming {what}: got {rc} {msg!r}")
    if not (raw == SENTINEL).all():
        errs.append("a rejected launch wrote its output")
    return errs
