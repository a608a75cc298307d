"""Seeded and hand-made cases of kbg_task_headroom_kernel and their flat layout
for the probe (kbg_tool_probe_task_headroom), at the smallest sizes where the
kernel can go wrong: tables of 1, 63, 64, 65, 70, 256, 257 and 330 nodes (a
wave owns a 64-node word, a workgroup four of them: one wave, a ragged word,
one workgroup, one workgroup and a word), shards whose table starts at node 64
and 128, shape counts of 1, a group, a group plus one and two groups plus one
(GROUP shapes share a workgroup), limits of 1, 2, 7 and 1024, dead nodes
holding garbage, garbage plane bits past the last node, cap_check 0 and 1,
nodes at their pod cap, BestEffort shapes, a class failing each stage, and
hand-made nodes (`claims`: node -> (k_idle, k_rel, cut), worked by hand) whose
loops end by each dimension, by the pod room, by the limit below and at the
room, with Releasing taken after Idle inside one room, with Releasing zero, on
the LessEqual tolerance and with non-integer values where the iterated
subtraction and a - k * req disagree.

The table block, the planes and the shape records are laid out as
tests/task_why_cases.py lays them out (the two kernels read the same data)."""
import functools

import numpy as np

import headroom_ref as hr
from kernel_ref import GUARD_BYTES, SENTINEL
from task_why_cases import CPU, EDGES, GPU, MEM, MI, blank as _blank, planes_words, shape, shape_records, table_block

GROUP = 16                  # kTaskWhyGroup
OUT_WORDS = len(hr.KEYS)    # kRoomOut: no padding word
FIELDS = ("n_nodes", "W", "tab_lo", "tab_n", "stride", "classes", "n_shapes", "cap_check", "limit")
BIG = 1 << 20               # a pod cap no limit reaches


def blank(name, n_nodes, limit, **kw):
    c = _blank(name, n_nodes, **kw)
    c.p["limit"] = limit
    c.claims = {}
    return c


def multiple(rng, values, d):
    """A node value holding zero to six copies of one of the requests of
    dimension d, on or around a LessEqual bound."""
    if rng.random() < 0.1:
        return 0.0
    k = int(rng.integers(0, 7))
    return float(max(0.0, k * values[int(rng.integers(0, 3))] + EDGES[int(rng.integers(0, len(EDGES)))] * hr.MIN[d]))


def garbage(rng):
    """What a dead node's row may hold: nothing a live lane may count."""
    return [float(rng.choice((-1e300, 1e300, 7e9, -3.5))) for _ in range(3)]


def random_case(name, seed, n_nodes, n_shapes, limit, tab_lo=0, tab_n=None, cap_check=1, classes=3):
    rng = np.random.default_rng(seed)
    c = blank(name, n_nodes, limit, tab_lo=tab_lo, tab_n=tab_n, classes=classes, cap_check=cap_check)
    c.live = (rng.random(n_nodes) >= 0.1).tolist()
    for row in range(c.p["stride"]):  # (rows past tab_n: values no lane may count)
        c.idle[row] = [multiple(rng, CPU, 0), multiple(rng, MEM, 1), multiple(rng, GPU, 2)]
        if rng.random() < 0.4:
            c.rel[row] = [multiple(rng, CPU, 0), multiple(rng, MEM, 1), multiple(rng, GPU, 2)]
        c.maxtasks[row] = int(rng.choice((2, 8, 110)))
        c.ntasks[row] = int(rng.choice((0, 1, c.maxtasks[row] - 1, c.maxtasks[row], c.maxtasks[row] + 1),
                                       p=(0.3, 0.3, 0.15, 0.15, 0.1)))
        n = tab_lo + row
        if n < n_nodes and not c.live[n]:
            c.idle[row], c.rel[row] = garbage(rng), garbage(rng)
            c.ntasks[row], c.maxtasks[row] = int(rng.integers(-2 ** 31, 2 ** 31)), int(rng.integers(-2 ** 31, 2 ** 31))
    c.unsched = (rng.random(n_nodes) < 0.1).tolist()
    c.sel_ok = (rng.random((classes, n_nodes)) < 0.8).tolist()
    c.taint_ok = (rng.random((classes, n_nodes)) < 0.85).tolist()
    for i in range(n_shapes):  # with three or more: shape 1 BestEffort, shape 2 without a GPU request
        be = rng.random() < 0.15 or (i == 1 and n_shapes >= 3)
        gpu = 0.0 if i == 2 else rng.choice(GPU)
        req = (5.0, MI, 0.0) if be else (rng.choice(CPU), rng.choice(MEM), gpu)  # (BestEffort: IsEmpty, not zero)
        shape(c, rng.integers(0, classes), req, be)
    return c


def loop_ends_case(limit=7):
    """One hand-made node per way a loop ends, request (1000, 1 Gi, 1000),
    limit 7; `claims` holds each node's hand-worked (k_idle, k_rel, cut).
    Node 63 is the first word's last lane, node 64 the second word's first."""
    c = blank(f"loop-ends-l{limit}", 70, limit, classes=2)
    G = 1024.0 * MI
    req = [1000.0, G, 1000.0]

    def node(n, idle, rel, nt, mt, claim):
        c.idle[n], c.rel[n], c.ntasks[n], c.maxtasks[n] = list(idle), list(rel), nt, mt
        if limit == 7:
            c.claims[n] = claim

    Z = (0.0, 0.0, 0.0)
    node(0, (3000.0, 64 * G, 9000.0), Z, 0, BIG, (3, 0, False))      # ends by cpu
    node(1, (9000.0, 2 * G, 9000.0), Z, 0, BIG, (2, 0, False))       # ends by memory
    node(2, (9000.0, 64 * G, 4000.0), Z, 0, BIG, (4, 0, False))      # ends by GPU
    node(3, (9000.0, 64 * G, 9000.0), Z, 105, 110, (5, 0, False))    # ends by the pod room (5 < limit)
    node(4, (9000.0, 64 * G, 9000.0), Z, 0, BIG, (7, 0, True))       # ends by the limit, limit < room
    node(5, (9000.0, 64 * G, 9000.0), Z, 103, 110, (7, 0, False))    # ends by the limit, limit == room
    node(6, (2000.0, 64 * G, 9000.0), (2000.0, 64 * G, 9000.0), 0, BIG, (2, 2, False))   # Releasing after Idle
    node(7, (2000.0, 64 * G, 9000.0), (9000.0, 64 * G, 9000.0), 107, 110, (2, 1, False))  # the room shared: 3
    node(8, (5000.0, 64 * G, 9000.0), (9000.0, 64 * G, 9000.0), 0, BIG, (5, 2, True))    # the limit shared: 5 + 2
    node(9, Z, (3000.0, 64 * G, 9000.0), 0, BIG, (0, 3, False))      # Releasing only
    node(10, Z, Z, 0, BIG, (0, 0, False))                            # nothing, Releasing zero
    node(11, (9000.0, 64 * G, 9000.0), Z, 110, 110, None)            # at its pod cap: not past the stages
    node(63, (1000.0, 64 * G, 9000.0), Z, 0, BIG, (1, 0, False))     # a word's last lane
    node(64, (6000.0, 64 * G, 9000.0), Z, 0, BIG, (6, 0, False))     # the next word's first: the largest below the limit
    for n in range(12, 63):
        c.idle[n] = [0.0, 0.0, 0.0]
    for n in range(65, 70):
        c.idle[n] = [0.0, 0.0, 0.0]
    c.unsched[69] = True
    c.idle[69] = [9000.0, 64 * G, 9000.0]
    shape(c, 0, req)
    shape(c, 1, req)
    shape(c, 0, [5.0, 0.0, 0.0], best_effort=True)  # (IsEmpty: every dimension below its min; a resource test would end it)
    shape(c, 0, [3000.0, G, 1000.0])  # node 8 holds the most, 1 from Idle and 3 from Releasing; Idle alone gives 3 at most
    c.sel_ok[1][0] = False    # class 1 fails each stage on one node that holds copies for class 0
    c.taint_ok[1][1] = False
    return c


def tolerance_case():
    """LessEqual's tolerance inside the loops (cap_check 0: no pod room).
    Shape 0 asks for (8, 64 Mi, 0), shape 1 for (1000, 1 Gi, 0), shape 2 for
    (57.6, 64 Mi, 0), shape 3 for (46.3, 64 Mi, 0). `claims[(shape, node)]`."""
    c = blank("tolerance", 8, 1024, classes=1, cap_check=0)
    G = 1024.0 * MI
    for n in range(8):
        c.idle[n] = [0.0, 0.0, 0.0]
    # cpu 3 against 8 fits by tolerance (|3 - 8| < 10) and leaves Idle at -5; |-5 - 8| = 13 does not
    c.idle[0] = [3.0, 8192.0 * MI, 0.0]
    # a zero request dimension against a zero Idle dimension never ends the loop: cpu does, after 3
    c.idle[1] = [3000.0, 64 * G, 0.0]
    # a request exactly equal to Idle: one copy, then 0 against 1000
    c.idle[2] = [1000.0, G, 0.0]
    # non-integer: 450.8 - 7 * 57.6 and seven subtractions differ in the last place, on the bound of copy 8
    c.idle[3] = [450.8, 8192.0 * MI, 0.0]
    c.idle[4] = [221.5, 8192.0 * MI, 0.0]
    # Releasing on the tolerance after an Idle that holds nothing
    c.rel[5] = [3.0, 8192.0 * MI, 0.0]
    # one below and one on the tolerance's far side: 8 + 10 and 8 - 10
    c.idle[6] = [18.0, 8192.0 * MI, 0.0]
    c.idle[7] = [-2.0, 8192.0 * MI, 0.0]
    shape(c, 0, [8.0, 64.0 * MI, 0.0])
    shape(c, 0, [1000.0, G, 0.0])
    shape(c, 0, [57.6, 64.0 * MI, 0.0])
    shape(c, 0, [46.3, 64.0 * MI, 0.0])
    # shape 0: node 0: 3 -> -5: 1. node 1: 3000, 2992, ...: cpu r < a holds while a > 8, and on a in (-2, 18):
    # a = 3000 - 8 k fits for k <= 375 (a = 0 fits by tolerance; a = -8 does not): 376 copies, memory 64 Gi / 64 Mi
    # = 1024 is not the end. node 2: 1000 - 8 k >= 0 for k <= 125, a = 0 fits, -8 does not: 126, memory 1 Gi / 64 Mi
    # = 16 copies ends it first, the 17th on |0 - 64 Mi| >= 10 Mi: 16. node 6: 18 fits (r < a), 10 fits, 2 fits,
    # -6 does not (|-6 - 8| = 14): 3. node 7: |-2 - 8| = 10 is not < 10: 0.
    c.claims = {(0, 0): (1, 0), (0, 1): (376, 0), (0, 2): (16, 0), (0, 5): (0, 1), (0, 6): (3, 0), (0, 7): (0, 0),
                (1, 1): (3, 0), (1, 2): (1, 0), (1, 0): (0, 0),
                (2, 3): (7, 0), (3, 4): (4, 0)}
    return c


def product_copies(have, req, bound):
    """The copies a - k * req would give: what the iteration is NOT (tests only)."""
    k = 0
    while k < bound and hr.less_equal(req, [have[d] - k * req[d] for d in range(3)]):
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [random_case(f"n{n}-s{s}-l{lim}", 9000 + n + s, n, s, lim) for n, s, lim in
          ((1, 1, 1), (63, GROUP, 2), (64, GROUP + 1, 7), (65, 2 * GROUP + 1, 1024), (70, 1, 7), (256, 3, 1024),
           (257, GROUP + 1, 2), (330, 5, 1))]
    cs.append(random_case("n200-s5-cap0-l1024", 9301, 200, 5, 1024, cap_check=0))
    cs.append(random_case("n200-s4-cap0-l2", 9305, 200, 4, 2, cap_check=0))
    cs.append(random_case("shard64-93of200-l7", 9302, 200, GROUP + 1, 7, tab_lo=64, tab_n=93))
    cs.append(random_case("shard128-72of200-l1024", 9303, 200, 3, 1024, tab_lo=128, tab_n=72))
    cs.append(random_case("shard128-1of300-l2", 9304, 300, 2, 2, tab_lo=128, tab_n=1))
    cs.append(loop_ends_case())
    cs.append(loop_ends_case(limit=1))
    cs.append(tolerance_case())
    return {c.name: c for c in cs}


def case(name):
    return _cases()[name]


NAMES = list(_cases())


# ------------------------------------------------------------------ layout
def out_bytes(rows_):
    """The probe's raw output for these rows, then the guard region still holding the sentinel."""
    w = np.array([[r[k] for k in hr.KEYS] for r in rows_], dtype=np.int32)
    return np.concatenate([np.frombuffer(w.tobytes(), dtype=np.uint8), np.full(GUARD_BYTES, SENTINEL, dtype=np.uint8)])


def rows_of(c, raw):
    """(rows, guard untouched) of a probe's raw output."""
    ns = len(c.shapes)
    w = np.frombuffer(raw[:ns * OUT_WORDS * 4].tobytes(), dtype=np.int32).reshape(ns, OUT_WORDS)
    return [dict(zip(hr.KEYS, r.tolist())) for r in w], bool((raw[ns * OUT_WORDS * 4:] == SENTINEL).all())


def compare_raw(c, raw):
    """Differences between a probe's raw output and the reference: the rows, then every byte."""
    got, clean = rows_of(c, raw)
    want = hr.rows(c)
    errs = hr.compare(c, want, got)
    if not clean:
        errs.append("the guard region after the rows was overwritten")
    if not errs and not (raw == out_bytes(want)).all():
        errs.append("raw output differs from the reference's bytes")
    return errs


def run_probe(lib, c, ptr, params, p_over=None, mutate=None):
    """One kbg_tool_probe_task_headroom call on copies of the case's arrays: (rc, arrays as left, raw output)."""
    import ctypes
    lib.kbg_tool_probe_task_headroom.restype = ctypes.c_int32
    a = dict(block=table_block(c), planes=planes_words(c), shapes=shape_records(c))
    if mutate:
        mutate(a)
    p = dict(c.p, **(p_over or {}))
    raw = np.full(len(a["shapes"]) * OUT_WORDS * 4 + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    planes = ptr(a["planes"]) if a["planes"] is not None else None
    rc = lib.kbg_tool_probe_task_headroom(params(FIELDS, p), ptr(a["block"]), planes, ptr(a["shapes"]), ptr(raw))
    return rc, a, raw


def check_probe(lib, c, ptr, params):
    rc, a, raw = run_probe(lib, c, ptr, params)
    if rc != 0:
        return [f"probe returned {rc}: {lib.kbg_tool_probe_error()}"]
    errs = compare_raw(c, raw)
    if not (a["block"] == table_block(c)).all():
        errs.append("node table block changed")
    return errs


def illegal_launches():
    """(id, parameter overrides, mutation, what the message names) of launches kbg_task_headroom never makes."""
    def cls(a):
        a["shapes"]["cls"][1] = 3

    def no_planes(a):
        a["planes"] = None
    return [("tab_lo", dict(tab_lo=32), None, "tab_lo"), ("range", dict(tab_n=0), None, "node range"),
            ("past-n", dict(tab_n=10 ** 6), None, "node range"), ("stride", dict(stride=5), None, "table block"),
            ("n_shapes0", dict(n_shapes=0), None, "n_shapes"), ("cls", None, cls, "cls"),
            ("limit0", dict(limit=0), None, "limit"), ("limit1025", dict(limit=1025), None, "limit"),
            # 2^21 + 64 nodes of which the table holds 2^21 + 1: times 1024 past INT32_MAX (refused before any array is read)
            ("overflow", dict(n_nodes=(1 << 21) + 64, W=(1 << 15) + 1, tab_lo=0, tab_n=(1 << 21) + 1,
                              stride=(1 << 21) + 1, limit=1024), None, "overflows"),
            ("planes", None, no_planes, "null planes")]


def check_illegal(lib, ptr, params, ident):
    _, over, mutate, what = next(x for x in illegal_launches() if x[0] == ident)
    rc, a, raw = run_probe(lib, case("shard64-93of200-l7"), ptr, params, over, mutate)
    msg = lib.kbg_tool_probe_error().decode()
    errs = []
    if rc != -2 or what not in msg:
        errs.append(f"expected -2 naming {what}: got {rc} {msg!r}")
    if not (raw == SENTINEL).all():
        errs.append("a rejected launch wrote its output")
    return errs
