"""Seeded cases of kbg_node_why_kernel and their flat layout for the probe
(kbg_tool_probe_node_why). The node tables, planes and requests are those of
tests/task_why_cases.py's builders (by import); each shape becomes a record with
a weight, the part of it in queues that are not overused and a first task, and
each case names the words it asks for. The cases sit on the kernel's
boundaries: tables of 1, 63, 64, 65, 127-129 and 1023-1025 nodes (a wave owns
a 64-node word, a workgroup four list entries), shards whose table starts at
node 64 and 128, shape counts of 1, a group less one, a group, a group plus one
and two groups plus one (GROUP records share a workgroup; more than one group
meets in the output through atomics), word lists of every word, only the
first, only the last (ragged) word, two non-adjacent words and one word of a
1025-node table, garbage plane bits past the last node, dead nodes that would
fail each stage, cap_check 0, nodes at and one below their pod cap, BestEffort
shapes, zero request dimensions, the LessEqual tolerance edges against Idle and
Releasing in each dimension, weights of 1 and of 100000, weight_open of 0 and
of the whole weight, two shapes under one cause with their first tasks in
either order, and a node that meets every device cause across its shapes."""
import functools

import numpy as np

import node_why_ref as nr
import task_why_cases as tc
import task_why_ref as tr
from kernel_ref import GUARD_BYTES, SENTINEL

GROUP = nr.GROUP
MI = tc.MI
DEVICE_CAUSES = (0, 1, 3, 4, 6, 7, 8)  # kNodeWhyCause: the order of the count and first_task planes
N_FIELDS = 2 * len(DEVICE_CAUSES) + 6  # kNodeWhyFields
NODE_SHAPE = np.dtype([("cls", "<i4"), ("flags", "<i4"), ("req", "<f8", (3,)), ("weight", "<i4"), ("weight_open", "<i4"),
                       ("first_task", "<i4"), ("pad", "<i4")])
assert NODE_SHAPE.itemsize == 48
FIELDS = ("n_nodes", "W", "tab_lo", "tab_n", "stride", "classes", "n_shapes", "cap_check", "n_words", "ostride")
BIG = 100000


def finish(c, seed, words=None, pad=5):
    """Weights and first tasks for the case's shapes (a seeded draw: shape 0
    weighs 1, the last BIG; weight_open is 0, the weight or in between; the
    first tasks are distinct and in no order), its word list and plane stride."""
    rng = np.random.default_rng(seed)
    first = rng.permutation(4 * len(c.shapes) + 3)
    for i, s in enumerate(c.shapes):
        w = 1 if i == 0 else BIG if i == len(c.shapes) - 1 else int(rng.integers(1, 40))
        s.setdefault("weight", w)
        s.setdefault("weight_open", int(rng.choice((0, s["weight"], rng.integers(0, s["weight"] + 1)))))
        s.setdefault("first_task", int(first[i]))
    tab_words = (c.p["tab_n"] + 63) // 64
    c.words = list(range(tab_words)) if words is None else [w % tab_words for w in words]
    c.p["n_words"] = len(c.words)
    c.p["ostride"] = 64 * len(c.words) + pad
    return c


def random_case(name, seed, n_nodes, n_shapes, words=None, pad=5, **kw):
    c = tc.random_case(name, seed, n_nodes, n_shapes, **kw)
    return finish(c, seed + 1, words, pad)


def every_cause_case():
    """130 nodes, three words, asked for words 0 and 2. The pod cap and the
    unschedulable flag are the node's alone, whatever the shape: node 3 (110
    of 110 pods; node 4 is one below) is under cause 0 and node 129, in the
    ragged word, under cause 3 for every shape. Node 10 meets every cause that
    depends on the shape across its nine shapes: 1, 4, 6, 7 and 8. Node 6 is
    dead and would fail each stage. Shapes 0 and 1 fit Idle everywhere with
    their first tasks descending (9, 4), shapes 2 and 3 with theirs ascending
    (11, 12); node 128 fits the large request on Releasing alone."""
    c = tc.blank("every-cause", 130, classes=4)
    big = [1000.0, 1024.0 * MI, 0.0]
    c.ntasks[3], c.maxtasks[3] = 110, 110
    c.ntasks[4], c.maxtasks[4] = 109, 110
    c.live[6] = False
    c.sel_ok[0][6] = c.taint_ok[0][6] = False
    c.unsched[6] = True
    c.ntasks[6], c.maxtasks[6] = 5, 5
    # node 10: class 1 fails the selector, class 2 the taints; Idle fits a small request only, Releasing a middle one
    c.sel_ok[1][10] = False
    c.taint_ok[2][10] = False
    c.idle[10] = [500.0, 512.0 * MI, 0.0]
    c.rel[10] = [1000.0, 1024.0 * MI, 0.0]
    c.unsched[129] = True  # the only unschedulable node: in the last (ragged) word
    c.idle[128], c.rel[128] = [0.0, 0.0, 0.0], list(big)
    for cls, req, be, first in ((0, [100.0, 100.0 * MI, 0.0], False, 9), (0, [200.0, 100.0 * MI, 0.0], False, 4),
                                (3, [100.0, 100.0 * MI, 0.0], False, 11), (3, [200.0, 100.0 * MI, 0.0], False, 12),
                                (1, big, False, 20), (2, big, False, 21), (0, big, False, 22),
                                (0, [4000.0, 1024.0 * MI, 0.0], False, 23), (0, [0.0, 0.0, 0.0], True, 2)):
        tc.shape(c, cls, req, be)
        c.shapes[-1]["first_task"] = first
    return finish(c, 7400, words=(0, 2))


def unschedulable_case():
    """Node 5 of 70 is unschedulable and dead node 7 would be: cause 3 for every shape on node 5 alone."""
    c = tc.blank("unschedulable", 70, classes=1)
    c.unsched[5] = c.unsched[7] = True
    c.live[7] = False
    tc.shape(c, 0, [100.0, 100.0 * MI, 0.0])
    tc.shape(c, 0, [0.0, 0.0, 0.0], best_effort=True)
    return finish(c, 7401)


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [random_case(f"n{n}-s{s}", 7500 + n + s, n, s) for n, s in
          ((1, 1), (63, GROUP - 1), (64, GROUP), (65, GROUP + 1), (127, 2), (128, 3), (129, GROUP + 1), (1023, 2),
           (1024, GROUP), (1025, 2 * GROUP + 1))]
    cs.append(random_case("n200-s5-cap0", 7601, 200, 5, cap_check=0))
    cs.append(random_case("shard64-93of200", 7602, 200, GROUP + 1, tab_lo=64, tab_n=93))
    cs.append(random_case("shard128-72of200", 7603, 200, 3, tab_lo=128, tab_n=72, words=(1,)))
    cs.append(random_case("shard128-1of300", 7604, 300, 2, tab_lo=128, tab_n=1))
    cs.append(random_case("n300-first-word", 7605, 300, 5, words=(0,)))
    cs.append(random_case("n300-last-word", 7606, 300, GROUP + 3, words=(4,)))  # 44 nodes of the ragged word
    cs.append(random_case("n600-words-1-7", 7607, 600, 4, words=(1, 7)))
    cs.append(random_case("n1025-word-16", 7608, 1025, 3, words=(16,), pad=0))   # the one node of the last word
    cs.append(random_case("n1025-word-9", 7609, 1025, 2 * GROUP + 1, words=(9,)))
    cs.append(finish(tc.edges_case(), 7610))
    cs.append(every_cause_case())
    cs.append(unschedulable_case())
    return {c.name: c for c in cs}


def case(name):
    return _cases()[name]


NAMES = list(_cases())


# ------------------------------------------------------------------ layout
planes_words = tc.planes_words
table_block = tc.table_block


def shape_records(c):
    s = np.zeros(len(c.shapes), dtype=NODE_SHAPE)
    for r, d in zip(s, c.shapes):
        r["cls"], r["flags"], r["req"] = d["cls"], int(d["best_effort"]), d["req"]
        r["weight"], r["weight_open"], r["first_task"] = d["weight"], d["weight_open"], d["first_task"]
    return s


def word_list(c):
    return np.array(c.words, dtype="<i4")


def _row_words(r):
    return ([r["count"][k] for k in DEVICE_CAUSES] + [r["first_task"][k] for k in DEVICE_CAUSES] + r["idle_short"] +
            [r["open_idle"], r["open_releasing"], r["idle_best_effort"]])


EMPTY = _row_words(nr.empty_row())


def out_bytes(c, rows_):
    """The probe's raw output for these rows: N_FIELDS planes of ostride words,
    the listed words' slots at their empty value or their row, the rest of a
    plane and the guard region after the planes still holding the sentinel."""
    P, nw = c.p["ostride"], len(c.words)
    planes = np.frombuffer(np.full(N_FIELDS * P * 4, SENTINEL, dtype=np.uint8).tobytes(), dtype="<i4").reshape(N_FIELDS, P).copy()
    planes[:, :64 * nw] = np.array(EMPTY, dtype="<i4")[:, None]
    for slot, r in rows_.items():
        planes[:, slot] = _row_words(r)
    return np.concatenate([np.frombuffer(planes.tobytes(), dtype=np.uint8), np.full(GUARD_BYTES, SENTINEL, dtype=np.uint8)])


def rows_of(c, raw):
    """({slot: row}, padding and guard untouched) of a probe's raw output. A
    slot holds a row when any of its words differs from the empty value (a
    live node's counts sum to the weights, never 0)."""
    P, nw = c.p["ostride"], len(c.words)
    planes = np.frombuffer(raw[:N_FIELDS * P * 4].tobytes(), dtype="<i4").reshape(N_FIELDS, P)
    nc = len(DEVICE_CAUSES)
    out = {}
    for slot in range(64 * nw):
        w = planes[:, slot].tolist()
        if w == EMPTY:
            continue
        r = nr.empty_row()
        for i, k in enumerate(DEVICE_CAUSES):
            r["count"][k], r["first_task"][k] = w[i], w[nc + i]
        r["idle_short"] = w[2 * nc:2 * nc + 3]
        r["open_idle"], r["open_releasing"], r["idle_best_effort"] = w[2 * nc + 3:]
        out[slot] = r
    pad = np.frombuffer(planes[:, 64 * nw:].tobytes(), dtype=np.uint8)
    return out, bool((pad == SENTINEL).all() and (raw[N_FIELDS * P * 4:] == SENTINEL).all())


def compare_raw(c, raw):
    """Differences between a probe's raw output and the reference: the rows, then every byte."""
    got, clean = rows_of(c, raw)
    want = nr.rows(c)
    errs = nr.compare(c, want, got)
    if not clean:
        errs.append("a plane's words past the listed slots, or the guard region after the planes, were overwritten")
    if not errs and not (raw == out_bytes(c, want)).all():
        errs.append("raw output differs from the reference's bytes")
    return errs


def run_probe(lib, c, ptr, params, p_over=None, mutate=None):
    """One kbg_tool_probe_node_why call on copies of the case's arrays: (rc, arrays as left, raw output)."""
    import ctypes
    lib.kbg_tool_probe_node_why.restype = ctypes.c_int32
    a = dict(block=table_block(c), planes=planes_words(c), shapes=shape_records(c), words=word_list(c))
    if mutate:
        mutate(a)
    p = dict(c.p, **(p_over or {}))
    raw = np.full(N_FIELDS * max(int(p["ostride"]), 0) * 4 + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    rc = lib.kbg_tool_probe_node_why(params(FIELDS, p), ptr(a["block"]), ptr(a["planes"]), ptr(a["shapes"]),
                                     ptr(a["words"]), ptr(raw))
    return rc, a, raw


def check_probe(lib, c, ptr, params):
    rc, a, raw = run_probe(lib, c, ptr, params)
    if rc != 0:
        return [f"probe returned {rc}: {lib.kbg_tool_probe_error()}"]
    errs = compare_raw(c, raw)
    if not (a["block"] == table_block(c)).all():
        errs.append("node table block changed")
    return errs


ILLEGAL_CASE = "n600-words-1-7"


def illegal_launches():
    """(id, parameter overrides, mutation, what the message names) of launches kbg_node_reasons never makes."""
    def setter(arr, field, i, v):
        def f(a):
            if field:
                a[arr][field][i] = v
            else:
                a[arr][i] = v
        return f

    def heavy(a):
        a["shapes"]["weight"][:] = 2 ** 30
        a["shapes"]["weight_open"][:] = 0
    return [("tab_lo", dict(tab_lo=32), None, "tab_lo"), ("range", dict(tab_n=0), None, "node range"),
            ("past-n", dict(tab_n=10 ** 6), None, "node range"), ("stride", dict(stride=5), None, "table block"),
            ("n_shapes0", dict(n_shapes=0), None, "n_shapes"), ("cls", None, setter("shapes", "cls", 1, 3), "cls"),
            ("weight0", None, setter("shapes", "weight", 2, 0), "weight below 1"),
            ("open-over", None, setter("shapes", "weight_open", 0, 2), "weight_open"),
            ("open-negative", None, setter("shapes", "weight_open", 0, -1), "weight_open"),
            ("first-negative", None, setter("shapes", "first_task", 1, -1), "first_task"),
            ("weights-overflow", None, heavy, "INT32_MAX"),
            ("words-unsorted", None, setter("words", None, slice(None), [7, 1]), "not ascending"),
            ("words-twice", None, setter("words", None, slice(None), [7, 7]), "not ascending"),
            ("words-past", None, setter("words", None, 1, 10), "outside the table"),
            ("words-negative", None, setter("words", None, 0, -1), "outside the table"),
            ("n_words0", dict(n_words=0), None, "n_words"), ("ostride", dict(ostride=127), None, "ostride")]


def check_illegal(lib, ptr, params, ident):
    _, over, mutate, what = next(x for x in illegal_launches() if x[0] == ident)
    rc, a, raw = run_probe(lib, case(ILLEGAL_CASE), ptr, params, over, mutate)
    msg = lib.kbg_tool_probe_error().decode()
    errs = []
    if rc != -2 or what not in msg:
        errs.append(f"expected -2 naming {what}: got {rc} {msg!r}")
    if not (raw == SENTINEL).all():
        errs.append("a rejected launch wrote its output")
    return errs
