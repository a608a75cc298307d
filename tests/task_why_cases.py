"""Seeded cases of kbg_task_why_kernel and their flat layout for the probe
(kbg_tool_probe_task_why). The cases sit on the kernel's boundaries: tables of
1, 63, 64, 65, 127-129 and 1023-1025 nodes (a wave owns a 64-node word, a
workgroup four of them), shards whose table starts at node 64 and 128, shape
counts of 1, a group less one, a group and a group plus one (GROUP shapes share
a workgroup), garbage plane bits past the last node, dead nodes, cap_check 0,
nodes at and one below their pod cap, BestEffort shapes, zero request
dimensions, the LessEqual tolerance edges against Idle and Releasing in each
dimension, nodes that fit Releasing only, every cause at once and a cause whose
only node is in the last word."""
import functools
from types import SimpleNamespace

import numpy as np

import task_why_ref as tr
from kernel_ref import GUARD_BYTES, SENTINEL, pack_words

GROUP = 16                       # kTaskWhyGroup
OUT_WORDS = 2 * tr.N_CAUSES + 4  # kTaskWhyOut: count, first_node, idle_short, one word of padding
MI = float(1 << 20)
TASK_SHAPE = np.dtype([("cls", "<i4"), ("flags", "<i4"), ("req", "<f8", (3,))])
assert TASK_SHAPE.itemsize == 32
FIELDS = ("n_nodes", "W", "tab_lo", "tab_n", "stride", "classes", "n_shapes", "cap_check")

CPU = (300.0, 1000.0, 4000.0)
MEM = (300.0 * MI, 1024.0 * MI, 4096.0 * MI)
GPU = (0.0, 1000.0, 2000.0)
# offsets from a request that sit on both sides of each LessEqual bound, in units of the dimension's tolerance
EDGES = (0.0, -1.0, -0.999, -0.5, 0.5, 1.0, -1.001, 3.0)


def blank(name, n_nodes, tab_lo=0, tab_n=None, classes=3, cap_check=1, stride=None):
    tab_n = n_nodes - tab_lo if tab_n is None else tab_n
    stride = tab_n + 3 if stride is None else stride
    c = SimpleNamespace(name=name, shapes=[])
    c.p = dict(n_nodes=n_nodes, W=(n_nodes + 63) // 64, tab_lo=tab_lo, tab_n=tab_n, stride=stride, classes=classes,
               n_shapes=0, cap_check=cap_check)
    c.idle = [[8000.0, 8192.0 * MI, 4000.0] for _ in range(stride)]
    c.rel = [[0.0, 0.0, 0.0] for _ in range(stride)]
    c.ntasks = [1] * stride
    c.maxtasks = [110] * stride
    c.live, c.unsched = [True] * n_nodes, [False] * n_nodes
    c.sel_ok = [[True] * n_nodes for _ in range(classes)]
    c.taint_ok = [[True] * n_nodes for _ in range(classes)]
    return c


def shape(c, cls, req, best_effort=False):
    c.shapes.append(dict(cls=int(cls), best_effort=bool(best_effort), req=[float(v) for v in req]))
    c.p["n_shapes"] = len(c.shapes)


def near(rng, values, d):
    """A node value on or around one of the requests of dimension d."""
    if rng.random() < 0.15:
        return 0.0
    return float(max(0.0, values[int(rng.integers(0, 3))] + EDGES[int(rng.integers(0, len(EDGES)))] * tr.MIN[d]))


def random_case(name, seed, n_nodes, n_shapes, tab_lo=0, tab_n=None, cap_check=1, classes=3):
    rng = np.random.default_rng(seed)
    c = blank(name, n_nodes, tab_lo, tab_n, classes, cap_check)
    for row in range(c.p["stride"]):  # (rows past tab_n: values no lane may count)
        c.idle[row] = [near(rng, CPU, 0), near(rng, MEM, 1), near(rng, GPU, 2)]
        if rng.random() < 0.4:
            c.rel[row] = [near(rng, CPU, 0), near(rng, MEM, 1), near(rng, GPU, 2)]
        c.maxtasks[row] = int(rng.choice((2, 110)))
        c.ntasks[row] = int(rng.choice((0, 1, c.maxtasks[row] - 1, c.maxtasks[row], c.maxtasks[row] + 1),
                                       p=(0.3, 0.3, 0.15, 0.15, 0.1)))
    c.live = (rng.random(n_nodes) >= 0.1).tolist()
    c.unsched = (rng.random(n_nodes) < 0.1).tolist()
    c.sel_ok = (rng.random((classes, n_nodes)) < 0.8).tolist()
    c.taint_ok = (rng.random((classes, n_nodes)) < 0.85).tolist()
    for i in range(n_shapes):  # with three or more: shape 1 BestEffort, shape 2 without a GPU request
        be = rng.random() < 0.15 or (i == 1 and n_shapes >= 3)
        gpu = 0.0 if i == 2 else rng.choice(GPU)
        shape(c, rng.integers(0, classes), (rng.choice(CPU), rng.choice(MEM), gpu), be)
    return c


def edges_case():
    """One node per (dimension, against Idle or Releasing, offset): the other
    two dimensions fit with room, the other resource is far short. Shape 0 asks
    for the middle request of every dimension, shape 1 for no GPU."""
    rows_ = []
    req = [CPU[1], MEM[1], GPU[1]]
    for against in ("idle", "rel"):
        for d in range(3):
            for e in EDGES:
                v = [8000.0, 8192.0 * MI, 4000.0]
                v[d] = req[d] + e * tr.MIN[d]
                rows_.append((against, v))
    c = blank("tolerance-edges", len(rows_), classes=1)
    for row, (against, v) in enumerate(rows_):
        c.idle[row] = list(v) if against == "idle" else [0.0, 0.0, 0.0]
        c.rel[row] = list(v) if against == "rel" else [0.0, 0.0, 0.0]
    shape(c, 0, req)
    shape(c, 0, [CPU[1], MEM[1], 0.0])
    return c


def every_cause_case():
    """130 nodes, three words. Every device cause occurs for shape 0; the only
    unschedulable node, and the only node that fits Releasing alone, are in the
    last (ragged) word; nodes 3 and 4 sit at and one below their pod cap; node
    5 fails three stages at once; node 6 is dead and would fail each."""
    c = blank("every-cause", 130, classes=2)
    req = [1000.0, 1024.0 * MI, 0.0]
    c.ntasks[3], c.maxtasks[3] = 110, 110
    c.ntasks[4], c.maxtasks[4] = 109, 110
    c.sel_ok[0][5] = c.taint_ok[0][5] = False
    c.unsched[5] = True
    c.live[6] = False
    c.sel_ok[0][6] = False
    c.taint_ok[0][7] = False
    c.idle[8] = [500.0, 8192.0 * MI, 0.0]  # short of cpu, fits nothing
    c.unsched[129] = True
    c.idle[128] = [0.0, 0.0, 0.0]
    c.rel[128] = [1000.0, 1024.0 * MI, 0.0]  # exactly the request: fits Releasing only
    shape(c, 0, req)
    shape(c, 1, req)
    shape(c, 0, [5.0, 0.0, 0.0], best_effort=True)
    return c


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [random_case(f"n{n}-s{s}", 7000 + n + s, n, s) for n, s in
          ((1, 1), (63, GROUP - 1), (64, GROUP), (65, GROUP + 1), (127, 2), (128, 3), (129, GROUP + 1), (1023, 2),
           (1024, GROUP), (1025, 2 * GROUP + 1))]
    cs.append(random_case("n200-s5-cap0", 7301, 200, 5, cap_check=0))
    cs.append(random_case("shard64-93of200", 7302, 200, GROUP + 1, tab_lo=64, tab_n=93))
    cs.append(random_case("shard128-72of200", 7303, 200, 3, tab_lo=128, tab_n=72))
    cs.append(random_case("shard128-1of300", 7304, 300, 2, tab_lo=128, tab_n=1))
    cs.append(edges_case())
    cs.append(every_cause_case())
    return {c.name: c for c in cs}


def case(name):
    return _cases()[name]


NAMES = list(_cases())


# ------------------------------------------------------------------ layout
def planes_words(c):
    """The stage planes as kbg::StagePlanes lays them out: sel_ok, taint_ok
    [classes][W], unsched, live [W]; the bits past n_nodes are garbage (ones)."""
    n, k, W = c.p["n_nodes"], c.p["classes"], c.p["W"]
    bits = np.ones((2 * k + 2, W * 64), dtype=bool)
    bits[0:k, :n] = np.array(c.sel_ok)
    bits[k:2 * k, :n] = np.array(c.taint_ok)
    bits[2 * k, :n] = np.array(c.unsched)
    bits[2 * k + 1, :n] = np.array(c.live)
    return pack_words(bits).reshape(-1)


def table_block(c):
    """FirstFitArgs.nodes: idle c/m/g, rel c/m/g f64[stride], ntasks, maxtasks i32[stride]."""
    f = np.array([[v[d] for v in src] for src in (c.idle, c.rel) for d in range(3)], dtype="<f8")
    i = np.array([c.ntasks, c.maxtasks], dtype="<i4")
    return np.frombuffer(f.tobytes() + i.tobytes(), dtype=np.uint8).copy()


def shape_records(c):
    s = np.zeros(len(c.shapes), dtype=TASK_SHAPE)
    for r, d in zip(s, c.shapes):
        r["cls"], r["flags"], r["req"] = d["cls"], int(d["best_effort"]), d["req"]
    return s


def out_bytes(rows_):
    """The probe's raw output for these rows, then the guard region still holding the sentinel."""
    w = np.array([r["count"] + r["first_node"] + r["idle_short"] + [0] for r in rows_], dtype=np.int32)
    return np.concatenate([np.frombuffer(w.tobytes(), dtype=np.uint8), np.full(GUARD_BYTES, SENTINEL, dtype=np.uint8)])


def rows_of(c, raw):
    """(rows, padding and guard untouched) of a probe's raw output."""
    ns, n = len(c.shapes), tr.N_CAUSES
    w = np.frombuffer(raw[:ns * OUT_WORDS * 4].tobytes(), dtype=np.int32).reshape(ns, OUT_WORDS)
    rows_ = [dict(count=r[:n].tolist(), first_node=r[n:2 * n].tolist(), idle_short=r[2 * n:2 * n + 3].tolist())
             for r in w]
    return rows_, bool((raw[ns * OUT_WORDS * 4:] == SENTINEL).all() and (w[:, 2 * n + 3] == 0).all())


def compare_raw(c, raw):
    """Differences between a probe's raw output and the reference: the rows, then every byte."""
    got, clean = rows_of(c, raw)
    want = tr.rows(c)
    errs = tr.compare(c, want, got)
    if not clean:
        errs.append("the guard region after the rows, or a row's padding word, was overwritten")
    if not errs and not (raw == out_bytes(want)).all():
        errs.append("raw output differs from the reference's bytes")
    return errs


def run_probe(lib, c, ptr, params, p_over=None, mutate=None):
    """One kbg_tool_probe_task_why call on copies of the case's arrays: (rc, arrays as left, raw output)."""
    import ctypes
    lib.kbg_tool_probe_task_why.restype = ctypes.c_int32
    a = dict(block=table_block(c), planes=planes_words(c), shapes=shape_records(c))
    if mutate:
        mutate(a)
    p = dict(c.p, **(p_over or {}))
    raw = np.full(len(a["shapes"]) * OUT_WORDS * 4 + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    rc = lib.kbg_tool_probe_task_why(params(FIELDS, p), ptr(a["block"]), ptr(a["planes"]), ptr(a["shapes"]), ptr(raw))
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
    """(id, parameter overrides, mutation, what the message names) of launches kbg_task_reasons never makes."""
    def cls(a):
        a["shapes"]["cls"][1] = 3
    return [("tab_lo", dict(tab_lo=32), None, "tab_lo"), ("range", dict(tab_n=0), None, "node range"),
            ("past-n", dict(tab_n=10 ** 6), None, "node range"), ("stride", dict(stride=5), None, "table block"),
            ("n_shapes0", dict(n_shapes=0), None, "n_shapes"), ("cls", None, cls, "cls")]


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
