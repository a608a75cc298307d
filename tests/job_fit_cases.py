"""Seeded and hand-made cases of kbg_job_fit_kernel and their flat layout for
the probe (kbg_tool_probe_job_fit), at the smallest sizes where the kernel can
go wrong: tables of 1, 63, 64, 65, 130, 257 and 600 nodes (a lane per node of
a 64-node word: one lane, a ragged word, one word, a word and a lane, three
words, more than four, ten), shards of 93 of 200 nodes from node 64 and of 1 of
300 from node 128, launches of 1, 2, 5 and 70 jobs (a wave and a workgroup per
job), walks of 1, 2, 7, 64, 65 and 512 steps (the overlay is looked through 64
entries at a time and holds 512), cap_check 0 and 1, dead nodes and rows past
tab_n holding garbage, garbage plane bits past the last node, and hand-worked
walks (`claims`: job -> [(node, kind)], written by hand).

The table block, the planes and the shape records are laid out as
tests/task_why_cases.py lays them out (the kernels read the same data)."""
import functools

import numpy as np

import job_fit_ref as jr
from headroom_cases import BIG, garbage, multiple
from kernel_ref import GUARD_BYTES, SENTINEL
from task_why_cases import CPU, GPU, MEM, MI, blank as _blank, planes_words, shape, shape_records, table_block

FIELDS = ("n_nodes", "W", "tab_lo", "tab_n", "stride", "classes", "n_shapes", "cap_check", "n_jobs", "n_steps")
STEP = np.dtype([("shape", "<i4"), ("prev", "<i4")])
G = 1024.0 * MI
A, P = jr.ALLOCATE, jr.PIPELINE
NOWHERE = (-1, 0)


def blank(name, n_nodes, **kw):
    c = _blank(name, n_nodes, **kw)
    c.jobs, c.claims = [], {}
    return c


def job(c, steps, claim=None):
    c.jobs.append([int(s) for s in steps])
    if claim is not None:
        c.claims[len(c.jobs) - 1] = list(claim)


def random_case(name, seed, n_nodes, walk_lens, n_shapes=4, tab_lo=0, tab_n=None, cap_check=1, classes=3):
    rng = np.random.default_rng(seed)
    c = blank(name, n_nodes, tab_lo=tab_lo, tab_n=tab_n, classes=classes, cap_check=cap_check)
    c.live = (rng.random(n_nodes) >= 0.1).tolist()
    for row in range(c.p["stride"]):
        c.idle[row] = [multiple(rng, CPU, 0), multiple(rng, MEM, 1), multiple(rng, GPU, 2)]
        if rng.random() < 0.4:
            c.rel[row] = [multiple(rng, CPU, 0), multiple(rng, MEM, 1), multiple(rng, GPU, 2)]
        c.maxtasks[row] = int(rng.choice((2, 8, 110)))
        c.ntasks[row] = int(rng.choice((0, 1, c.maxtasks[row] - 1, c.maxtasks[row], c.maxtasks[row] + 1),
                                       p=(0.3, 0.3, 0.15, 0.15, 0.1)))
        n = tab_lo + row
        if row >= c.p["tab_n"] or (n < n_nodes and not c.live[n]):  # values no lane may use
            c.idle[row], c.rel[row] = garbage(rng), garbage(rng)
            c.ntasks[row], c.maxtasks[row] = int(rng.integers(-2 ** 31, 2 ** 31)), int(rng.integers(-2 ** 31, 2 ** 31))
    c.unsched = (rng.random(n_nodes) < 0.1).tolist()
    c.sel_ok = (rng.random((classes, n_nodes)) < 0.8).tolist()
    c.taint_ok = (rng.random((classes, n_nodes)) < 0.85).tolist()
    for i in range(n_shapes):  # shape 2 without a GPU request
        shape(c, rng.integers(0, classes), (rng.choice(CPU), rng.choice(MEM), 0.0 if i == 2 else rng.choice(GPU)))
    for ln in walk_lens:  # a gang: mostly copies of one member, some members of their own
        main = int(rng.integers(0, n_shapes))
        job(c, [main if rng.random() < 0.7 else int(rng.integers(0, n_shapes)) for _ in range(ln)])
    return c


def empty(name, n_nodes, **kw):
    """Every node with nothing Idle or Releasing and a pod room no walk fills."""
    c = blank(name, n_nodes, **kw)
    for row in range(c.p["stride"]):
        c.idle[row], c.rel[row], c.ntasks[row], c.maxtasks[row] = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0, BIG
    return c


def hand_cases():
    """The hand-worked walks. R asks for 1000m / 1Gi, H for 500m / 512Mi."""
    R, H = [1000.0, G, 0.0], [500.0, G / 2, 0.0]
    out = []

    c = empty("two-on-one-node", 3, classes=1)
    c.idle[0] = [2000.0, 2 * G, 0.0]
    shape(c, 0, R)
    job(c, [0, 0, 0], [(0, A), (0, A), NOWHERE])  # the second sees the first's subtraction, the third both
    out.append(c)

    c = empty("lane-63-then-64", 70, classes=1)
    c.idle[63], c.idle[64] = list(R), list(R)
    shape(c, 0, R)
    job(c, [0, 0, 0], [(63, A), (64, A), NOWHERE])
    out.append(c)

    c = empty("releasing-before-the-next-node", 3, classes=1)
    c.idle[0], c.rel[0], c.idle[1] = list(R), list(R), [5000.0, 8 * G, 0.0]
    shape(c, 0, R)
    job(c, [0, 0, 0], [(0, A), (0, P), (1, A)])  # node 0's Releasing before node 1's Idle
    out.append(c)

    c = empty("pod-room-of-one", 2, classes=1)
    c.idle[0], c.idle[1] = [9000.0, 64 * G, 0.0], [9000.0, 64 * G, 0.0]
    c.ntasks[0], c.maxtasks[0] = 109, 110
    shape(c, 0, R)
    job(c, [0, 0], [(0, A), (1, A)])  # the walk itself fills node 0's last pod slot
    out.append(c)

    c = empty("another-class-before-the-cursor", 3, classes=2)
    c.idle[0], c.idle[2] = [9000.0, 64 * G, 0.0], [9000.0, 64 * G, 0.0]
    c.sel_ok[0][0] = False
    shape(c, 0, R)
    shape(c, 1, R)
    job(c, [0, 1, 0], [(2, A), (0, A), (2, A)])  # class 1's first fit, node 0, lies before class 0's cursor
    out.append(c)

    c = empty("back-to-a-touched-word", 130, classes=1)
    c.idle[5], c.idle[70] = [1500.0, 2 * G, 0.0], list(R)
    shape(c, 0, R)
    shape(c, 0, H)
    job(c, [0, 1, 0], [(5, A), (5, A), (70, A)])  # H leaves node 5 at 0m / 512Mi: R's cursor node no longer fits
    out.append(c)

    c = empty("unplaced-then-smaller", 2, classes=1)
    c.idle[0] = [500.0, G, 0.0]
    shape(c, 0, R)
    shape(c, 0, H)
    job(c, [0, 1, 0], [NOWHERE, (0, A), NOWHERE])  # the walk goes on; R's prev landed nowhere, so does R
    out.append(c)

    c = empty("tolerance-once", 2, classes=1, cap_check=0)
    c.idle[0] = [3.0, 8192.0 * MI, 0.0]
    shape(c, 0, [8.0, 64.0 * MI, 0.0])
    job(c, [0, 0], [(0, A), NOWHERE])  # |3 - 8| < 10 fits and leaves -5; |-5 - 8| = 13 does not
    out.append(c)

    c = empty("non-integer", 6, classes=1, cap_check=0)  # headroom_cases.tolerance_case's nodes 3 and 4
    c.idle[3], c.idle[4] = [450.8, 8192.0 * MI, 0.0], [221.5, 8192.0 * MI, 0.0]
    shape(c, 0, [57.6, 64.0 * MI, 0.0])
    shape(c, 0, [46.3, 64.0 * MI, 0.0])
    # 57.6 from 450.8: seven subtractions leave 47.6 and a bit, |a - 57.6| not below 10 (450.8 - 7 * 57.6 would
    # be): 7 on node 3. Node 4: 221.5, 163.9, 106.3 fit, 48.7 fits within the tolerance (8.9), -8.9 does not: 4.
    job(c, [0] * 12, [(3, A)] * 7 + [(4, A)] * 4 + [NOWHERE])
    # 46.3 from 450.8: 450.8, 404.5, ..., 80.4 fit (nine), 34.1 does not (12.2 away): 9 on node 3. Node 4: 221.5,
    # 175.2, 128.9, 82.6 fit; four subtractions leave 36.3 and a bit, not within 10 (the product would be): 4.
    job(c, [1] * 14, [(3, A)] * 9 + [(4, A)] * 4 + [NOWHERE])
    out.append(c)

    c = empty("512-on-one-node", 2, classes=1)
    c.idle[1] = [51200.0, 512 * 64.0 * MI, 0.0]
    shape(c, 0, [100.0, 64.0 * MI, 0.0])
    job(c, [0] * 512, [(1, A)] * 512)  # 51200 - 100 k: the 512th meets exactly 100m / 64Mi
    out.append(c)

    c = empty("512-on-512-nodes", 600, classes=1)
    for n in range(600):
        c.idle[n] = [100.0, 64.0 * MI, 0.0]
    c.live[10] = c.live[100] = False
    c.idle[10], c.idle[100] = [1e300, 1e300, 1e300], [1e300, 1e300, 1e300]
    shape(c, 0, [100.0, 64.0 * MI, 0.0])
    live = [n for n in range(600) if n not in (10, 100)]
    job(c, [0] * 512, [(n, A) for n in live[:512]])  # one each: the i-th step on the i-th live node
    out.append(c)

    c = empty("shard-70-of-200", 200, tab_lo=64, tab_n=70, classes=1, stride=70)
    c.idle[3], c.idle[69] = list(R), list(R)  # nodes 67 and 133, the table's last row
    shape(c, 0, R)
    job(c, [0, 0, 0], [(67, A), (133, A), NOWHERE])  # global indices; nothing past the table's last row
    out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [random_case(f"n{n}-j{len(w)}", 11001 + n, n, w) for n, w in
          ((1, (1,)), (63, (2, 7)), (64, (7,) * 5), (65, (64, 65)), (130, (1, 2, 7, 64, 65)), (257, (7,) * 70),
           (600, (512, 65)))]
    cs.append(random_case("n200-j5-cap0", 11301, 200, (7, 64, 2, 65, 1), cap_check=0))
    cs.append(random_case("shard64-93of200", 11303, 200, (64, 7), tab_lo=64, tab_n=93))
    cs.append(random_case("shard128-1of300", 11315, 300, (2, 1), tab_lo=128, tab_n=1))
    return {c.name: c for c in cs + hand_cases()}


def case(name):
    return _cases()[name]


NAMES = list(_cases())
HAND = [c.name for c in hand_cases()]
SEEDED = [n for n in NAMES if n not in HAND]


# ------------------------------------------------------------------ layout
def step_records(c):
    recs = np.zeros(sum(len(j) for j in c.jobs), dtype=STEP)
    k = 0
    for j in c.jobs:
        for s, p in zip(j, jr.links(c, j)):
            recs[k] = (s, p)
            k += 1
    return recs


def job_offsets(c):
    return np.cumsum([0] + [len(j) for j in c.jobs]).astype("<i4")


def out_bytes(walks_):
    """The probe's raw output for these walks, then the guard region still holding the sentinel."""
    w = np.array([v for wk in walks_ for pl in wk for v in pl], dtype=np.int32)
    return np.concatenate([np.frombuffer(w.tobytes(), dtype=np.uint8), np.full(GUARD_BYTES, SENTINEL, dtype=np.uint8)])


def walks_of(c, raw):
    """(walks, guard untouched) of a probe's raw output."""
    n = sum(len(j) for j in c.jobs)
    w = np.frombuffer(raw[:n * 8].tobytes(), dtype=np.int32).reshape(n, 2).tolist()
    out, k = [], 0
    for j in c.jobs:
        out.append([tuple(p) for p in w[k:k + len(j)]])
        k += len(j)
    return out, bool((raw[n * 8:] == SENTINEL).all())


def compare_raw(c, raw):
    """Differences between a probe's raw output and the reference: the walks, then every byte."""
    got, clean = walks_of(c, raw)
    want = jr.walks(c)
    errs = jr.compare(c, want, got)
    if not clean:
        errs.append("the guard region after the places was overwritten")
    if not errs and not (raw == out_bytes(want)).all():
        errs.append("raw output differs from the reference's bytes")
    return errs


def run_probe(lib, c, ptr, params, p_over=None, mutate=None):
    """One kbg_tool_probe_job_fit call on copies of the case's arrays: (rc, arrays as left, raw output)."""
    import ctypes
    lib.kbg_tool_probe_job_fit.restype = ctypes.c_int32
    a = dict(block=table_block(c), planes=planes_words(c), shapes=shape_records(c), steps=step_records(c),
             off=job_offsets(c))
    if mutate:
        mutate(a)
    p = dict(c.p, n_jobs=len(a["off"]) - 1, n_steps=len(a["steps"]), **(p_over or {}))
    raw = np.full(len(a["steps"]) * 8 + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    planes = ptr(a["planes"]) if a["planes"] is not None else None
    rc = lib.kbg_tool_probe_job_fit(params(FIELDS, p), ptr(a["block"]), planes, ptr(a["shapes"]), ptr(a["steps"]),
                                    ptr(a["off"]), ptr(raw))
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
    """(id, parameter overrides, mutation, what the message names) of launches kbg_job_fit never makes."""
    def shape_index(a):
        a["steps"]["shape"][3] = len(a["shapes"])

    def best_effort(a):
        a["shapes"]["flags"][int(a["steps"]["shape"][0])] = 1

    def prev_later(a):
        a["steps"]["prev"][2] = 2

    def prev_other_shape(a):
        s = a["steps"]
        k = next(i for i in range(1, 64) if s["shape"][i] != s["shape"][0])
        s["prev"][k] = 0

    def prev_other_job(a):  # the second job's first step naming a step of the first
        a["steps"]["prev"][64] = 3

    def steps_513(a):
        a["steps"] = np.zeros(513, dtype=STEP)
        a["steps"]["prev"] = -1
        a["off"] = np.array([0, 513], dtype="<i4")

    def no_planes(a):
        a["planes"] = None
    return [("tab_lo", dict(tab_lo=32), None, "tab_lo"), ("range", dict(tab_n=0), None, "node range"),
            ("past-n", dict(tab_n=10 ** 6), None, "node range"), ("stride", dict(stride=5), None, "table block"),
            ("planes", None, no_planes, "null planes"), ("shape-index", None, shape_index, "shape index"),
            ("best-effort", None, best_effort, "BestEffort"), ("prev-later", None, prev_later, "prev"),
            ("prev-other-shape", None, prev_other_shape, "prev"), ("prev-other-job", None, prev_other_job, "prev"),
            ("steps-513", None, steps_513, "more than 512 steps"),
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
