"""Seeded cases of the victim-reasons kernels and their flat layout for the
probe (kbg_tool_probe_victim_why): the tables of tests/victim_ref.py's seeded
generators, the four stage planes drawn over them, and several queries on one
table.

Per case: the planes are drawn first (some nodes dead, some failing two or
three stages at once, so the order of the stages matters), then class_mask is
set to sel_ok & taint_ok & ~unsched & live, as the session's is. The queries
mix modes, classes, jobs (with their queues), requests, drf shares and tier
lists (0, 1 and 2 tiers over the fn subsets); two of them are equal whenever a
case has more than one. Node counts 1, 15, 16, 17, 63, 64, 65 and 200 put the
table's end inside and at the end of a workgroup's nodes; candidate counts 0,
1, 63, 64, 65, 127, 128, 129 and 1024 sit on the chunk bounds of both kernels,
1025 is past them (neither kernel counts it); `big-group` puts several big
rows into one 32-node group."""
import functools
from types import SimpleNamespace

import numpy as np

import victim_ref as vr
import victim_why_ref as wr
from kernel_ref import GUARD_BYTES, SENTINEL, pack_words

OUT_WORDS = 2 * wr.N_CAUSES + 3  # kVictimWhyOut: count, first_node, fn_empty

VICTIM_SCAN = np.dtype([("n_nodes", "<i4"), ("W", "<i4"), ("cls", "<i4"), ("cap_check", "<i4"), ("node_lo", "<i4"),
                        ("node_n", "<i4"), ("mode", "<i4"), ("n_tiers", "<i4"), ("tier_fns", "<i4", (8,)),
                        ("job", "<i4"), ("queue", "<i4"), ("req", "<f8", (3,)), ("ls", "<f8")])
assert VICTIM_SCAN.itemsize == 104

FIELDS = ("n_nodes", "W", "node_lo", "node_n", "stride", "classes", "n_cand", "n_jobs", "n_queues", "nq", "n_rows")
TIER_LISTS = ([], [1], [2], [4], [3], [5], [6], [7], [1, 2], [1, 4], [2, 4], [4, 2], [3, 4], [1, 6], [5, 2], [7, 7],
              [2, 1], [6, 1])
BOUNDARY_L = (0, 1, 63, 64, 65, 127, 128)


def draw_planes(c, rng, dead=0.1, sel=0.8, tol=0.85, uns=0.1):
    n, k = c.p["n_nodes"], c.p["classes"]
    c.live = (rng.random(n) >= dead).tolist()
    c.unsched = (rng.random(n) < uns).tolist()
    c.sel_ok = (rng.random((k, n)) < sel).tolist()
    c.taint_ok = (rng.random((k, n)) < tol).tolist()
    set_class_mask(c)


def set_class_mask(c):
    n, k, W = c.p["n_nodes"], c.p["classes"], c.p["W"]
    bits = np.zeros((k, W * 64), dtype=bool)
    for cls in range(k):
        bits[cls, :n] = np.array(c.sel_ok[cls]) & np.array(c.taint_ok[cls]) & ~np.array(c.unsched) & np.array(c.live)
    c.class_mask = pack_words(bits).reshape(k, W)


def draw_queries(c, b, rng, nq, cap_check, tier_lists=TIER_LISTS):
    qs = []
    for i in range(nq):
        job = int(rng.integers(0, len(b.jobs)))
        tiers = list(tier_lists[int(rng.integers(0, len(tier_lists)))])
        qs.append(dict(mode=int(rng.integers(0, 3)), cls=int(rng.integers(0, c.p["classes"])),
                       cap_check=int(cap_check if cap_check in (0, 1) else rng.integers(0, 2)), n_tiers=len(tiers),
                       tier_fns=tiers, job=job, queue=b.jobs[job]["queue"],
                       req=[float(v) for v in (rng.choice((300, 1000, 4000)), rng.choice((300, 1024, 4096)) * vr.MI,
                                               rng.choice((300, 1000, 4000)))],
                       ls=float(b.ls * rng.choice((0.0, 0.5, 1.0, 1.0, 1.5)))))
    if nq > 1:  # two equal queries: computed once by the session, copied to both jobs
        qs[-1] = dict(qs[int(rng.integers(0, nq - 1))])
    c.queries = qs
    c.p["nq"] = nq


def make(name, seed, counts, nq, cap_check=1, classes=3, node_lo=0, node_n=None, fns=7, mode=vr.VM_RECLAIM,
         tier_lists=TIER_LISTS, W=None, zero_gpu_total=False):
    rng = np.random.default_rng(seed)
    b = vr.random_builder(rng, mode, fns, counts, zero_gpu_total=zero_gpu_total)
    c = b.finish(name, seed, node_lo=node_lo, node_n=node_n, W=W, classes=classes)
    draw_planes(c, rng)
    draw_queries(c, b, rng, nq, cap_check, tier_lists)
    return c


def counts_for(rng, n_nodes, must=()):
    return vr.rand_counts(rng, n_nodes, must)


def _sized(n_nodes, nq, seed, cap_check=1, must=None):
    rng = np.random.default_rng(seed + 1000)
    must = BOUNDARY_L if must is None and n_nodes >= 15 else (must or (64,))
    return make(f"n{n_nodes}-q{nq}-cap{cap_check}", seed, counts_for(rng, n_nodes, must[:n_nodes]), nq, cap_check)


def _big_group():
    """Nine big rows, seven of them inside the 32-node group [32, 64), next to
    a node past the bound; the rest of the table mixed."""
    rng = np.random.default_rng(9100)
    counts = counts_for(rng, 70, BOUNDARY_L)
    for n, L in zip((33, 34, 35, 36, 38, 40, 63, 0, 69, 37), (129, 192, 1023, 1024, 193, 130, 257, 129, 1024, 1025)):
        counts[n] = L
    c = make("big-group", 9100, counts, 3, cap_check=2)
    for n in (33, 34, 35, 36, 38, 40, 63, 0, 69, 37):  # the big nodes are the point: live, inside every stage
        c.live[n], c.unsched[n], c.panic_node[n] = True, False, 0
        c.ntasks[n - c.p["node_lo"]], c.maxtasks[n - c.p["node_lo"]] = 1, 110
        for k in range(c.p["classes"]):
            c.sel_ok[k][n] = c.taint_ok[k][n] = True
    set_class_mask(c)
    return c


def _shard():
    rng = np.random.default_rng(9200)
    return make("shard64-93of200", 9200, counts_for(rng, 200, BOUNDARY_L + (129, 1024)), 3, node_lo=64, node_n=93, W=4)


def _tiers(nq, seed, lists, name):
    rng = np.random.default_rng(seed + 1000)
    return make(name, seed, counts_for(rng, 65, BOUNDARY_L), nq, tier_lists=lists)


def _edge_lanes():
    """Nodes of L candidates whose only preemptee is the last one (a chunk's
    last lane for 64, 128 and 1024, the first lane of the next chunk for 65
    and 129): the reclaimer's own queue holds the others. Gang keeps it and
    its request covers the reclaimer's: VICTIMS, unless the lane is lost."""
    b = vr.Builder(vr.VM_RECLAIM, 1)
    other = b.job(b.queue(), jmin=1, ready=3)
    for L in (64, 65, 128, 129, 1024):
        b.node([(0, vr.R1)] * (L - 1) + [(other, vr.R1)])
    c = b.finish("edge-lanes", 9500)
    n = c.p["n_nodes"]
    c.live, c.unsched, c.sel_ok, c.taint_ok = [True] * n, [False] * n, [[True] * n], [[True] * n]
    set_class_mask(c)
    q = dict(mode=vr.VM_RECLAIM, cls=0, cap_check=1, n_tiers=1, tier_fns=[1], job=0, queue=0,
             req=[300.0, 300.0 * vr.MI, 300.0], ls=0.0)
    c.queries = [q, dict(q, mode=vr.VM_PREEMPT_TASKS, tier_fns=[2, 1], n_tiers=2), dict(q)]
    c.p["nq"] = 3
    return c


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [_sized(1, 1, 9001, must=(64,)), _sized(1, 2, 9002, cap_check=0, must=(0,)), _sized(15, 2, 9003),
          _sized(16, 3, 9004), _sized(17, 1, 9005, cap_check=0), _sized(63, 3, 9006), _sized(64, 2, 9007),
          _sized(65, 17, 9008), _sized(200, 17, 9009, cap_check=2), _sized(200, 3, 9010, cap_check=0)]
    cs.append(_big_group())
    cs.append(_shard())
    cs.append(_edge_lanes())
    # every fn subset alone, then in two tiers; no tier at all
    cs.append(_tiers(17, 9300, [[f] for f in range(1, 8)], "one-tier-subsets"))
    cs.append(_tiers(17, 9301, [[a, b] for a in range(1, 8) for b in (1, 2, 4, 7)], "two-tier-subsets"))
    cs.append(_tiers(2, 9302, [[]], "no-tier"))
    rng = np.random.default_rng(9400)
    cs.append(make("big-mixed", 9400, [int(rng.choice((0, 3, 64, 128, 129, 500, 1024))) for _ in range(40)], 3,
                   mode=vr.VM_PREEMPT_JOBS, fns=3, zero_gpu_total=True))
    return {c.name: c for c in cs}


def case(name):
    return _cases()[name]


NAMES = list(_cases())


# ------------------------------------------------------------------ layout
def planes_words(c):
    """The stage planes as kbg::StagePlanes lays them out: sel_ok, taint_ok
    [classes][W], unsched, live [W] (bits past n_nodes: garbage, never read)."""
    n, k, W = c.p["n_nodes"], c.p["classes"], c.p["W"]
    bits = np.ones((2 * k + 2, W * 64), dtype=bool)
    bits[0:k, :n] = np.array(c.sel_ok)
    bits[k:2 * k, :n] = np.array(c.taint_ok)
    bits[2 * k, :n] = np.array(c.unsched)
    bits[2 * k + 1, :n] = np.array(c.live)
    return pack_words(bits).reshape(-1)


def query_records(c):
    q = np.zeros(len(c.queries), dtype=VICTIM_SCAN)
    for r, d in zip(q, c.queries):
        for f in ("n_nodes", "W", "node_lo", "node_n"):
            r[f] = c.p[f]
        for f in ("cls", "cap_check", "mode", "n_tiers", "job", "queue", "ls"):
            r[f] = d[f]
        r["tier_fns"][:d["n_tiers"]] = d["tier_fns"]
        r["req"] = d["req"]
    return q


def out_bytes(rows_):
    """The probe's raw output for these rows: [nq][OUT_WORDS] words, then the
    guard region still holding the sentinel."""
    w = np.array([r["count"] + r["first_node"] + r["fn_empty"] for r in rows_], dtype=np.int32)
    return np.concatenate([np.frombuffer(w.tobytes(), dtype=np.uint8), np.full(GUARD_BYTES, SENTINEL, dtype=np.uint8)])


def rows_of(c, raw):
    """(rows, guard_ok) of a probe's raw output."""
    nq = len(c.queries)
    w = np.frombuffer(raw[:nq * OUT_WORDS * 4].tobytes(), dtype=np.int32).reshape(nq, OUT_WORDS)
    n = wr.N_CAUSES
    rows_ = [dict(count=r[:n].tolist(), first_node=r[n:2 * n].tolist(), fn_empty=r[2 * n:].tolist()) for r in w]
    return rows_, bool((raw[nq * OUT_WORDS * 4:] == SENTINEL).all())


TABLES = ("panic_node", "nt_off", "c_jq", "c_req", "c_run", "j_min", "j_ready", "j_alloc", "q_alloc", "q_deserved")


def run_probe(lib, c, ptr, params, p_over=None, mutate=None):
    """One kbg_tool_probe_victim_why call on copies of the case's arrays:
    (rc, the arrays as the probe left them, raw output)."""
    import ctypes
    lib.kbg_tool_probe_victim_why.restype = ctypes.c_int32
    a = {k: np.ascontiguousarray(getattr(c, k)).copy() for k in TABLES}
    a["block"] = vr.table_block(c)
    a["planes"] = planes_words(c)
    a["total"] = np.ascontiguousarray(c.dbl[4:7]).copy()
    a["queries"] = query_records(c)
    if mutate:
        mutate(a)
    p = dict(dict(c.p, n_rows=len(vr.big_rows(c))), **(p_over or {}))
    raw = np.full(len(a["queries"]) * OUT_WORDS * 4 + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    order = ("block", "panic_node", "planes", "nt_off", "c_jq", "c_req", "c_run", "j_min", "j_ready", "j_alloc",
             "q_alloc", "q_deserved", "total", "queries")
    rc = lib.kbg_tool_probe_victim_why(params(FIELDS, p), *[ptr(a[k]) for k in order], ptr(raw))
    return rc, a, raw


def check_probe(lib, c, ptr, params):
    """Errors of one case through the probe: rows, guard, untouched tables."""
    rc, a, raw = run_probe(lib, c, ptr, params)
    if rc != 0:
        return rc, [f"probe returned {rc}: {lib.kbg_tool_probe_error()}"]
    got, guard_ok = rows_of(c, raw)
    errs = wr.compare(c, wr.rows(c, huge=False), got)
    if not guard_ok:
        errs.append("guard region after the result rows overwritten")
    if not (raw == out_bytes(wr.rows(c, huge=False))).all() and not errs:
        errs.append("raw output differs from the reference's bytes")
    for k in TABLES:
        if not (a[k] == np.ascontiguousarray(getattr(c, k))).all():
            errs.append(f"input table {k} changed")
    if not (a["block"] == vr.table_block(c)).all():
        errs.append("node table block changed")
    return 0, errs
