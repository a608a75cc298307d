"""Plain reference of the preempt / reclaim victim scan, the seeded cases of
its kernel probe (tests/test_victim_kernels_gpu.py) and what each case claims
to hold (tests/test_victim_ref.py checks the claims on the reference alone).

`evaluate` restates, for one node, what the Go scheduler does when a
preemptor or reclaimer reaches it: PredicateFn (static class bit, the nil
node panic, the pod cap), the preemptee filter of the action over the node's
Running tasks in NodeInfo.Tasks order, the victim fns of the deciding tier
(gang.go:104-124, drf.go:80-105, proportion.go:161-186) intersected as
session_plugins.go:59-140 does, and validateVictims (preempt.go:238-253,
reclaim.go:137-150). It works on lists and dicts, one candidate after the
other; nothing of the kernels' chunks, lanes or masks is in it. All values are
float64 (Python floats), so the comparison with the device is exact.

`defect` selects one deliberately wrong variant (DEFECTS): the tests use them
to show that the cases and the comparator would notice a kernel that is wrong
in that way."""
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from kernel_ref import GUARD_BYTES, K_MIN, NODE_DELTA, SENTINEL, pack_words

VP_GANG, VP_DRF, VP_PROP = 1, 2, 4
VM_PREEMPT_JOBS, VM_PREEMPT_TASKS, VM_RECLAIM = 0, 1, 2
MAX_NODE_CANDIDATES = 1024  # kMaxNodeCandidates
ARG_NODE_DELTAS, ARG_STATE_DELTAS = 16, 48
SHARE_DELTA = 0.000001  # drf.go shareDelta
NONE, STOP, PANIC = 0, 1, 2
MI = 1 << 20

STATE_DELTA = np.dtype([("kind", "<i4"), ("index", "<i4"), ("v", "<f8", (3,))])

DEFECTS = ("earlier_chunks_ignored", "before_own_subtraction", "c_run_ignored", "panic_dropped",
           "skip_subtracts", "gang_list_to_drf", "sum_preemptees", "last_lane_lost", "big_wrong_word",
           "stale_byte")


class RefPanic(Exception):
    """The Go process would panic here (Resource.Sub, resource_info.go:100-110)."""


# ---------------------------------------------------------------- Resource
def less(a, b):
    return a[0] < b[0] and a[1] < b[1] and a[2] < b[2]


def less_equal(a, b, kmin=K_MIN):
    return all(a[d] < b[d] or abs(b[d] - a[d]) < kmin[d] for d in range(3))


def share(alloc, total):
    """drf.go:156-166 with helpers.Share."""
    res = 0
    for d in range(3):
        if total[d] == 0:
            s = 0 if alloc[d] == 0 else 1
        else:
            s = alloc[d] / total[d]
        if s > res:
            res = s
    return res


# ------------------------------------------------------------------- state
def state(c, prep=True, num=float):
    """The tables the scan reads, as lists of `num`, after the case's deltas
    (prep) or before them."""
    s = SimpleNamespace()
    s.ntasks = [int(v) for v in c.ntasks]
    s.maxtasks = [int(v) for v in c.maxtasks]
    s.c_run = [int(v) for v in c.c_run]
    s.j_ready = [int(v) for v in c.j_ready]
    conv = (lambda v: Fraction(float(v))) if num is Fraction else float
    rows = lambda a: [[conv(v) for v in r] for r in a]
    s.c_req = rows(c.c_req)
    s.j_alloc = rows(c.j_alloc)
    s.q_alloc = rows(c.q_alloc)
    s.q_deserved = rows(c.q_deserved)
    s.req = [conv(v) for v in c.dbl[0:3]]
    s.ls = conv(c.dbl[3])
    s.total = [conv(v) for v in c.dbl[4:7]]
    s.kmin = [conv(v) for v in K_MIN]
    s.share_delta = conv(SHARE_DELTA)
    if prep:
        for d in c.nd[:c.p["nn"]]:
            s.ntasks[d["node"]] = int(d["ntasks"])
            s.maxtasks[d["node"]] = int(d["maxtasks"])
        for d in c.sd[:c.p["ns"]]:
            k, i = int(d["kind"]), int(d["index"])
            if k == 0:
                s.c_run[i] = int(d["v"][0] != 0.0)
            elif k == 1:
                s.j_ready[i] = int(d["v"][0])
            else:
                (s.j_alloc if k == 2 else s.q_alloc)[i] = [conv(v) for v in d["v"]]
    return s


def is_preemptee(p, job, queue):
    if p["mode"] == VM_PREEMPT_JOBS:  # preempt.go:100-112
        return queue == p["queue"] and job != p["job"]
    if p["mode"] == VM_PREEMPT_TASKS:  # preempt.go:146-154
        return job == p["job"]
    return queue != p["queue"]  # reclaim.go:122-133


def evaluate(c, s, n, defect=None, events=None, victims_out=None):
    """NONE (the action moves on to the next node), STOP (validated victims)
    or PANIC at node n. `events` collects the names of the branches taken;
    `victims_out` receives the victims' candidate indices within the node."""
    p = c.p
    ev = events.add if events is not None else (lambda name: None)
    if not (int(c.class_mask[p["cls"], n >> 6]) >> (n & 63)) & 1:
        if c.panic_node[n]:
            ev("panic_node_class_off")
        return NONE
    off, L = int(c.nt_off[n]), int(c.nt_off[n + 1] - c.nt_off[n])
    if c.panic_node[n]:  # predicates.go:122-123
        ev("panic_node_empty" if L == 0 else "panic_node")
        return PANIC
    row = n - p["node_lo"]
    if s.ntasks[row] == s.maxtasks[row]:
        ev("cap_equal_checked" if p["cap_check"] else "cap_equal_unchecked")
    if p["cap_check"] and s.ntasks[row] >= s.maxtasks[row]:  # predicates.go:125-127
        return NONE
    job = lambda k: int(c.c_jq[off + k, 0])
    queue = lambda k: int(c.c_jq[off + k, 1])
    req = lambda k: s.c_req[off + k]
    pre = []
    for k in range(L):
        if defect == "last_lane_lost" and k % 64 == 63:
            continue
        if not s.c_run[off + k] and defect != "c_run_ignored":
            continue
        if is_preemptee(p, job(k), queue(k)):
            pre.append(k)
    if p["n_tiers"] == 0 or not pre:
        return NONE
    pre_set, pre_jobs, pre_queues = set(pre), {job(k) for k in pre}, {queue(k) for k in pre}
    for k in range(L):
        if k in pre_set:
            continue
        kind = "not_running" if not s.c_run[off + k] else "filtered"
        if job(k) in pre_jobs:
            ev(kind + "_shares_job")
        if queue(k) in pre_queues:
            ev(kind + "_shares_queue")
    fns = p["tier_fns"]

    def sub(a, r, who):  # Resource.Sub
        if not less_equal(r, a, s.kmin):
            ev(who + "_sub_panic")
            if defect != "panic_dropped":
                raise RefPanic()
        elif any(a[d] < r[d] for d in range(3)):
            ev(who + "_sub_negative_within_tolerance")
        for d in range(3):
            a[d] = a[d] - r[d]

    keeps = []
    try:
        gang = []
        for k in pre:  # gang.go:104-124
            jmin, ready = int(c.j_min[job(k)]), s.j_ready[job(k)]
            if jmin == ready - 1:
                ev("gang_min_eq_ready_minus_1")
            if jmin == ready:
                ev("gang_min_eq_ready")
            if jmin <= ready - 1:
                gang.append(k)
        if fns & VP_GANG:
            keeps.append(set(gang))
        feed = gang if defect == "gang_list_to_drf" and fns & VP_GANG else pre
        if fns & VP_DRF:  # drf.go:80-105
            keep, alloc, chunk = set(), {}, -1
            for k in feed:
                if defect == "earlier_chunks_ignored" and k // 64 != chunk:
                    alloc, chunk = {}, k // 64
                if job(k) not in alloc:
                    alloc[job(k)] = list(s.j_alloc[job(k)])
                a = alloc[job(k)]
                if defect == "before_own_subtraction":
                    rs = share(a, s.total)
                sub(a, req(k), "drf")
                if defect != "before_own_subtraction":
                    rs = share(a, s.total)
                for d in range(3):
                    if s.total[d] == 0:
                        ev("drf_zero_total_zero_alloc" if a[d] == 0 else "drf_zero_total_nonzero_alloc")
                if s.ls < rs:
                    ev("drf_ls_lt_rs")
                elif abs(s.ls - rs) <= s.share_delta:
                    ev("drf_within_share_delta")
                elif abs(s.ls - rs) <= 2 * s.share_delta:
                    ev("drf_just_beyond_share_delta")
                if s.ls < rs or abs(s.ls - rs) <= s.share_delta:
                    keep.add(k)
            keeps.append(keep)
        if fns & VP_PROP:  # proportion.go:161-186
            keep, alloc, chunk = set(), {}, -1
            for k in feed:
                if defect == "earlier_chunks_ignored" and k // 64 != chunk:
                    alloc, chunk = {}, k // 64
                q = queue(k)
                if q not in alloc:
                    alloc[q] = list(s.q_alloc[q])
                a = alloc[q]
                if less(a, req(k)):
                    ev("prop_less_skip")
                    if defect == "skip_subtracts":
                        for d in range(3):
                            a[d] = a[d] - req(k)[d]
                    continue
                if any(a[d] == req(k)[d] for d in range(3)) and sum(a[d] < req(k)[d] for d in range(3)) == 2:
                    ev("prop_one_dim_equal_no_skip")
                before = list(a)
                sub(a, req(k), "prop")
                des = s.q_deserved[q]
                at = before if defect == "before_own_subtraction" else a
                if less_equal(des, at, s.kmin):
                    if any(0 < des[d] - at[d] < s.kmin[d] for d in range(3)):
                        ev("deserved_le_inside_tolerance")
                    keep.add(k)
                elif sum(not (des[d] < at[d] or abs(at[d] - des[d]) < s.kmin[d]) for d in range(3)) == 1 and \
                        any(des[d] - at[d] == s.kmin[d] for d in range(3)):
                    ev("deserved_le_at_tolerance")
            keeps.append(keep)
    except RefPanic:
        return PANIC
    victims = [k for k in pre if all(k in keep for keep in keeps)]  # session_plugins.go:59-140
    if victims_out is not None:
        victims_out[:] = victims
    if not victims:
        return NONE
    total = [0, 0, 0]  # validateVictims
    for k in (pre if defect == "sum_preemptees" else victims):
        for d in range(3):
            total[d] = total[d] + req(k)[d]
    if less(total, s.req):
        ev("validate_sum_less")
        return NONE
    if sum(not total[d] < s.req[d] for d in range(3)) == 1:
        ev("validate_one_dim_not_less")
    return STOP


# ------------------------------------------------------------------ layout
def big_rows(c):
    """Table rows of the range the big-node kernel evaluates (kbg_victims.ipp
    vt_setup): 129..MAX_NODE_CANDIDATES candidates."""
    lo, nn = c.p["node_lo"], c.p["node_n"]
    cnt = np.diff(c.nt_off)[lo:lo + nn]
    return [int(r) for r in np.flatnonzero((cnt > 128) & (cnt <= MAX_NODE_CANDIDATES))]


def verdicts(c, defect=None, prep=True, events=None, num=float, victims=None):
    """evaluate() of every node of the scanned range, by node; `victims`
    receives each node's victim list."""
    s = state(c, prep, num)
    lo = c.p["node_lo"]
    out = {}
    for n in range(lo, lo + c.p["node_n"]):
        v = []
        out[n] = evaluate(c, s, n, defect, events, v)
        if victims is not None:
            victims[n] = v
    return out


def victim_words(n_nodes):
    return (n_nodes + 31) // 32


def expected(c, out_mode, defect=None, prep=True):
    """The probe's raw outputs (bytes, guards included) after a run that
    started from sentinel-filled words. Bytes [node_lo / 8, node_lo / 8 +
    ceil(node_n / 8)) of each map hold the range's bits (0 past its end),
    every other byte keeps the sentinel. out_mode 0 (mapped): the big nodes'
    verdicts are row_out's n_rows bytes (bit 0 stop, bit 1 panic) and their
    map bits stay 0; out_mode 1 (device): they are ORed into the maps and
    row_out is not written. Nodes holding more than MAX_NODE_CANDIDATES
    candidates report nothing."""
    p = c.p
    v = verdicts(c, defect, prep)
    lo, nn = p["node_lo"], p["node_n"]
    cnt = np.diff(c.nt_off)
    wb = victim_words(p["n_nodes"]) * 4
    stop = np.full(wb + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    panic = stop.copy()
    b0, nb = lo // 8, (nn + 7) // 8
    if defect != "stale_byte":
        stop[b0:b0 + nb] = 0
        panic[b0:b0 + nb] = 0
    rows = big_rows(c)
    row_out = np.full(len(rows) + GUARD_BYTES, SENTINEL, dtype=np.uint8)
    for n in range(lo, lo + nn):
        if cnt[n] > MAX_NODE_CANDIDATES or v[n] == NONE:
            continue
        if cnt[n] > 128 and out_mode == 0:
            continue
        at = n - lo if defect == "big_wrong_word" and cnt[n] > 128 else n
        stop[at >> 3] |= 1 << (at & 7)
        if v[n] == PANIC:
            panic[at >> 3] |= 1 << (at & 7)
    if out_mode == 0:
        for i, r in enumerate(rows):
            row_out[i] = (0, 1, 3)[v[lo + r]]
    return SimpleNamespace(stop=stop, panic=panic, row_out=row_out)


def prepped_tables(c):
    """What the probe returns of the tables after the prep: the node table
    block, c_run, j_ready, j_alloc, q_alloc. Entries no delta names keep
    their value."""
    f, i = c.node_f.copy(), np.stack([c.ntasks, c.maxtasks]).astype(np.int32)
    c_run, j_ready = c.c_run.copy(), c.j_ready.copy()
    j_alloc, q_alloc = c.j_alloc.copy(), c.q_alloc.copy()
    for d in c.nd[:c.p["nn"]]:
        f[0:3, d["node"]] = d["idle"]
        f[3:6, d["node"]] = d["rel"]
        i[0, d["node"]] = d["ntasks"]
        i[1, d["node"]] = d["maxtasks"]
    for d in c.sd[:c.p["ns"]]:
        k, x = int(d["kind"]), int(d["index"])
        if k == 0:
            c_run[x] = d["v"][0] != 0.0
        elif k == 1:
            j_ready[x] = int(d["v"][0])
        elif k == 2:
            j_alloc[x] = d["v"]
        else:
            q_alloc[x] = d["v"]
    return SimpleNamespace(block=np.frombuffer(f.tobytes() + i.tobytes(), dtype=np.uint8).copy(), c_run=c_run,
                           j_ready=j_ready, j_alloc=j_alloc, q_alloc=q_alloc)


def table_block(c):
    return np.frombuffer(c.node_f.tobytes() + np.stack([c.ntasks, c.maxtasks]).astype(np.int32).tobytes(),
                         dtype=np.uint8).copy()


def compare(c, exp, stop, panic, row_out):
    """Readable differences between a probe's raw outputs and `exp`."""
    errs = []
    lo, nn = c.p["node_lo"], c.p["node_n"]
    wb = victim_words(c.p["n_nodes"]) * 4
    cnt = np.diff(c.nt_off)
    for name, got, want in (("stop", stop, exp.stop), ("panic", panic, exp.panic)):
        for b in np.flatnonzero(got != want)[:8]:
            b = int(b)
            if b >= wb:
                errs.append(f"{name}: guard byte {b - wb} overwritten ({int(got[b]):#x})")
            elif not lo // 8 <= b < lo // 8 + (nn + 7) // 8:
                errs.append(f"{name}: byte {b} outside the range's bytes is {int(got[b]):#x}, not the sentinel")
            else:
                for bit in range(8):
                    if (int(got[b]) ^ int(want[b])) >> bit & 1:
                        n = 8 * b + bit
                        what = f"node {n} ({int(cnt[n])} candidates)" if n < lo + nn else \
                            f"bit of node {n} past the range"
                        errs.append(f"{name}: {what}: device {int(got[b]) >> bit & 1}, "
                                    f"reference {int(want[b]) >> bit & 1}")
    rows = big_rows(c)
    for i in np.flatnonzero(row_out != exp.row_out)[:8]:
        i = int(i)
        if i >= len(rows):
            errs.append(f"row_out: guard byte {i - len(rows)} overwritten ({int(row_out[i]):#x})")
        else:
            errs.append(f"row_out[{i}] (node {lo + rows[i]}, {int(cnt[lo + rows[i]])} candidates): device "
                        f"{int(row_out[i]):#x}, reference {int(exp.row_out[i]):#x}")
    return errs


# ------------------------------------------------------------------- cases
R1 = (1000, 1024 * MI, 1000)  # the hand-made nodes' usual request
BIG = (10 ** 9, 10 ** 15, 10 ** 9)


class Builder:
    """Accumulates one case: job and queue tables, then nodes as lists of
    candidates (job, request, running). Job 0 in queue 0 is the preemptor's."""

    def __init__(self, mode, fns, n_tiers=1, req=(300, 300 * MI, 300), ls=0.0, total=(2 ** 24, 2 ** 44, 2 ** 24)):
        self.mode, self.fns, self.n_tiers = mode, fns, n_tiers
        self.req, self.ls, self.total = req, ls, total
        self.jobs, self.queues, self.nodes = [], [], []
        self.queue()
        self.job(0)

    def queue(self, alloc=BIG, deserved=(0, 0, 0)):
        self.queues.append(dict(alloc=list(alloc), deserved=list(deserved)))
        return len(self.queues) - 1

    def job(self, queue, jmin=1, ready=5, alloc=BIG):
        self.jobs.append(dict(queue=queue, min=jmin, ready=ready, alloc=list(alloc)))
        return len(self.jobs) - 1

    def node(self, cands, ntasks=1, maxtasks=110, panic=0, classbit=1):
        """cands: (job, request) or (job, request, running)."""
        self.nodes.append(dict(cands=[(c[0], tuple(c[1]), c[2] if len(c) > 2 else 1) for c in cands], ntasks=ntasks,
                               maxtasks=maxtasks, panic=panic, classbit=classbit))
        return len(self.nodes) - 1

    def finish(self, name, seed, node_lo=0, node_n=None, W=None, cls=0, classes=1, cap_check=1, prep=0, nd=None,
               sd=None):
        rng = np.random.default_rng(seed)
        n_nodes = len(self.nodes)
        W = W or (n_nodes + 63) // 64
        node_n = n_nodes - node_lo if node_n is None else node_n
        stride = node_n + 2
        c = SimpleNamespace(name=name)
        cnt = [len(nd_["cands"]) for nd_ in self.nodes]
        c.nt_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        P = int(c.nt_off[-1])
        flat = [x for nd_ in self.nodes for x in nd_["cands"]]
        c.c_jq = np.zeros((max(P, 1), 2), dtype=np.int32)
        c.c_req = np.zeros((max(P, 1), 3), dtype=np.float64)
        c.c_run = np.zeros(max(P, 1), dtype=np.uint8)
        for k, (j, r, run) in enumerate(flat):
            c.c_jq[k] = (j, self.jobs[j]["queue"])
            c.c_req[k] = r
            c.c_run[k] = run
        c.j_min = np.array([j["min"] for j in self.jobs], dtype=np.int32)
        c.j_ready = np.array([j["ready"] for j in self.jobs], dtype=np.int32)
        c.j_alloc = np.array([j["alloc"] for j in self.jobs], dtype=np.float64)
        c.q_alloc = np.array([q["alloc"] for q in self.queues], dtype=np.float64)
        c.q_deserved = np.array([q["deserved"] for q in self.queues], dtype=np.float64)
        c.dbl = np.array(list(self.req) + [self.ls] + list(self.total), dtype=np.float64)
        c.panic_node = np.array([nd_["panic"] for nd_ in self.nodes], dtype=np.uint8)
        # rows of the table block are nodes node_lo ..; the rows past node_n are never read
        c.ntasks = rng.integers(0, 5, size=stride).astype(np.int32)
        c.maxtasks = rng.integers(0, 5, size=stride).astype(np.int32)
        for r in range(node_n):
            c.ntasks[r] = self.nodes[node_lo + r]["ntasks"]
            c.maxtasks[r] = self.nodes[node_lo + r]["maxtasks"]
        c.node_f = np.floor(rng.random((6, stride)) * 1e6)
        bits = np.ones((classes, W * 64), dtype=bool)  # garbage past n_nodes; the other classes random
        for k in range(classes):
            bits[k, :n_nodes] = rng.random(n_nodes) < 0.5
        bits[cls, :n_nodes] = [nd_["classbit"] for nd_ in self.nodes]
        c.class_mask = pack_words(bits).reshape(classes, W)
        c.nd = np.zeros(1, dtype=NODE_DELTA) if nd is None else nd
        c.sd = np.zeros(1, dtype=STATE_DELTA) if sd is None else sd
        c.p = dict(n_nodes=n_nodes, W=W, cls=cls, cap_check=cap_check, node_lo=node_lo, node_n=node_n, mode=self.mode,
                   n_tiers=self.n_tiers, tier_fns=self.fns, job=0, queue=0, stride=stride, classes=classes, n_cand=P,
                   n_jobs=len(self.jobs), n_queues=len(self.queues), prep=prep,
                   nn=0 if nd is None else len(nd), ns=0 if sd is None else len(sd))
        c.p["n_rows"] = len(big_rows(c))
        return c


CPU_POOL = (100, 250, 500, 1000, 2000)
MEM_POOL = (64 * MI, 128 * MI, 256 * MI, 512 * MI, 1024 * MI)
GPU_POOL = (100, 500, 1000, 2000)
RANDOM_L = (0, 1, 2, 3, 5, 8, 13, 30, 63, 64, 65, 100, 127, 128)


def rand_req(rng):
    return (int(rng.choice(CPU_POOL)), int(rng.choice(MEM_POOL)), int(rng.choice(GPU_POOL)))


def random_builder(rng, mode, fns, counts, n_tiers=1, zero_gpu_total=False):
    """A session-like case: 4 queues, 10 jobs, nodes of `counts` candidates
    with mixed requests. The job and queue allocations are set from the
    largest per-node sum of each job's / queue's preemptee requests, so that
    the fns' running subtractions cross their thresholds (and, for a few,
    underflow) part of the way through a node's list."""
    b = Builder(mode, fns, n_tiers)
    for _ in range(3):
        b.queue()
    gaps = (0, 1, 1, 2, 5, 0, 1, 3, 1)  # ready - min
    for i in range(9):
        jmin = int(rng.integers(1, 6))
        b.job(queue=(0, 0, 0, 1, 1, 2, 2, 3, 3)[i], jmin=jmin, ready=jmin + gaps[i])
    weights = {VM_PREEMPT_JOBS: [1, 3, 3, 3, .5, .5, .5, .5, .5, .5],
               VM_PREEMPT_TASKS: [8, 1, 1, 1, .5, .5, .5, .5, .5, .5],
               VM_RECLAIM: [1, 1, .5, .5, 2, 2, 2, 2, 2, 2]}[mode]
    weights = np.array(weights) / sum(weights)
    for L in counts:
        # a node holds the tasks of a few jobs: one dominant job, the others mixed in
        w = weights.copy()
        w[int(rng.integers(1 if mode != VM_PREEMPT_TASKS else 0, 10))] += 1.0
        w /= w.sum()
        jobs = rng.choice(10, size=L, p=w)
        run = rng.random(L) >= 0.1
        b.node([(int(j), rand_req(rng), int(r)) for j, r in zip(jobs, run)], ntasks=int(rng.integers(0, 4)),
               maxtasks=int(rng.integers(2, 5)), panic=int(rng.random() < 0.04), classbit=int(rng.random() < 0.85))
    p = dict(mode=mode, job=0, queue=0)
    jsum, qsum = np.zeros((10, 3)), np.zeros((4, 3))
    for nd_ in b.nodes:
        js, qs = np.zeros((10, 3)), np.zeros((4, 3))
        for j, r, run in nd_["cands"]:
            if run and is_preemptee(p, j, b.jobs[j]["queue"]):
                js[j] += r
                qs[b.jobs[j]["queue"]] += r
        jsum, qsum = np.maximum(jsum, js), np.maximum(qsum, qs)
    # slack over the largest node's sum: none, within the Sub tolerance below it, beyond it (a panic
    # on that node), and comfortable
    slack = [(0, 0, 0), (-5, -5 * MI, -5), (-5, 0, 0), (2000, 2048 * MI, 2000), (2000, 2048 * MI, 2000),
             (-1000, 0, 0), (5000, 0, 5000), (0, 0, 0), (2000, 2048 * MI, 2000), (10000, 10240 * MI, 10000)]
    for j in range(10):
        b.jobs[j]["alloc"] = [max(0.0, jsum[j][d] + slack[j][d]) for d in range(3)]
    qslack = [(0, 0, 0), (2000, 2048 * MI, 2000), (-5, -5 * MI, 0), (-1000, -1024 * MI, -1000)]
    frac = (0.5, 0.3, 0.7, 1.0)
    for q in range(4):
        b.queues[q]["alloc"] = [max(0.0, qsum[q][d] + qslack[q][d]) for d in range(3)]
        b.queues[q]["deserved"] = [float(int(b.queues[q]["alloc"][d] * frac[q])) for d in range(3)]
    amax = np.array([j["alloc"] for j in b.jobs]).max(axis=0)
    b.total = tuple(float(4 * max(1.0, v)) for v in amax)
    if zero_gpu_total:
        b.total = (b.total[0], b.total[1], 0.0)
    half = [share([b.jobs[j]["alloc"][d] - jsum[j][d] / 2 for d in range(3)], b.total) for j in range(1, 10)
            if jsum[j].any()]
    b.ls = float(np.median(half)) if half else 0.1
    b.req = (int(rng.choice((300, 1000, 4000))), int(rng.choice((300, 1024, 4096))) * MI,
             int(rng.choice((300, 1000, 4000))))
    return b


def rand_counts(rng, n_nodes, must=()):
    counts = [int(rng.choice(RANDOM_L)) for _ in range(n_nodes)]
    for i, L in zip(rng.permutation(n_nodes)[:len(must)], must):
        counts[int(i)] = L
    return counts


def mixed(rng, L):
    return [rand_req(rng) for _ in range(L)]


def rsum(reqs):
    return tuple(sum(r[d] for r in reqs) for d in range(3))


def radd(a, b, sign=1):
    return tuple(a[d] + sign * b[d] for d in range(3))


def chunk_nodes(b, rng, L):
    """Two nodes of L candidates of one queue under gang + proportion whose
    last candidate is the only one gang keeps, with proportion's verdict on
    it resting on every earlier subtraction: the queue's allocation is
    deserved + the others' sum (the last one falls short of deserved: NONE)
    or deserved + everyone's sum (it is a victim: STOP); and a third node
    where the last Sub underflows (PANIC)."""
    des = (5000, 5000 * MI, 5000)
    for kind in ("none", "stop", "panic"):
        reqs = mixed(rng, L - 1) + [R1]
        if kind == "none":
            alloc = radd(des, rsum(reqs[:-1]))
        elif kind == "stop":
            alloc = radd(des, rsum(reqs))
        else:
            alloc = radd(rsum(reqs), (20, 0, 0), -1)  # (short in one dimension only: not Less, no skip)
        q = b.queue(alloc, BIG if kind == "panic" else des)
        held, last = b.job(q, jmin=3, ready=3), b.job(q, jmin=3, ready=4)
        b.node([(held, r) for r in reqs[:-1]] + [(last, reqs[-1])])


def drf_chunk_case(L, seed):
    """Job preemption under drf alone, three nodes with the same L mixed
    requests, each a job of its own; the preemptor asks for exactly their
    sum, so validateVictims passes only if all L are victims. ls = 1/4 of
    totals 2^24 / 2^44 / 2^24: the job whose allocation ends at a share of
    1/4 stops, the one ending 17 / 2^24 below it loses its last candidate
    (NONE), the third one's last Sub underflows (PANIC)."""
    rng = np.random.default_rng(seed)
    reqs = mixed(rng, L)
    tot = rsum(reqs)
    b = Builder(VM_PREEMPT_JOBS, VP_DRF, req=tot, ls=0.25)
    for alloc in ((2 ** 22 + tot[0] - 17, tot[1], tot[2]), (2 ** 22 + tot[0], tot[1], tot[2]),
                  (tot[0] - 20, tot[1], tot[2])):
        j = b.job(0, alloc=alloc)
        b.node([(j, r) for r in reqs])
    return b.finish(f"edge-drf-chunks-L{L}", seed)


def edge_prop():
    """Reclaim under proportion alone, hand-made nodes (request 300 / 300 Mi / 300)."""
    b = Builder(VM_RECLAIM, VP_PROP)

    def one(alloc, deserved, cands, **kw):
        q = b.queue(alloc, deserved)
        j = b.job(q)
        return b.node([(j,) + tuple(c) for c in cands], **kw)

    n = {}
    # Less in all three dimensions: the first is skipped and must not subtract; the second is a victim
    n["skip"] = one((500, 512 * MI, 500), (0, 0, 0), [(R1,), ((400, 400 * MI, 400),)])
    # one dimension equal, the others short within the Sub tolerance: subtracted, a victim
    n["eq_noskip"] = one((1000, 1019 * MI, 995), (0, 0, 0), [(R1,)])
    # one dimension equal, another short beyond the tolerance: Sub panics
    n["prop_panic"] = one((1000, 1004 * MI, 1000), (0, 0, 0), [(R1,)])
    # deserved 9 above the allocation (inside LessEqual's tolerance) and 10 above it (outside)
    n["des_in"] = one((3000, 4096 * MI, 3000), (2009, 0, 0), [(R1,)])
    n["des_out"] = one((3000, 4096 * MI, 3000), (2010, 0, 0), [(R1,)])
    # validateVictims: 200 / 200 Mi / 200 is Less than the request; 200 / 200 Mi / 300 is not, in one dimension
    n["val_less"] = one(BIG, (0, 0, 0), [((100, 100 * MI, 100),)] * 2)
    n["val_one_dim"] = one(BIG, (0, 0, 0), [((100, 100 * MI, 150),)] * 2)
    # a task no longer Running ahead of a Running one of the same queue: had it subtracted, the second
    # would fall short of deserved
    n["not_running"] = one((6950, 6144 * MI, 6000), (5000, 5000 * MI, 5000),
                           [((100, 100 * MI, 100), 0), (R1,)])
    # panic nodes: outside the class (nothing), inside it with no candidate (panic)
    n["panic_class_off"] = one(BIG, (0, 0, 0), [(R1,)], panic=1, classbit=0)
    n["panic_empty"] = b.node([], panic=1)
    n["stop_plain"] = one(BIG, (0, 0, 0), [(R1,)])
    n["cap_equal"] = one(BIG, (0, 0, 0), [(R1,)], ntasks=7, maxtasks=7)
    return b, n


def edge_drf():
    """Job preemption under drf alone with a zero GPU total: shares are exact
    binary fractions (totals 2^24 and 2^34), ls = 1/4."""
    b = Builder(VM_PREEMPT_JOBS, VP_DRF, ls=0.25, total=(2 ** 24, 2 ** 34, 0))
    q = 2 ** 22  # a quarter of the CPU total

    def one(alloc, cands):
        j = b.job(0, alloc=alloc)
        return b.node([(j,) + tuple(c) for c in cands])

    n = {}
    n["gpu_left"] = one((2000, 2048 * MI, 1500), [(R1,)])  # GPU allocation stays nonzero: share 1
    n["lt"] = one((q + 2000, 2048 * MI, 1000), [(R1,)])  # ls < rs, GPU allocation becomes exactly 0
    n["close_in"] = one((q - 16 + 1000, 2048 * MI, 1000), [(R1,)])  # |ls - rs| = 16 / 2^24 < 1e-6
    n["close_out"] = one((q - 17 + 1000, 2048 * MI, 1000), [(R1,)])  # 17 / 2^24 > 1e-6
    n["neg_ok"] = one((995, 2 ** 33 + 1024 * MI, 1000), [(R1,)])  # CPU goes to -5: inside Sub's tolerance
    n["neg_panic"] = one((980, 2 ** 33 + 1024 * MI, 1000), [(R1,)])  # -20: panic
    # a task of the same job that is no longer Running must not subtract: with it the share would
    # fall below ls
    n["not_running"] = one((q + 1500, 2048 * MI, 1400), [((1000, 64 * MI, 400), 0), (R1,)])
    other = b.job(b.queue())  # another queue's task on the node: filtered out
    b.nodes[-1]["cands"].append((other, R1, 1))
    return b, n


def edge_gang():
    b = Builder(VM_PREEMPT_JOBS, VP_GANG)
    yes, no = b.job(0, jmin=3, ready=4), b.job(0, jmin=3, ready=3)
    n = {"yes": b.node([(yes, R1)]), "no": b.node([(no, R1)]), "mixed": b.node([(no, R1), (yes, R1), (0, R1)])}
    return b, n


def state_deltas(c, rng, ns):
    """ns distinct (kind, index) deltas of all four kinds that move the fns'
    inputs: running flags flipped, readiness at or just above MinAvailable,
    allocations scaled."""
    sd = np.zeros(ns, dtype=STATE_DELTA)
    J, Q, P = c.p["n_jobs"], c.p["n_queues"], c.p["n_cand"]
    picks = [(1, j) for j in rng.permutation(J)[:min(J, max(1, ns // 8))]]
    picks += [(2, j) for j in rng.permutation(J)[:min(J, max(1, ns // 8))]]
    picks += [(3, q) for q in rng.permutation(Q)[:min(Q, max(1, ns // 16))]]
    picks = picks[:max(0, ns - 1)]
    picks += [(0, k) for k in rng.permutation(P)[:ns - len(picks)]]
    assert len(picks) == ns
    for d, (kind, i) in zip(sd, [picks[x] for x in rng.permutation(ns)]):
        d["kind"], d["index"] = kind, i
        if kind == 0:
            d["v"] = (float(not c.c_run[i]), 7.0, -1.0)  # only v[0] is read
        elif kind == 1:
            d["v"] = (float(c.j_min[i] + (0 if c.j_ready[i] > c.j_min[i] else 1)), 0.0, 0.0)
        else:
            src = c.j_alloc[i] if kind == 2 else c.q_alloc[i]
            d["v"] = np.floor(src * rng.choice((0.9, 1.5, 2.0)))
    return sd


def node_deltas(c, rng, nn):
    nd = np.zeros(nn, dtype=NODE_DELTA)
    rows = np.concatenate([[0, c.p["stride"] - 1], rng.permutation(np.arange(1, c.p["stride"] - 1))])[:nn]
    nd["node"] = rng.permutation(rows)
    nd["maxtasks"] = rng.integers(1, 4, size=nn)
    nd["ntasks"] = nd["maxtasks"] - rng.integers(0, 3, size=nn)  # at the pod cap or just below it
    nd["idle"] = np.floor(rng.random((nn, 3)) * 1e9)
    nd["rel"] = np.floor(rng.random((nn, 3)) * 1e6)
    nd["pad"] = 0
    return nd


def with_prep(c, seed, prep, nn, ns):
    rng = np.random.default_rng(seed)
    c.nd = node_deltas(c, rng, nn) if nn else np.zeros(1, dtype=NODE_DELTA)
    c.sd = state_deltas(c, rng, ns) if ns else np.zeros(1, dtype=STATE_DELTA)
    c.p.update(prep=prep, nn=nn, ns=ns)
    return c


NODE_COUNTS = (1, 7, 8, 9, 63, 64, 65, 200, 33)
BOUNDARY_L = (0, 1, 63, 64, 65, 127, 128)


def _combo(mode, fns):
    i = mode * 7 + fns - 1
    n_nodes = NODE_COUNTS[i % len(NODE_COUNTS)]
    rng = np.random.default_rng(7000 + i)
    b = random_builder(rng, mode, fns, rand_counts(rng, n_nodes, BOUNDARY_L if n_nodes >= 63 else (63, 64, 65, 128)))
    return b.finish(f"m{mode}-f{fns}-n{n_nodes}", 100 + i, W=(n_nodes + 63) // 64 + (i % 3 == 0))


def _no_tier():
    rng = np.random.default_rng(7100)
    b = random_builder(rng, VM_RECLAIM, 0, rand_counts(rng, 40), n_tiers=0)
    return b.finish("no-tier", 7100)


def _shard(lo, n_nodes, node_n, mode, fns, seed, big=()):
    rng = np.random.default_rng(seed)
    counts = rand_counts(rng, n_nodes, BOUNDARY_L)
    inside = [int(x) for x in lo + rng.permutation(node_n)[:len(big)]]
    for n, L in zip(inside, big):
        counts[n] = L
    if big:  # big nodes outside the shard's range are not among its rows
        counts[0], counts[n_nodes - 1] = 150, 300
    b = random_builder(rng, mode, fns, counts)
    return b.finish(f"shard{lo}-{node_n}of{n_nodes}" + ("-big" if big else ""), seed, node_lo=lo, node_n=node_n, W=4,
                    cls=2, classes=3)


def _big(name, seed, mode, fns, bigs, n_nodes=12, at=None, zero_gpu_total=False, req_frac=None):
    rng = np.random.default_rng(seed)
    counts = [int(rng.choice((0, 3, 64, 128))) for _ in range(n_nodes)]
    for n, L in zip(at or range(1, 1 + len(bigs)), bigs):
        counts[n] = L
    b = random_builder(rng, mode, fns, counts, zero_gpu_total=zero_gpu_total)
    for n, L in enumerate(counts):
        if L > 128:  # the big nodes are the point: inside the class, below the pod cap, no nil node
            b.nodes[n].update(panic=0, classbit=1, ntasks=1, maxtasks=110)
    if req_frac:  # a request so large that validateVictims turns on the victims' exact sum
        b.req = tuple(float(int(v * req_frac)) for v in rsum([r for _, r, _ in b.nodes[1]["cands"]]))
    return b.finish(name, seed)


def _edge_chunks(name, Ls, seed):
    rng = np.random.default_rng(seed)
    b = Builder(VM_RECLAIM, VP_GANG | VP_PROP)
    for L in Ls:
        chunk_nodes(b, rng, L)
    return b.finish(name, seed)


def _cap(cap_check):
    b, _ = edge_prop()
    return b.finish(f"edge-prop-cap{cap_check}", 11, cap_check=cap_check)


@functools.lru_cache(maxsize=None)
def _cases():
    cs = [_combo(m, f) for m in range(3) for f in range(1, 8)]
    cs.append(_no_tier())
    cs += [_cap(1), _cap(0)]
    cs.append(edge_drf()[0].finish("edge-drf", 12))
    cs.append(edge_gang()[0].finish("edge-gang", 13))
    # chunk boundaries of the main scan (second chunk: lane 0, lane 63) and of the big-node kernel
    # (chunk 15: lane 0, lane 63; chunk 2 lane 0)
    cs.append(_edge_chunks("edge-chunks-main", (65, 128), 14))
    cs.append(_edge_chunks("edge-chunks-big", (129, 961, 1024), 15))
    cs += [drf_chunk_case(L, 16 + i) for i, L in enumerate((65, 128, 129, 961, 1024))]
    cs.append(_shard(64, 200, 61, VM_RECLAIM, 7, 7200))
    cs.append(_shard(128, 200, 67, VM_PREEMPT_JOBS, 3, 7201))
    cs.append(_shard(64, 200, 93, VM_RECLAIM, 6, 7202, big=(129, 193, 1024)))
    cs.append(_big("big-rows1", 7300, VM_RECLAIM, 7, (1023,)))
    cs.append(_big("big-rows4", 7301, VM_PREEMPT_JOBS, 3, (129, 192, 193, 1024)))
    # five rows (a second workgroup of one wave), all in one 32-bit word, and a node past the bound
    cs.append(_big("big-rows5", 7302, VM_RECLAIM, 6, (129, 192, 1023, 1024, 193, 1025), n_nodes=40,
                   at=(33, 34, 35, 36, 38, 37)))
    cs.append(_big("big-tasks", 7303, VM_PREEMPT_TASKS, 3, (500, 1024), zero_gpu_total=True))
    cs.append(_big("big-validate", 7305, VM_RECLAIM, 6, (600, 1024, 900), req_frac=0.5))
    cs.append(_big("big-rows9-200", 7304, VM_RECLAIM, 5, (129, 130, 191, 192, 193, 256, 257, 700, 1024), n_nodes=200,
                   at=(0, 31, 32, 63, 64, 65, 127, 128, 199)))
    # prep: the argument-carried path at its capacity, with ns == 0 and with nn == 0; the host-mapped
    # path with the node / state split inside the first workgroup and the total past 256, and with
    # nn == 0
    mk = lambda i, mode, fns, n: random_builder(np.random.default_rng(7400 + i), mode, fns,
                                                rand_counts(np.random.default_rng(7450 + i), n, BOUNDARY_L))
    cs.append(with_prep(mk(0, VM_RECLAIM, 7, 70).finish("prep-inline-16-48", 7400), 7500, 1, 16, 48))
    cs.append(with_prep(mk(1, VM_PREEMPT_JOBS, 3, 20).finish("prep-inline-ns0", 7401), 7501, 1, 9, 0))
    cs.append(with_prep(mk(2, VM_RECLAIM, 5, 20).finish("prep-inline-nn0", 7402), 7502, 1, 0, 20))
    cs.append(with_prep(mk(3, VM_RECLAIM, 7, 130).finish("prep-mapped-100-200", 7403), 7503, 2, 100, 200))
    cs.append(with_prep(mk(4, VM_PREEMPT_TASKS, 3, 30).finish("prep-mapped-nn0", 7404), 7504, 2, 0, 40))
    cs.append(with_prep(mk(5, VM_PREEMPT_JOBS, 1, 30).finish("prep-mapped-ns0", 7405), 7505, 2, 30, 0))
    return {c.name: c for c in cs}


def case(name):
    return _cases()[name]


NAMES = list(_cases())
