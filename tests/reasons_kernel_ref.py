"""Plain references and seeded inputs for the two kernels behind the
per-predicate unschedulable reasons (kbg_kernels.hip kbg_stage_mask_kernel,
kbg_reasons_kernel; kbg_device.hpp StagePlanes, ReasonArgs), launched alone
through the probes of the tool library (tests/test_reasons_kernels_gpu.py).
The references are direct loops over numpy inputs; tests/test_reasons_kernel_ref.py
checks them on the CPU against hand-made inputs with known answers."""
import numpy as np

from kernel_ref import FIT_QUERY, GUARD_BYTES, sentinel_words

REQ_PROG = np.dtype([("kind", "<i4"), ("mask_off", "<i4"), ("col", "<i4"), ("pad", "<i4"), ("value", "<i8")])
TERM_PROG = np.dtype([("req_off", "<i4"), ("req_len", "<i4")])
CLASS_PROG = np.dtype([("sel_req", "<i4"), ("has_affinity", "<i4"), ("term_off", "<i4"), ("term_len", "<i4"),
                       ("tol_off", "<i4"), ("always", "<i4")])
REQ_FALSE, REQ_TRUE, REQ_ALL, REQ_ANY, REQ_NONE, REQ_GT, REQ_LT, REQ_NAME_EQ, REQ_NAME_NE = range(9)
NF_UNSCHED, NF_NIL, NF_DEAD = 1, 2, 4
REASON_OUT = 16  # words per query: visited, count[6], first_node[6], 3 unused
WHY_POD_CAP, WHY_SELECTOR, WHY_HOST_PORTS, WHY_UNSCHEDULABLE, WHY_TAINTS, WHY_POD_AFFINITY = range(6)


def bit(words, n):
    return (int(words[n >> 6]) >> (n & 63)) & 1


def pack(bits, W):
    out = np.zeros(W, dtype=np.uint64)
    for n in np.flatnonzero(bits):
        out[n >> 6] |= np.uint64(1 << (int(n) & 63))
    return out


# ------------------------------------------------------------- stage planes
def eval_req(t, r, n):
    k = int(r["kind"])
    if k in (REQ_FALSE, REQ_TRUE):
        return k == REQ_TRUE
    if k in (REQ_ALL, REQ_ANY, REQ_NONE):
        any_, all_ = False, True
        for w in range(t["label_words"]):
            m = int(t["mask_pool"][int(r["mask_off"]) + w])
            b = int(t["label_bits"][w, n]) & m
            any_ |= b != 0
            all_ &= b == m
        return all_ if k == REQ_ALL else (any_ if k == REQ_ANY else not any_)
    if k in (REQ_GT, REQ_LT):
        if not t["num_ok"][int(r["col"]), n]:
            return False
        v = int(t["num_vals"][int(r["col"]), n])
        return v > int(r["value"]) if k == REQ_GT else v < int(r["value"])
    return (int(t["name_id"][n]) == int(r["value"])) == (k == REQ_NAME_EQ)


def stage_reference(t):
    """(sel_ok [C][W], taint_ok [C][W], unsched [W], live [W], class_mask [C][W])
    of the static tables `t`: every stage on its own; class_mask as
    kbg_mask_kernel folds them (nil first, then unschedulable / deleted)."""
    N, W, C = t["n_nodes"], t["W"], len(t["classes"])
    sel, tol, cm = (np.zeros((C, N), dtype=bool) for _ in range(3))
    uns, live = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    for n in range(N):
        fl = int(t["node_flags"][n])
        nil = bool(fl & NF_NIL)
        live[n] = nil or not fl & NF_DEAD
        uns[n] = not nil and bool(fl & NF_UNSCHED)
        for c, cp in enumerate(t["classes"]):
            s = o = True
            if not cp["always"] and not nil:
                if cp["sel_req"] >= 0:
                    s = eval_req(t, t["reqs"][int(cp["sel_req"])], n)
                if s and cp["has_affinity"]:
                    s = any(all(eval_req(t, t["reqs"][int(tp["req_off"]) + j], n) for j in range(int(tp["req_len"])))
                            for tp in t["terms"][int(cp["term_off"]):int(cp["term_off"]) + int(cp["term_len"])])
                o = all(not int(t["taint_bits"][w, n]) & ~int(t["tol_pool"][int(cp["tol_off"]) + w])
                        for w in range(t["taint_words"]))
            sel[c, n], tol[c, n] = s, o
            cm[c, n] = True if cp["always"] or nil else (not fl & (NF_UNSCHED | NF_DEAD)) and s and o
    pk = lambda m: np.stack([pack(r, W) for r in m])  # noqa: E731
    return pk(sel), pk(tol), pack(uns, W), pack(live, W), pk(cm)


def stage_case(seed, n_nodes, classes=5):
    """Random static tables: two label words, one taint word, one numeric
    column, requirements of every kind, classes with a selector, with terms
    (some empty), with neither, and one `always`; node flags in every
    combination."""
    rng = np.random.default_rng(seed)
    N, W, LW = n_nodes, (n_nodes + 63) // 64, 2
    u64 = lambda *shape, p=0.5: np.packbits(rng.random(shape + (64,)) < p, axis=-1, bitorder="little").view("<u8")[..., 0]  # noqa: E731
    t = dict(n_nodes=N, W=W, label_words=LW, taint_words=1, n_numcols=1)
    t["label_bits"] = u64(LW, N)
    t["taint_bits"] = u64(1, N, p=0.03)
    t["num_vals"] = rng.integers(-5, 20, size=(1, N)).astype("<i8")
    t["num_ok"] = (rng.random((1, N)) < 0.8).astype(np.uint8)
    t["name_id"] = rng.permutation(N).astype("<i4")
    t["node_flags"] = rng.choice(np.array([0, 0, 0, 0, 1, 2, 4, 5, 3, 6], dtype=np.uint8), size=N)
    n_reqs = 24
    reqs = np.zeros(n_reqs, dtype=REQ_PROG)
    reqs["kind"] = np.concatenate([np.arange(9), rng.integers(0, 9, size=n_reqs - 9)])
    reqs["mask_off"] = rng.integers(0, 8, size=n_reqs) * LW
    reqs["value"] = rng.integers(0, 12, size=n_reqs)
    t["mask_pool"] = u64(8 * LW, p=0.04)
    t["reqs"] = reqs
    terms = np.zeros(8, dtype=TERM_PROG)
    terms["req_off"] = rng.integers(0, n_reqs - 3, size=8)
    terms["req_len"] = rng.integers(0, 4, size=8)
    t["terms"] = terms
    cl = np.zeros(classes, dtype=CLASS_PROG)
    cl["sel_req"] = rng.integers(-1, n_reqs, size=classes)
    cl["has_affinity"] = rng.integers(0, 2, size=classes)
    cl["term_off"] = rng.integers(0, 6, size=classes)
    cl["term_len"] = rng.integers(0, 3, size=classes)
    cl["tol_off"] = np.arange(classes)
    cl["always"][classes - 1] = 1
    cl["sel_req"][0], cl["has_affinity"][0] = -1, 0  # taints alone
    t["classes"] = cl
    t["tol_pool"] = u64(classes, p=0.7)
    return t


# ------------------------------------------------------------------ reasons
def reasons_reference(c):
    """kbg_reasons_kernel restated: per query the live nodes of [tab_lo,
    min(vend, tab_lo + tab_n)), vend = win + 1 when the task was placed (win >=
    0) else end, counted by the first failing stage — pod cap at the query's
    point (the final pod count less the node's decisions at or after it),
    selector, unschedulable, taints — for the nodes before `end`; with
    cap_check 0 (predicates off) only `visited` is counted."""
    p = c["p"]
    out = sentinel_words(p["nq"] * REASON_OUT + GUARD_BYTES // 4, "<i4")
    tab_end = p["tab_lo"] + p["tab_n"]
    for qi, q in enumerate(c["q"]):
        cls, end, win, point = int(q["cls"]), int(q["end"]), int(q["win"]), int(q["point"])
        vend = min(win + 1 if win >= 0 else end, tab_end)
        visited, count, first = 0, [0] * 6, [-1] * 6
        for n in range(p["tab_lo"], vend):
            if not bit(c["live"], n):
                continue
            visited += 1
            if not p["cap_check"] or n >= min(end, tab_end):
                continue
            undone = sum(1 for e in range(int(c["hoff"][n]), int(c["hoff"][n + 1]))
                         if (int(c["hk"][e]) & 0x7FFFFFFF) >= point)
            if int(c["ntasks"][n]) - undone >= int(c["maxtasks"][n]):
                k = WHY_POD_CAP
            elif not bit(c["sel_ok"][cls], n):
                k = WHY_SELECTOR
            elif bit(c["unsched"], n):
                k = WHY_UNSCHEDULABLE
            elif not bit(c["taint_ok"][cls], n):
                k = WHY_TAINTS
            else:
                continue
            if count[k] == 0:
                first[k] = n
            count[k] += 1
        out[qi * REASON_OUT:(qi + 1) * REASON_OUT] = [visited] + count + first + [0, 0, 0]
    return out


def reasons_case(seed, n_nodes, nq, cap_check=1, window=None, classes=3, max_dec=40):
    """Random planes, node records and queries. Nodes carry 0 .. max_dec
    decisions (most a few, some the maximum) so the binary search has work to
    do and the pod cap flips with the query's point. The queries: the first
    fits nowhere (every node), then placements and pipelines at nodes in the
    middle of a word, at a word's edge, at node 0 and at the last node, and
    one with end 0. The last class (`rare`, query 0's) passes the selector
    everywhere (a reason that appears nowhere) and fails the taints at the
    table's last node only, which is live, schedulable and below its cap."""
    rng = np.random.default_rng(seed)
    N, W = n_nodes, (n_nodes + 63) // 64
    lo, tn = window or (0, N)
    stride = max(64, (tn + 63) // 64 * 64)
    nd = np.where(rng.random(N) < 0.1, max_dec, rng.integers(0, 4, size=N))
    nd[rng.random(N) < 0.3] = 0
    hoff = np.concatenate([[0], np.cumsum(nd)]).astype("<i4")
    E = int(hoff[-1])
    owner = np.repeat(np.arange(N), nd)
    order = rng.permutation(E)  # decision indices are unique over the log, ascending within a node
    hk = np.zeros(E, dtype="<i4")
    for n in range(N):
        hk[hoff[n]:hoff[n + 1]] = np.sort(order[owner == n])
    hk = np.where(rng.random(E) < 0.2, hk | np.int32(-0x80000000), hk).astype("<i4")
    base = rng.integers(0, 3, size=N)
    ntasks = (base + nd).astype("<i4")
    maxtasks = np.where(rng.random(N) < 0.5, ntasks - rng.integers(0, 3, size=N), 110).astype("<i4")
    rand_plane = lambda pr: pack(rng.random(N) < pr, W)  # noqa: E731
    sel_ok = np.stack([rand_plane(0.7) for _ in range(classes)])
    taint_ok = np.stack([rand_plane(0.8) for _ in range(classes)])
    unsched, live = rand_plane(0.1), rand_plane(0.95)
    # the rare class (the last): passes every stage everywhere but the taints at the table's last node,
    # which is live, schedulable and below its cap whatever the point: TAINTS once, at the last lane
    rare, last = classes - 1, N - 1
    sel_ok[rare] = pack(np.ones(N, dtype=bool), W)
    taint_ok[rare] = pack(np.arange(N) != last, W)
    live[last >> 6] |= np.uint64(1 << (last & 63))
    unsched[last >> 6] &= ~np.uint64(1 << (last & 63))
    maxtasks[last] = 1 << 20
    picks = [(N, -1), (N // 2 + 7, N // 2 + 7), (min(N, 64), min(N, 64) - 1), (0, 0), (N, N - 1), (0, -1),
             (min(N - 1, 1024), min(N - 1, 1024))]
    q = np.zeros(nq, dtype=FIT_QUERY)
    for i in range(nq):
        end, win = picks[i % len(picks)] if i else picks[0]
        q[i]["cls"] = rare if i == 0 else int(rng.integers(0, classes))
        q[i]["end"], q[i]["win"] = end, win
        q[i]["point"] = int(rng.integers(0, E + 1)) if i else 0
    f = np.full((6, stride), 2.0 ** 52)
    i32 = np.zeros((2, stride), dtype="<i4")
    i32[1] = 1 << 30
    i32[0, :tn], i32[1, :tn] = ntasks[lo:lo + tn], maxtasks[lo:lo + tn]
    p = dict(n_nodes=N, W=W, stride=stride, classes=classes, tab_lo=lo, tab_n=tn, nq=nq, cap_check=cap_check, n_dec=E)
    return dict(p=p, block=f.tobytes() + i32.tobytes(), ntasks=ntasks, maxtasks=maxtasks, hoff=hoff, hk=hk, q=q,
                sel_ok=sel_ok, taint_ok=taint_ok, unsched=unsched, live=live, rare=rare,
                planes=np.concatenate([sel_ok.ravel(), taint_ok.ravel(), unsched, live]))


NODE_COUNTS = (63, 64, 65, 1024, 1025, 2100)
QUERY_COUNTS = (1, 2, 3, 5)
REASON_CASES = {f"n{n}-q{nq}-cap{cap}": dict(seed=9100 + 7 * i + nq, n_nodes=n, nq=nq, cap_check=cap)
                for i, n in enumerate(NODE_COUNTS) for nq in QUERY_COUNTS
                for cap in ((1, 0) if nq == 3 else (1,))}
REASON_CASES["n2100-q7-window"] = dict(seed=9300, n_nodes=2100, nq=7, window=(128, 1500))
