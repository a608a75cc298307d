"""The plain references of tests/reasons_kernel_ref.py on the CPU: hand-made
inputs with answers worked out by hand, and the seeded cases holding what
they claim (tests/test_reasons_kernels_gpu.py compares the kernels with these
references, so they are checked on their own first)."""
import numpy as np
import pytest

import reasons_kernel_ref as rr
from kernel_ref import FIT_QUERY, GUARD_BYTES, SENTINEL


def _hand_case(cap_check=1):
    """Five nodes, one class, decisions 0 .. 3 of one log:
    node 0: 2 of 2 pods, decisions 1 and 3 -> capped only if both are applied
    node 1: selector fails, cordoned           node 2: cordoned, taints fail
    node 3: taints fail                        node 4: deleted (not live)"""
    N, W = 5, 1
    c = dict(p=dict(n_nodes=N, W=W, stride=64, classes=1, tab_lo=0, tab_n=N, nq=0, cap_check=cap_check, n_dec=4))
    c["ntasks"] = np.array([2, 0, 0, 0, 0], dtype="<i4")
    c["maxtasks"] = np.array([2, 9, 9, 9, 9], dtype="<i4")
    c["hoff"] = np.array([0, 2, 3, 3, 4, 4], dtype="<i4")
    c["hk"] = np.array([1, 3 | -0x80000000, 0, 2], dtype="<i4")
    c["sel_ok"] = np.array([[0b11101]], dtype=np.uint64)
    c["taint_ok"] = np.array([[0b10011]], dtype=np.uint64)
    c["unsched"] = np.array([0b00110], dtype=np.uint64)
    c["live"] = np.array([0b01111], dtype=np.uint64)
    return c


def _rows(c, queries):
    q = np.zeros(len(queries), dtype=FIT_QUERY)
    for i, (end, win, point) in enumerate(queries):
        q[i]["end"], q[i]["win"], q[i]["point"] = end, win, point
    c["q"], c["p"]["nq"] = q, len(q)
    out = rr.reasons_reference(c)
    assert (out[len(q) * rr.REASON_OUT:].view(np.uint8) == SENTINEL).all() and \
        len(out) == len(q) * rr.REASON_OUT + GUARD_BYTES // 4
    return [(int(r[0]), r[1:7].tolist(), r[7:13].tolist()) for r in out[:len(q) * rr.REASON_OUT].reshape(-1, rr.REASON_OUT)]


def test_reasons_reference_by_hand():
    none = [-1] * 6
    rows = _rows(_hand_case(), [(5, -1, 4), (5, -1, 3), (5, -1, 0), (3, 3, 4), (3, 2, 4), (0, -1, 4), (0, 0, 4)])
    # every decision applied: node 0 at its cap; 1 selector (before cordoned), 2 cordoned (before taints), 3 taints
    assert rows[0] == (4, [1, 1, 0, 1, 1, 0], [0, 1, -1, 2, 3, -1])
    # decision 3 undone: node 0 holds 1 of 2 and passes every stage
    assert rows[1] == (4, [0, 1, 0, 1, 1, 0], [-1, 1, -1, 2, 3, -1])
    assert rows[2] == rows[1]
    # allocated at node 3 (end 3): node 3 is visited, its stages are not counted
    assert rows[3] == (4, [1, 1, 0, 1, 0, 0], [0, 1, -1, 2, -1, -1])
    # pipelined at node 2 (end 3 = win + 1): nodes 0 .. 2, all counted
    assert rows[4] == (3, [1, 1, 0, 1, 0, 0], [0, 1, -1, 2, -1, -1])
    assert rows[5] == (0, [0] * 6, none)
    assert rows[6] == (1, [0] * 6, none)  # allocated at node 0
    # predicates off: the visited nodes, no reason
    assert _rows(_hand_case(cap_check=0), [(5, -1, 4)]) == [(4, [0] * 6, none)]


def test_stage_reference_by_hand():
    """One label word, labels: node 0 {a}, node 1 {a, b}, node 2 {b}, node 3
    {a} (cordoned), node 4 nil, node 5 {a} deleted. Class 0 selects `a`
    (REQ_ALL) and tolerates taint 0; class 1 has one empty term list under a
    required affinity (matches nothing) and tolerates nothing; class 2 always."""
    N = 6
    t = dict(n_nodes=N, W=1, label_words=1, taint_words=1, n_numcols=1)
    t["label_bits"] = np.array([[1, 3, 2, 1, 0, 1]], dtype=np.uint64)
    t["taint_bits"] = np.array([[0, 1, 2, 0, 3, 0]], dtype=np.uint64)  # node 1: taint 0, node 2: taint 1
    t["num_vals"], t["num_ok"] = np.zeros((1, N), dtype="<i8"), np.zeros((1, N), dtype=np.uint8)
    t["name_id"] = np.arange(N, dtype="<i4")
    t["node_flags"] = np.array([0, 0, 0, rr.NF_UNSCHED, rr.NF_NIL, rr.NF_DEAD], dtype=np.uint8)
    t["mask_pool"], t["tol_pool"] = np.array([1], dtype=np.uint64), np.array([1, 0, 0], dtype=np.uint64)
    t["reqs"] = np.array([(rr.REQ_ALL, 0, 0, 0, 0)], dtype=rr.REQ_PROG)
    t["terms"] = np.zeros(1, dtype=rr.TERM_PROG)
    t["classes"] = np.array([(0, 0, 0, 0, 0, 0), (-1, 1, 0, 0, 1, 0), (-1, 0, 0, 0, 2, 1)], dtype=rr.CLASS_PROG)
    sel, tol, uns, live, cm = rr.stage_reference(t)
    assert [int(x[0]) for x in sel] == [0b111011, 0b010000, 0b111111]  # the nil node passes every stage
    assert [int(x[0]) for x in tol] == [0b111011, 0b111001, 0b111111]
    assert (int(uns[0]), int(live[0])) == (0b001000, 0b011111)
    assert [int(x[0]) for x in cm] == [0b010011, 0b010000, 0b111111]
    for c in (0, 1):
        assert int(cm[c][0]) == int(sel[c][0]) & int(tol[c][0]) & ~int(uns[0]) & int(live[0])


@pytest.mark.parametrize("n_nodes", rr.NODE_COUNTS)
def test_stage_cases_hold_what_they_claim(n_nodes):
    t = rr.stage_case(9000 + n_nodes, n_nodes)
    sel, tol, uns, live, cm = rr.stage_reference(t)
    assert set(t["reqs"]["kind"].tolist()) == set(range(9))
    assert set(t["node_flags"].tolist()) >= {0, 1, 2, 4, 5}
    for c, cp in enumerate(t["classes"]):
        if not cp["always"]:
            assert (cm[c] == sel[c] & tol[c] & ~uns & live).all()
    # the stages differ from one another: the planes are not all the same
    assert (sel[0] != tol[0]).any()
    assert int(live[-1]) >> ((n_nodes - 1) & 63) < 2  # nothing past the last node


@pytest.mark.parametrize("name", sorted(rr.REASON_CASES))
def test_reason_cases_hold_what_they_claim(name):
    c = rr.reasons_case(**rr.REASON_CASES[name])
    p = c["p"]
    out = rr.reasons_reference(c)[:p["nq"] * rr.REASON_OUT].reshape(-1, rr.REASON_OUT)
    assert (np.diff(c["hoff"]) == 40).any() and (np.diff(c["hoff"]) == 0).any()
    windowed = (p["tab_lo"], p["tab_n"]) != (0, p["n_nodes"])
    r0 = out[0]  # the rare class over every node
    if p["cap_check"] and not windowed:
        last = p["n_nodes"] - 1
        assert r0[1 + rr.WHY_TAINTS] == 1 and r0[7 + rr.WHY_TAINTS] == last  # once, at the table's last node
        assert r0[1 + rr.WHY_SELECTOR] == 0 and r0[7 + rr.WHY_SELECTOR] == -1  # nowhere
        assert r0[0] == sum(rr.bit(c["live"], n) for n in range(p["n_nodes"]))
    if not p["cap_check"]:
        assert not out[:, 1:7].any() and (out[:, 7:13] == -1).all() and out[0][0] > 0
    assert not out[:, 1 + rr.WHY_HOST_PORTS].any() and not out[:, 1 + rr.WHY_POD_AFFINITY].any()
    if p["cap_check"] and p["n_nodes"] >= 1024 and not windowed:
        # the pod cap depends on the query's point: the same query at the log's end caps other nodes
        c2 = dict(c, q=c["q"].copy())
        c2["q"]["point"] = p["n_dec"]
        assert rr.reasons_reference(c2)[1 + rr.WHY_POD_CAP] != r0[1 + rr.WHY_POD_CAP]
