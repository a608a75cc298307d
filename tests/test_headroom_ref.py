"""The reference of the pending-task headroom (tests/headroom_ref.py) and its
cases (tests/headroom_cases.py), on the CPU: rows worked by hand for a 5-node
case, each case holding what it claims, and the comparator reporting each of
the twelve defects a kernel could have. Nothing of the library runs here."""
import pytest

import headroom_cases as hc
import headroom_ref as hr
from kernel_ref import SENTINEL

MI = hc.MI


def hand_case(limit=4):
    """Five nodes, one class, the predicates plugin on; request 1000m / 1Gi / no GPU; limit 4.
      n0  2 of 2 pods                                          -> not past the stages
      n1  unschedulable                                        -> not past the stages
      n2  Idle 2995m (the third copy within the 10m tolerance) / 8Gi, 100 of 110 pods -> 3 from Idle
      n3  Idle 1000m / 1Gi, Releasing 2000m / 8Gi, 108 of 110 pods -> 1 from Idle, then the room of 2 leaves 1
      n4  Idle 9000m / 64Gi, Releasing the same, 0 of 110 pods -> 4 from Idle: cut by the limit (room 110)
    """
    c = hc.blank("hand", 5, limit, classes=1, stride=5)
    c.ntasks[0], c.maxtasks[0] = 2, 2
    c.unsched[1] = True
    c.idle[1] = [9000.0, 65536.0 * MI, 0.0]
    c.idle[2], c.ntasks[2] = [2995.0, 8192.0 * MI, 0.0], 100
    c.idle[3], c.rel[3], c.ntasks[3] = [1000.0, 1024.0 * MI, 0.0], [2000.0, 8192.0 * MI, 0.0], 108
    c.idle[4], c.rel[4], c.ntasks[4] = [9000.0, 65536.0 * MI, 0.0], [9000.0, 65536.0 * MI, 0.0], 0
    hc.shape(c, 0, [1000.0, 1024.0 * MI, 0.0])
    hc.shape(c, 0, [0.0, 0.0, 0.0], best_effort=True)
    return c


def test_hand_worked_rows():
    r0, r1 = hr.rows(hand_case())
    assert r0 == dict(copies_idle=3 + 1 + 4, copies_releasing=1, nodes_idle=3, nodes_releasing_only=0, first_node=2,
                      max_node_copies=4, nodes_pass=3, limit_hit=1)
    # the BestEffort shape: min(limit, room) on every node past the stages: 4, 2 (room 2 < limit), 4
    assert r1 == dict(copies_idle=4 + 2 + 4, copies_releasing=0, nodes_idle=3, nodes_releasing_only=0, first_node=2,
                      max_node_copies=4, nodes_pass=3, limit_hit=2)
    # limit 1: one copy a node, every node cut (their rooms are 10, 2 and 110)
    r0, _ = hr.rows(hand_case(limit=1))
    assert (r0["copies_idle"], r0["copies_releasing"], r0["max_node_copies"], r0["limit_hit"]) == (3, 0, 1, 3)


@pytest.mark.parametrize("name", hc.NAMES)
def test_rows_are_consistent(name):
    c = hc.case(name)
    live = sum(c.live[c.p["tab_lo"]:c.p["tab_lo"] + c.p["tab_n"]])
    for r in hr.rows(c):
        assert r["nodes_idle"] + r["nodes_releasing_only"] <= r["nodes_pass"] <= live
        assert (r["first_node"] >= 0) == (r["copies_idle"] + r["copies_releasing"] > 0)
        assert r["max_node_copies"] <= c.p["limit"] and r["limit_hit"] <= r["nodes_pass"]
        assert r["copies_idle"] + r["copies_releasing"] <= r["max_node_copies"] * r["nodes_pass"]
        assert r["first_node"] < 0 or c.p["tab_lo"] <= r["first_node"] < c.p["tab_lo"] + c.p["tab_n"]


def test_cases_hold_what_they_claim():
    cs = [hc.case(n) for n in hc.NAMES]
    assert {c.p["tab_n"] for c in cs} >= {1, 63, 64, 65, 70, 256, 257, 330}
    assert {c.p["tab_lo"] for c in cs} >= {0, 64, 128}
    assert {c.p["n_shapes"] for c in cs} >= {1, hc.GROUP, hc.GROUP + 1, 2 * hc.GROUP + 1}
    assert {c.p["limit"] for c in cs} >= {1, 2, 7, 1024}
    assert {c.p["cap_check"] for c in cs} == {0, 1}
    assert any(c.p["tab_n"] % 64 and c.p["tab_lo"] + c.p["tab_n"] < c.p["n_nodes"] for c in cs)
    for c in cs:
        if c.p["tab_n"] >= 63 and c.name.startswith("n"):
            lo = c.p["tab_lo"]
            assert not all(c.live[lo:lo + c.p["tab_n"]]), f"{c.name}: no dead node"
            dead = next(n for n in range(lo, lo + c.p["tab_n"]) if not c.live[n])
            assert abs(c.idle[dead - lo][0]) > 1e6 or c.idle[dead - lo][0] < 0, f"{c.name}: a dead node without garbage"
            assert any(c.ntasks[r] >= c.maxtasks[r] for r in range(c.p["tab_n"]) if c.live[lo + r])
            assert any(s["best_effort"] for s in c.shapes) or c.p["n_shapes"] < 3
    # the seeded cases together: copies from Releasing, Releasing-only nodes, cut nodes, several copies a node
    tot = hr.empty_row()
    for c in cs:
        if c.name.startswith(("n", "shard")):
            for r in hr.rows(c):
                for k in hr.KEYS:
                    tot[k] = max(tot[k], r[k])
    assert all(tot[k] > 0 for k in hr.KEYS) and tot["max_node_copies"] >= 5
    # how a loop ends: the hand-worked copies of each node, shape 0
    c = hc.case("loop-ends-l7")
    for n, claim in c.claims.items():
        got = hr.node_copies(c, c.shapes[0], n, n)
        assert got == ((True,) + claim if claim else (False, 0, 0, False)), (n, got)
    assert {(k[0] > 0, k[1] > 0, k[2]) for k in c.claims.values() if k} == \
        {(True, False, False), (True, False, True), (True, True, False), (True, True, True), (False, True, False),
         (False, False, False)}
    r0, r1, r2, r3 = hr.rows(c)
    assert r3["max_node_copies"] == 4 and hr.node_copies(c, c.shapes[3], 8, 8) == (True, 1, 3, False)
    assert (r0["limit_hit"], r0["max_node_copies"], r0["first_node"]) == (2, 7, 0)
    # class 1 fails the selector on node 0 and the taints on node 1: its first node is node 2
    assert r1["first_node"] == 2 and r1["nodes_pass"] == r0["nodes_pass"] - 2
    assert r1["copies_idle"] == r0["copies_idle"] - 3 - 2
    # the BestEffort shape: min(7, room) on every node past the stages (node 69 unschedulable, node 11 capped)
    rooms = [c.maxtasks[n] - c.ntasks[n] for n in range(70) if n not in (11, 69)]
    assert r2["copies_idle"] == sum(min(7, r) for r in rooms) and r2["copies_releasing"] == 0
    assert r2["limit_hit"] == sum(7 < r for r in rooms) and r2["nodes_pass"] == 68
    # limit 1 on the same nodes: one copy a node, and every node holding one is cut (no room is 1)
    r0 = hr.rows(hc.case("loop-ends-l1"))[0]
    assert r0["max_node_copies"] == 1 and r0["copies_idle"] == r0["nodes_idle"]
    assert r0["copies_releasing"] == r0["nodes_releasing_only"] == 1
    assert r0["limit_hit"] == r0["nodes_idle"] + r0["nodes_releasing_only"]
    # the tolerance edges and the non-integer pins
    c = hc.case("tolerance")
    for (s, n), (ki, kr) in c.claims.items():
        assert hr.node_copies(c, c.shapes[s], n, n)[1:3] == (ki, kr), (s, n)
    for s, n in ((2, 3), (3, 4)):  # the iterated subtraction and a - k * req disagree
        it = hr.take(c.shapes[s]["req"], c.idle[n], 0, 1024)
        assert hc.product_copies(c.idle[n], c.shapes[s]["req"], 1024) == it + 1


# a case on which each defect must show
DEFECT_CASES = {"rel_restart": "loop-ends-l7", "room_ignored": "loop-ends-l7", "limit_ignored": "loop-ends-l7",
                "division": "tolerance", "no_tolerance": "tolerance", "last_lane_lost": "loop-ends-l7",
                "ragged_counted": "shard64-93of200-l7", "first_node_local": "shard64-93of200-l7",
                "max_idle_only": "loop-ends-l7", "limit_hit_eq": "loop-ends-l7", "be_tested": "loop-ends-l7",
                "wrong_class": "loop-ends-l7"}


def test_defect_list_is_the_issue_s():
    assert set(DEFECT_CASES) == set(hr.DEFECTS) and len(hr.DEFECTS) == 12


@pytest.mark.parametrize("defect", hr.DEFECTS)
def test_comparator_reports_defect(defect):
    c = hc.case(DEFECT_CASES[defect])
    want = hr.rows(c)
    assert not hr.compare(c, want, hr.rows(c))
    errs = hr.compare(c, want, hr.rows(c, defect))
    assert errs, f"{defect} goes unnoticed on {c.name}"
    assert hc.compare_raw(c, hc.out_bytes(hr.rows(c, defect)))


@pytest.mark.parametrize("defect", ("rel_restart", "room_ignored", "limit_ignored", "division", "no_tolerance",
                                    "max_idle_only", "limit_hit_eq", "be_tested", "wrong_class", "last_lane_lost"))
def test_seeded_cases_show_the_defect_too(defect):
    """The arithmetic defects do not need the hand-made nodes to show."""
    assert any(hr.compare(c, hr.rows(c), hr.rows(c, defect)) for c in map(hc.case, hc.NAMES) if c.name[0] in "ns")


def test_comparator_reports_one_overwritten_sentinel():
    c = hc.case("n65-s33-l1024")
    raw = hc.out_bytes(hr.rows(c))
    assert not hc.compare_raw(c, raw)
    bad = raw.copy()
    bad[len(c.shapes) * hc.OUT_WORDS * 4 + 1234] ^= 0xFF
    assert any("guard" in e for e in hc.compare_raw(c, bad))
    bad = raw.copy()
    bad[hc.OUT_WORDS * 4 - 4:hc.OUT_WORDS * 4] = SENTINEL  # a row's last word left as the probe filled it
    assert hc.compare_raw(c, bad)


def test_layout_round_trip():
    c = hc.case("shard64-93of200-l7")
    rows_, clean = hc.rows_of(c, hc.out_bytes(hr.rows(c)))
    assert clean and rows_ == hr.rows(c)
    assert hc.OUT_WORDS == 8 and hc.FIELDS[-1] == "limit"
