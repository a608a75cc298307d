"""The reference of the pending-task reasons (tests/task_why_ref.py) and its
seeded cases (tests/task_why_cases.py), on the CPU: rows worked by hand for a
5-node case, each case holding what it claims, and the comparator reporting
each defect a kernel could have. Nothing of the library runs here."""
import numpy as np
import pytest

import task_why_cases as tc
import task_why_ref as tr
from kernel_ref import SENTINEL

MI = tc.MI


def hand_case():
    """Five nodes, one class, the predicates plugin on; request 1000m / 1Gi / no GPU.
      n0  2 of 2 pods                                   -> pod cap
      n1  unschedulable and its taints not tolerated    -> unschedulable (the earlier stage)
      n2  Idle 995m (within the 10m tolerance), 2Gi     -> fits Idle; FitDelta cpu is 995 - 1010 < 0 but not counted
      n3  Idle 500m / 512Mi, Releasing 1000m / 1Gi      -> fits Releasing; short of cpu and memory
      n4  Idle 2000m / 1Gi - 10Mi (at the bound: |a - r| == min), Releasing 0 -> short; short of memory only
    """
    c = tc.blank("hand", 5, classes=1, stride=5)
    c.ntasks[0], c.maxtasks[0] = 2, 2
    c.unsched[1] = True
    c.taint_ok[0][1] = False
    c.idle[2] = [995.0, 2048.0 * MI, 0.0]
    c.idle[3], c.rel[3] = [500.0, 512.0 * MI, 0.0], [1000.0, 1024.0 * MI, 0.0]
    c.idle[4] = [2000.0, 1014.0 * MI, 0.0]
    tc.shape(c, 0, [1000.0, 1024.0 * MI, 0.0])
    tc.shape(c, 0, [1.0, 0.0, 0.0], best_effort=True)
    return c


def test_hand_worked_rows():
    c = hand_case()
    r0, r1 = tr.rows(c)
    assert r0["count"] == [1, 0, 0, 1, 0, 0, 1, 1, 1, 0]
    assert r0["first_node"] == [0, -1, -1, 1, -1, -1, 2, 3, 4, -1]
    assert r0["idle_short"] == [1, 2, 0]
    # the BestEffort shape: every node past the stages, no resource test, no idle_short
    assert r1["count"] == [1, 0, 0, 1, 0, 0, 3, 0, 0, 0]
    assert r1["first_node"] == [0, -1, -1, 1, -1, -1, 2, -1, -1, -1]
    assert r1["idle_short"] == [0, 0, 0]


@pytest.mark.parametrize("name", tc.NAMES)
def test_every_live_node_has_one_cause(name):
    c = tc.case(name)
    live = sum(c.live[c.p["tab_lo"]:c.p["tab_lo"] + c.p["tab_n"]])
    for r in tr.rows(c):
        assert sum(r["count"]) == live
        assert r["count"][tr.HOST_PORTS] == r["count"][tr.POD_AFFINITY] == r["count"][tr.PANIC] == 0
        for k in range(tr.N_CAUSES):
            assert (r["first_node"][k] >= 0) == (r["count"][k] > 0)
        assert all(v <= r["count"][tr.FITS_RELEASING] + r["count"][tr.SHORT] for v in r["idle_short"])


def test_cases_hold_what_they_claim():
    sizes = {tc.case(n).p["tab_n"] for n in tc.NAMES}
    assert {1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025} <= sizes
    assert {tc.case(n).p["tab_lo"] for n in tc.NAMES} >= {0, 64, 128}
    assert {tc.case(n).p["n_shapes"] for n in tc.NAMES} >= {1, tc.GROUP - 1, tc.GROUP, tc.GROUP + 1}
    assert any(not tc.case(n).p["cap_check"] for n in tc.NAMES)
    assert any(c.p["tab_n"] % 64 and c.p["tab_lo"] + c.p["tab_n"] < c.p["n_nodes"] for c in map(tc.case, tc.NAMES))
    for n in tc.NAMES:
        c = tc.case(n)
        if c.p["tab_n"] >= 63 and n.startswith("n"):
            lo = c.p["tab_lo"]
            assert not all(c.live[lo:lo + c.p["tab_n"]]), f"{n}: no dead node"
            assert any(s["best_effort"] for s in c.shapes) or c.p["n_shapes"] < 3
            assert any(0.0 in s["req"] for s in c.shapes) or c.p["n_shapes"] < 3
    # cap_check 0: no stage cause, whatever the planes and the pod counts say
    for r in tr.rows(tc.case("n200-s5-cap0")):
        assert sum(r["count"][:6]) == 0
    # the tolerance edges: per dimension, against Idle and against Releasing, both sides of the bound
    c = tc.case("tolerance-edges")
    k = [tr.cause(c, c.shapes[0], row, row)[0] for row in range(c.p["tab_n"])]
    per = len(tc.EDGES)
    fits = [e >= 0 or abs(e) < 1.0 for e in tc.EDGES]
    assert True in fits and False in fits
    for block, code in ((0, tr.FITS_IDLE), (3, tr.FITS_RELEASING)):
        for d in range(3):
            got = k[(block + d) * per:(block + d + 1) * per]
            assert got == [code if f else tr.SHORT for f in fits], (block, d, got)
    r0, r1 = tr.rows(c)
    assert r0["count"][tr.FITS_RELEASING] > 0 and r0["count"][tr.SHORT] > 0
    # a request dimension of 0 is never short: the nodes of no GPU Idle count for shape 0 only
    assert r0["idle_short"][2] > 0 and r1["idle_short"][2] == 0
    # every cause, and causes whose only node is in the last word
    c = tc.case("every-cause")
    r = tr.rows(c)[0]
    assert all(r["count"][k] > 0 for k in (0, 1, 3, 4, 6, 7, 8))
    assert r["count"][tr.UNSCHEDULABLE] == 1 and r["first_node"][tr.UNSCHEDULABLE] == 129
    assert r["count"][tr.FITS_RELEASING] == 1 and r["first_node"][tr.FITS_RELEASING] == 128
    assert r["count"][tr.POD_CAP] == 1 and r["first_node"][tr.POD_CAP] == 3  # node 4, one below its cap, passes
    assert r["first_node"][tr.SELECTOR] == 5  # three stages fail there: the first names it; dead node 6 is nowhere
    assert tr.rows(c)[2]["count"][tr.FITS_IDLE] == 130 - 1 - sum(r["count"][:6])


# a case on which each defect must show
DEFECT_CASES = {"stage_swap": "n1024-s16", "cap_gt": "every-cause", "no_tolerance": "tolerance-edges",
                "releasing_first": "n1024-s16", "short_on_idle": "tolerance-edges", "zero_dim_short": "tolerance-edges",
                "be_tested": "n1024-s16", "garbage_counted": "shard64-93of200", "dead_counted": "every-cause",
                "first_node_last": "n129-s17", "offset_dropped": "shard64-93of200"}


def test_defect_list_is_the_issue_s():
    assert set(DEFECT_CASES) == set(tr.DEFECTS) and len(tr.DEFECTS) == 11  # the twelfth is the sentinel below


@pytest.mark.parametrize("defect", tr.DEFECTS)
def test_comparator_reports_defect(defect):
    c = tc.case(DEFECT_CASES[defect])
    want = tr.rows(c)
    assert not tr.compare(c, want, tr.rows(c))
    errs = tr.compare(c, want, tr.rows(c, defect))
    assert errs, f"{defect} goes unnoticed on {c.name}"
    raw = tc.out_bytes(tr.rows(c, defect))
    assert tc.compare_raw(c, raw)


def test_comparator_reports_one_overwritten_sentinel():
    c = tc.case("n65-s17")
    raw = tc.out_bytes(tr.rows(c))
    assert not tc.compare_raw(c, raw)
    bad = raw.copy()
    bad[len(c.shapes) * tc.OUT_WORDS * 4 + 1234] ^= 0xFF
    assert any("guard" in e for e in tc.compare_raw(c, bad))
    bad = raw.copy()
    bad[tc.OUT_WORDS * 4 - 1] = SENTINEL  # a row's padding word left as the probe filled it
    assert tc.compare_raw(c, bad)


def test_layout_round_trip():
    c = tc.case("shard64-93of200")
    rows_, clean = tc.rows_of(c, tc.out_bytes(tr.rows(c)))
    assert clean and rows_ == tr.rows(c)
    assert tc.table_block(c).size == c.p["stride"] * 56
    assert tc.planes_words(c).size == (2 * c.p["classes"] + 2) * c.p["W"]
    assert tc.shape_records(c).tobytes()[:8] == np.array([c.shapes[0]["cls"], int(c.shapes[0]["best_effort"])],
                                                         dtype="<i4").tobytes()
