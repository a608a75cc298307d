"""The reference of the node reasons (tests/node_why_ref.py) and its seeded
cases (tests/node_why_cases.py), on the CPU: rows worked by hand for a 5-node
case, each case holding what it claims, and the comparator reporting each
defect a kernel could have. Nothing of the library runs here."""
import numpy as np
import pytest

import node_why_cases as nc
import node_why_ref as nr
import task_why_cases as tc
import task_why_ref as tr
from kernel_ref import SENTINEL

MI = tc.MI


def hand_case():
    """Five nodes, one class, the predicates plugin on. Three shapes:
      s0  1000m / 1Gi           7 tasks, 3 in open queues, first task 40
      s1  BestEffort            2 tasks, 2 open,           first task 3
      s2  3000m / 1Gi           5 tasks, 0 open,           first task 12
      n0  2 of 2 pods                                   -> pod cap for all 14
      n1  unschedulable and its taints not tolerated    -> unschedulable (the earlier stage) for all 14
      n2  Idle 995m (within the 10m tolerance), 2Gi     -> s0 and s1 fit Idle; s2 short of cpu
      n3  Idle 500m / 512Mi, Releasing 1000m / 1Gi      -> s1 fits Idle, s0 fits Releasing (short of cpu and memory),
                                                           s2 short of cpu and memory
      n4  dead
    """
    c = tc.blank("hand", 5, classes=1, stride=5)
    c.ntasks[0], c.maxtasks[0] = 2, 2
    c.unsched[1] = True
    c.taint_ok[0][1] = False
    c.idle[2] = [995.0, 2048.0 * MI, 0.0]
    c.idle[3], c.rel[3] = [500.0, 512.0 * MI, 0.0], [1000.0, 1024.0 * MI, 0.0]
    c.live[4] = False
    tc.shape(c, 0, [1000.0, 1024.0 * MI, 0.0])
    tc.shape(c, 0, [1.0, 0.0, 0.0], best_effort=True)
    tc.shape(c, 0, [3000.0, 1024.0 * MI, 0.0])
    for s, (w, o, f) in zip(c.shapes, ((7, 3, 40), (2, 2, 3), (5, 0, 12))):
        s["weight"], s["weight_open"], s["first_task"] = w, o, f
    return nc.finish(c, 1)


def test_hand_worked_rows():
    c = hand_case()
    r = nr.rows(c)
    assert sorted(r) == [0, 1, 2, 3]  # the dead node has no row
    e = nr.empty_row()
    assert r[0] == dict(e, count=[14, 0, 0, 0, 0, 0, 0, 0, 0, 0], first_task=[3] + [-1] * 9)
    assert r[1] == dict(e, count=[0, 0, 0, 14, 0, 0, 0, 0, 0, 0], first_task=[-1] * 3 + [3] + [-1] * 6)
    assert r[2] == dict(count=[0, 0, 0, 0, 0, 0, 9, 0, 5, 0], first_task=[-1] * 6 + [3, -1, 12, -1], idle_short=[5, 0, 0],
                        open_idle=5, open_releasing=0, idle_best_effort=2)
    assert r[3] == dict(count=[0, 0, 0, 0, 0, 0, 2, 7, 5, 0], first_task=[-1] * 6 + [3, 40, 12, -1],
                        idle_short=[12, 12, 0], open_idle=2, open_releasing=3, idle_best_effort=2)


@pytest.mark.parametrize("name", nc.NAMES)
def test_every_pending_task_has_one_cause(name):
    c = nc.case(name)
    total = sum(s["weight"] for s in c.shapes)
    rows_ = nr.rows(c)
    lo, nn = c.p["tab_lo"], c.p["tab_n"]
    named = [64 * w + l for w in c.words for l in range(64) if 64 * w + l < nn]
    assert len(rows_) == sum(c.live[lo + row] for row in named)
    for r in rows_.values():
        assert sum(r["count"]) == total
        assert r["count"][tr.HOST_PORTS] == r["count"][tr.POD_AFFINITY] == r["count"][tr.PANIC] == 0
        for k in range(tr.N_CAUSES):
            assert (r["first_task"][k] >= 0) == (r["count"][k] > 0)
        assert all(v <= r["count"][tr.FITS_RELEASING] + r["count"][tr.SHORT] for v in r["idle_short"])
        assert r["open_idle"] <= r["count"][tr.FITS_IDLE] and r["open_releasing"] <= r["count"][tr.FITS_RELEASING]
        assert r["idle_best_effort"] <= r["count"][tr.FITS_IDLE]


def test_cases_hold_what_they_claim():
    cases = [nc.case(n) for n in nc.NAMES]
    assert {1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025} <= {c.p["tab_n"] for c in cases}
    assert {c.p["tab_lo"] for c in cases} >= {0, 64, 128}
    G = nc.GROUP
    assert {c.p["n_shapes"] for c in cases} >= {1, G - 1, G, G + 1, 2 * G + 1}
    assert any(not c.p["cap_check"] for c in cases)
    # word lists: every word, only the first, only the last and ragged, two non-adjacent, one word of 1025 nodes
    full = lambda c: (c.p["tab_n"] + 63) // 64
    assert any(c.words == list(range(full(c))) and full(c) > 4 for c in cases)
    assert any(c.words == [0] and full(c) > 1 for c in cases)
    assert any(c.words == [full(c) - 1] and full(c) > 1 and c.p["tab_n"] % 64 for c in cases)
    assert any(len(c.words) == 2 and c.words[1] - c.words[0] > 1 for c in cases)
    assert sum(c.p["tab_n"] == 1025 and len(c.words) == 1 for c in cases) >= 2
    assert any(c.p["ostride"] == 64 * len(c.words) for c in cases) and any(c.p["ostride"] > 64 * len(c.words) for c in cases)
    # garbage plane bits past the last node, and a table that ends before the planes do
    c = nc.case("n65-s33")
    assert int(nc.planes_words(c)[1]) >> 1 == (1 << 63) - 1
    assert any(c.p["tab_n"] % 64 and c.p["tab_lo"] + c.p["tab_n"] < c.p["n_nodes"] for c in cases)
    for c in cases:
        if c.p["tab_n"] >= 63 and c.name.startswith("n") and len(c.words) > 1:
            lo = c.p["tab_lo"]
            assert not all(c.live[lo:lo + c.p["tab_n"]]), f"{c.name}: no dead node"
        if c.name.startswith("n") and c.p["n_shapes"] >= 3:
            assert any(s["best_effort"] for s in c.shapes) and any(0.0 in s["req"] for s in c.shapes)
        ws = [s["weight"] for s in c.shapes]
        assert ws[0] == 1 or c.name == "every-cause"
        assert sum(ws) < 2 ** 31
    # weights of 1 and 100000, weight_open of 0 and of the weight
    shapes = [s for c in cases for s in c.shapes]
    assert any(s["weight"] == nc.BIG for s in shapes)
    assert any(s["weight_open"] == 0 and s["weight"] > 1 for s in shapes)
    assert any(s["weight_open"] == s["weight"] > 1 for s in shapes)
    assert any(0 < s["weight_open"] < s["weight"] for s in shapes)
    # cap_check 0: no stage cause, whatever the planes and the pod counts say
    c = nc.case("n200-s5-cap0")
    assert any(c.ntasks[r] >= c.maxtasks[r] for r in range(c.p["tab_n"]))
    for r in nr.rows(c).values():
        assert sum(r["count"][:6]) == 0
    # the tolerance edges: per dimension, against Idle and against Releasing, both sides of the bound
    c = nc.case("tolerance-edges")
    rows_ = nr.rows(c)
    per = len(tc.EDGES)
    fits = [e >= 0 or abs(e) < 1.0 for e in tc.EDGES]
    assert [s["weight"] for s in c.shapes] == [1, nc.BIG]  # (shape 0, the one with every dimension: the odd task)
    for block, code in ((0, tr.FITS_IDLE), (3, tr.FITS_RELEASING)):
        for d in range(3):
            got = [rows_[(block + d) * per + i]["count"][code] % nc.BIG == 1 for i in range(per)]
            assert got == fits, (block, d, got)
    # every cause; the causes that depend on the shape all on node 10; dead node 6 nowhere
    c = nc.case("every-cause")
    rows_ = nr.rows(c)
    assert c.words == [0, 2] and 6 not in rows_
    total = sum(s["weight"] for s in c.shapes)
    assert rows_[3]["count"][tr.POD_CAP] == total and rows_[4]["count"][tr.POD_CAP] == 0
    assert rows_[64 + 1]["count"][tr.UNSCHEDULABLE] == total  # node 129: lane 1 of the second entry
    assert rows_[64]["count"][tr.FITS_RELEASING] > 0         # node 128 fits the large request on Releasing alone
    assert all(rows_[10]["count"][k] > 0 for k in (1, 4, 6, 7, 8))
    seen = [any(r["count"][k] for r in rows_.values()) for k in range(10)]
    assert [k for k in range(10) if seen[k]] == list(nc.DEVICE_CAUSES)
    # two shapes under one cause on one node, their first tasks in either order
    f = [s["first_task"] for s in c.shapes]
    assert f[0] > f[1] and f[2] < f[3] and rows_[0]["first_task"][tr.FITS_IDLE] == min(f[:4] + f[8:])
    # dead nodes that would fail each stage
    c = nc.case("unschedulable")
    assert not c.live[7] and c.unsched[7] and 7 not in nr.rows(c) and nr.rows(c)[5]["count"][tr.UNSCHEDULABLE] > 0


# a case on which each defect must show
DEFECT_CASES = {"weight_ignored": "n65-s33", "open_for_count": "n65-s33", "min_over_shape_index": "every-cause",
                "dead_row": "every-cause", "ragged_counted": "n300-last-word", "last_group_only": "n1025-word-9",
                "stage_swap": "n1024-s32", "releasing_first": "n1024-s32", "short_on_idle": "tolerance-edges",
                "be_tested": "n1024-s32", "cap_without_check": "n200-s5-cap0", "unnamed_word_written": "n600-words-1-7"}


def test_defect_list_is_the_issue_s():
    assert set(DEFECT_CASES) == set(nr.DEFECTS) and len(nr.DEFECTS) == 12


@pytest.mark.parametrize("defect", nr.DEFECTS)
def test_comparator_reports_defect(defect):
    c = nc.case(DEFECT_CASES[defect])
    want = nr.rows(c)
    assert not nr.compare(c, want, nr.rows(c))
    errs = nr.compare(c, want, nr.rows(c, defect))
    assert errs, f"{defect} goes unnoticed on {c.name}"
    raw = nc.out_bytes(c, nr.rows(c, defect))
    assert nc.compare_raw(c, raw)


def test_comparator_reports_one_overwritten_sentinel():
    c = nc.case("n65-s33")
    raw = nc.out_bytes(c, nr.rows(c))
    assert not nc.compare_raw(c, raw)
    bad = raw.copy()
    bad[nc.N_FIELDS * c.p["ostride"] * 4 + 1234] ^= 0xFF
    assert any("guard" in e for e in nc.compare_raw(c, bad))
    bad = raw.copy()
    bad[(c.p["ostride"] - 1) * 4] = 0  # a word of the first plane past the listed slots
    assert nc.compare_raw(c, bad)
    bad = raw.copy()
    bad[65 * 4:65 * 4 + 4] = SENTINEL  # a ragged lane's slot left as the probe filled it
    assert nc.compare_raw(c, bad)


def test_layout_round_trip():
    c = nc.case("shard64-93of200")
    rows_, clean = nc.rows_of(c, nc.out_bytes(c, nr.rows(c)))
    assert clean and rows_ == nr.rows(c)
    assert nc.table_block(c).size == c.p["stride"] * 56
    assert nc.shape_records(c).tobytes()[32:44] == np.array(
        [c.shapes[0][k] for k in ("weight", "weight_open", "first_task")], dtype="<i4").tobytes()
    assert nc.word_list(c).tolist() == [0, 1]
