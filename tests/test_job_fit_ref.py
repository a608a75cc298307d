"""The reference of the job fit walk (tests/job_fit_ref.py) and its cases
(tests/job_fit_cases.py), on the CPU: the hand-worked walks, each case holding
what it claims, the layout, and the comparator reporting each of the twelve
defects a kernel could have. Nothing of the library runs here."""
import numpy as np
import pytest

import headroom_cases as hc
import job_fit_cases as jc
import job_fit_ref as jr
from kernel_ref import SENTINEL


@pytest.mark.parametrize("name", jc.HAND)
def test_hand_worked_walks(name):
    c = jc.case(name)
    got = jr.walks(c)
    assert c.claims and sorted(c.claims) == list(range(len(c.jobs)))
    for j, claim in c.claims.items():
        assert got[j] == claim, (name, j)


def test_hand_cases_are_the_issue_s():
    """What each hand case is there for, from its claims alone."""
    def claim(name, j=0):
        return jc.case(name).claims[j]
    A, P, NO = jc.A, jc.P, jc.NOWHERE
    assert claim("two-on-one-node")[:2] == [(0, A), (0, A)]
    assert claim("lane-63-then-64")[:2] == [(63, A), (64, A)]
    assert claim("releasing-before-the-next-node") == [(0, A), (0, P), (1, A)]
    c = jc.case("pod-room-of-one")
    assert c.maxtasks[0] - c.ntasks[0] == 1 and claim("pod-room-of-one") == [(0, A), (1, A)]
    c = jc.case("another-class-before-the-cursor")
    assert c.shapes[0]["cls"] != c.shapes[1]["cls"] and claim(c.name)[1][0] < claim(c.name)[0][0]
    c = jc.case("back-to-a-touched-word")
    assert c.jobs[0] == [0, 1, 0] and claim(c.name)[0][0] // 64 == claim(c.name)[1][0] // 64 != claim(c.name)[2][0] // 64
    assert claim("unplaced-then-smaller") == [NO, (0, A), NO]
    assert jr.links(jc.case("unplaced-then-smaller"), [0, 1, 0]) == [-1, -1, 0]
    c = jc.case("tolerance-once")
    assert c.idle[0][0] == 3.0 and c.shapes[0]["req"][0] == 8.0 and claim(c.name) == [(0, A), NO]
    c, t = jc.case("non-integer"), hc.case("tolerance")
    assert c.idle[3] == t.idle[3] and c.idle[4] == t.idle[4]
    assert [s["req"] for s in c.shapes] == [s["req"] for s in t.shapes[2:4]]
    assert hc.product_copies(c.idle[3], c.shapes[0]["req"], 1024) == 8 and claim(c.name, 0).count((3, A)) == 7
    assert hc.product_copies(c.idle[4], c.shapes[1]["req"], 1024) == 5 and claim(c.name, 1).count((4, A)) == 4
    assert claim("512-on-one-node") == [(1, A)] * 512
    nodes = [n for n, _ in claim("512-on-512-nodes")]
    assert len(set(nodes)) == 512 == jr.MAX_STEPS and nodes == sorted(nodes) and 10 not in nodes and 100 not in nodes


def test_cases_hold_what_they_claim():
    cs = [jc.case(n) for n in jc.SEEDED]
    assert {c.p["tab_n"] for c in cs} >= {1, 63, 64, 65, 130, 257, 600, 93}
    assert {(c.p["tab_lo"], c.p["tab_n"], c.p["n_nodes"]) for c in cs} >= {(64, 93, 200), (128, 1, 300)}
    assert {len(c.jobs) for c in cs} >= {1, 2, 5, 70}
    assert {len(j) for c in cs for j in c.jobs} >= {1, 2, 7, 64, 65, 512}
    assert {c.p["cap_check"] for c in cs} == {0, 1}
    for c in cs:
        lo, nn = c.p["tab_lo"], c.p["tab_n"]
        assert c.p["stride"] > nn  # rows past tab_n, holding garbage
        assert all(abs(c.idle[r][0]) > 1e6 or c.idle[r][0] < 0 for r in range(nn, c.p["stride"])), c.name
        if nn >= 63:
            dead = [n for n in range(lo, lo + nn) if not c.live[n]]
            assert dead and all(abs(c.idle[n - lo][0]) > 1e6 or c.idle[n - lo][0] < 0 for n in dead), c.name
        assert not any(s["best_effort"] for s in c.shapes)
    # garbage plane bits past the last node
    c = jc.case("n65-j2")
    w = jc.planes_words(c).reshape(-1, c.p["W"])
    assert all(int(row[-1]) >> 1 == (1 << 63) - 1 for row in w)
    # together: placements from Idle and from Releasing, unplaced steps, a node taking several, several shapes a walk
    kinds, multi, shapes = set(), False, 0
    for c in cs:
        for j, wk in zip(c.jobs, jr.walks(c)):
            kinds |= {(n >= 0, k) for n, k in wk}
            placed = [n for n, _ in wk if n >= 0]
            multi = multi or len(set(placed)) < len(placed)
            shapes = max(shapes, len(set(j)))
    assert kinds == {(True, 0), (True, 1), (False, 0)} and multi and shapes >= 3


# a hand case on which each defect must show
DEFECT_CASES = {"no_overlay": "two-on-one-node", "touched_lost": "lane-63-then-64",
                "rel_not_subtracted": "releasing-before-the-next-node", "pods_not_counted": "pod-room-of-one",
                "idle_everywhere_first": "releasing-before-the-next-node",
                "one_cursor": "another-class-before-the-cursor", "exclusive_cursor": "two-on-one-node",
                "stops_at_unplaced": "unplaced-then-smaller", "kinds_swapped": "releasing-before-the-next-node",
                "local_nodes": "shard-70-of-200", "dead_takes": "512-on-512-nodes", "ragged_counted": "shard-70-of-200"}


def test_defect_list_is_the_issue_s():
    assert set(DEFECT_CASES) == set(jr.DEFECTS) and len(jr.DEFECTS) == 12
    assert set(DEFECT_CASES.values()) <= set(jc.HAND)


@pytest.mark.parametrize("defect", jr.DEFECTS)
def test_comparator_reports_defect(defect):
    c = jc.case(DEFECT_CASES[defect])
    want = jr.walks(c)
    assert not jr.compare(c, want, jr.walks(c))
    errs = jr.compare(c, want, jr.walks(c, defect))
    assert errs, f"{defect} goes unnoticed on {c.name}"
    assert jc.compare_raw(c, jc.out_bytes(jr.walks(c, defect)))


@pytest.mark.parametrize("defect", jr.DEFECTS)
def test_seeded_cases_show_the_defect_too(defect):
    assert any(jr.compare(c, jr.walks(c), jr.walks(c, defect)) for c in map(jc.case, jc.SEEDED))


def test_the_cursor_changes_no_result():
    """The argument of kbg_device.hpp: a walk that starts each step at its
    `prev` step's node, and gives up where that step landed nowhere, is the
    plain walk (requests without a negative dimension)."""
    for c in map(jc.case, jc.NAMES):
        for job, want in zip(c.jobs, jr.walks(c)):
            prev, land = jr.links(c, job), [n - c.p["tab_lo"] if n >= 0 else -1 for n, _ in want]
            for i, p in enumerate(prev):
                if p >= 0:
                    assert land[i] == -1 or 0 <= land[p] <= land[i], (c.name, i)
    c = jc.blank("negative", 2)
    jc.shape(c, 0, [-5.0, 0.0, 0.0])
    assert jr.links(c, [0, 0, 0]) == [-1, -1, -1]


def test_comparator_reports_one_overwritten_sentinel():
    c = jc.case("n65-j2")
    raw = jc.out_bytes(jr.walks(c))
    assert not jc.compare_raw(c, raw)
    bad = raw.copy()
    bad[sum(len(j) for j in c.jobs) * 8 + 1234] ^= 0xFF
    assert any("guard" in e for e in jc.compare_raw(c, bad))
    bad = raw.copy()
    bad[4:8] = SENTINEL  # a step's kind left as the probe filled it
    assert jc.compare_raw(c, bad)


def test_layout_round_trip():
    c = jc.case("shard64-93of200")
    walks_, clean = jc.walks_of(c, jc.out_bytes(jr.walks(c)))
    assert clean and walks_ == jr.walks(c)
    assert jc.STEP.itemsize == 8 and jc.FIELDS[-2:] == ("n_jobs", "n_steps")
    off, steps = jc.job_offsets(c), jc.step_records(c)
    assert off.tolist() == [0, 64, 71] and len(steps) == 71 and off.dtype == np.dtype("<i4")
    for j, job in enumerate(c.jobs):
        assert steps["shape"][off[j]:off[j + 1]].tolist() == job
        assert steps["prev"][off[j]:off[j + 1]].tolist() == jr.links(c, job)


def test_rows_of():
    places = [(7, -1, 0), (8, 2, 0), (9, 2, 1), (10, 5, 0)]
    assert jr.rows_of(places, 1, 3) == dict(walked=4, placed_idle=2, placed_releasing=1, first_unplaced=7,
                                            nodes_used=2, ready_after=3)
    assert jr.rows_of(places, 3, 3)["ready_after"] == 0 and jr.rows_of(places, 0, 4)["ready_after"] == -1
