"""The reference of the node drain walk (tests/drain_ref.py) and its cases
(tests/drain_cases.py), on the CPU: the hand-worked walks, each case holding
what it claims, the layout, and the comparator reporting each of the twelve
defects a kernel could have. Nothing of the library runs here."""
import numpy as np
import pytest

import drain_cases as dc
import drain_ref as dr
from kernel_ref import SENTINEL


@pytest.mark.parametrize("name", dc.HAND)
def test_hand_worked_walks(name):
    c = dc.case(name)
    got = dr.walks(c)
    assert c.claims and sorted(c.claims) == list(range(len(c.walks)))
    for j, claim in c.claims.items():
        assert got[j] == claim, (name, j)


def test_hand_cases_are_the_issue_s():
    """What each hand case is there for, from its claims alone."""
    def claim(name, j=0):
        return dc.case(name).claims[j]
    A, P, NO = dc.A, dc.P, dc.NOWHERE
    # the drained node is the lowest fit and is skipped
    c = dc.case("drained-is-the-lowest-fit")
    assert c.drain == [0] and dr.less_equal(c.shapes[0]["req"], c.idle[0]) and claim(c.name)[0] == (1, A)
    # Releasing on node k is taken before Idle on node k + 1
    assert claim("releasing-before-the-next-node") == [(1, A), (1, P), (2, A)]
    # a BestEffort step lands where a requesting one cannot
    c = dc.case("best-effort-where-a-request-cannot")
    assert c.shapes[1]["best_effort"] and not c.shapes[0]["best_effort"]
    assert not dr.less_equal(c.shapes[1]["req"], c.idle[1]) and not dr.less_equal(c.shapes[0]["req"], c.idle[1])
    assert claim(c.name) == [(1, A), (3, A), (1, A)]
    c = dc.case("best-effort-fills-the-last-pod-slot")
    assert c.maxtasks[1] - c.ntasks[1] == 1 and claim(c.name) == [(1, A), (2, A), (2, A)]
    # a step lands nowhere and then a smaller one places
    assert claim("unplaced-then-smaller") == [NO, (1, A), NO]
    assert dr.links(dc.case("unplaced-then-smaller"), [0, 1, 0]) == [-1, -1, 0]
    # a walk goes back to a touched word
    c = dc.case("back-to-a-touched-word")
    assert c.walks[0] == [0, 1, 0] and claim(c.name)[0][0] // 64 == claim(c.name)[1][0] // 64 != claim(c.name)[2][0] // 64
    # the tolerance case (3, ., 0) takes (8, 64Mi, 0) once
    c = dc.case("tolerance-once")
    assert c.idle[1][0] == 3.0 and c.shapes[0]["req"] == [8.0, 64.0 * dc.MI, 0.0] and claim(c.name) == [(1, A), NO]
    # the cordon: the node the first fit would have been
    c = dc.case("cordon-takes-the-first-fit")
    assert c.cordon == {1} and claim(c.name)[0] == (65, A)
    c.cordon = set()
    try:
        assert dr.walks(c)[0][0] == (1, A)
    finally:
        c.cordon = {1}
    assert claim("exclusion-is-per-walk", 1)[0] == (0, A) and dc.case("exclusion-is-per-walk").drain == [0, 1]
    assert claim("cursor-is-per-walk", 1)[0] == (0, A)
    c = dc.case("shard-70-of-200")
    assert c.drain == [67, 3, 150, -1] and dc.walk_rows(c).tolist() == [3, -1, 86, -1]
    assert claim(c.name, 0)[0] == (70, A) and all(claim(c.name, j)[0] == (67, A) for j in (1, 2, 3))
    c = dc.case("cap-check-off-still-excludes")
    assert c.p["cap_check"] == 0 and claim(c.name) == [(2, A), (2, A), NO]
    assert set(claim("the-only-node")) == {NO}
    c = dc.case("whole-word-cordoned")
    nodes = [n for n, _ in claim(c.name)]
    assert c.cordon == set(range(64, 128)) and not set(nodes) & c.cordon and 128 in nodes and 63 not in nodes


def test_cases_hold_what_they_claim():
    cs = [dc.case(n) for n in dc.SEEDED]
    assert {c.p["tab_n"] for c in cs} >= {1, 63, 64, 65, 130, 257, 600, 93}
    assert {(c.p["tab_lo"], c.p["tab_n"], c.p["n_nodes"]) for c in cs} >= {(64, 93, 200), (128, 1, 300)}
    assert {len(c.walks) for c in cs} >= {1, 2, 5, 70}
    assert {len(w) for c in cs for w in c.walks} >= {1, 2, 7, 64, 65, 512}
    assert {c.p["cap_check"] for c in cs} == {0, 1}
    # where the drained node sits: lane 0, lane 63, lane 0 of word 1, the ragged last word, the only node, outside
    rows = {(c.name, int(r)) for c in cs for r in dc.walk_rows(c)}
    assert {("n64-w5", 0), ("n64-w5", 63), ("n65-w2", 64), ("n130-w5", 129), ("n257-w70", 256), ("n1-w1", 0)} <= rows
    c = dc.case("shard64-93of200")
    assert dc.walk_rows(c).tolist() == [0, 92, -1, 116] and c.p["tab_n"] == 93
    # the cordons: empty, one bit in another word than the drained node's, a whole word
    assert not dc.case("n64-w5").cordon and dc.case("n130-w5").cordon == {70} and 0 in dc.case("n130-w5").drain
    assert dc.case("n257-w70").cordon == set(range(64, 128))
    assert [int(w) for w in dc.excl_words(dc.case("n257-w70"))[:3]] == [0, 2 ** 64 - 1, 0]
    for c in cs:
        lo, nn = c.p["tab_lo"], c.p["tab_n"]
        assert c.p["stride"] > nn  # rows past tab_n, holding garbage
        assert all(abs(c.idle[r][0]) > 1e6 or c.idle[r][0] < 0 for r in range(nn, c.p["stride"])), c.name
        if nn >= 63:
            dead = [n for n in range(lo, lo + nn) if not c.live[n]]
            assert dead and all(abs(c.idle[n - lo][0]) > 1e6 or c.idle[n - lo][0] < 0 for n in dead), c.name
        assert [s["best_effort"] for s in c.shapes].count(True) == 1
        assert all(c.live[d] for d in c.drain if lo <= d < lo + nn)
    # garbage plane bits past the last node, in the stage planes and in the excluded plane
    c = dc.case("n65-w2")
    w = dc.planes_words(c).reshape(-1, c.p["W"])
    assert all(int(row[-1]) >> 1 == (1 << 63) - 1 for row in w)
    assert int(dc.excl_words(c)[-1]) >> 1 == (1 << 63) - 1 and int(dc.excl_words(c)[0]) == 1
    # together: placements from Idle and from Releasing, unplaced steps, a node taking several, several shapes a
    # walk, BestEffort steps that land, an exclusion that changed a place
    kinds, multi, shapes, be_lands, moved = set(), False, 0, 0, 0
    for c in cs:
        free = dr.walks(c, "drained_not_excluded")
        for w, wk, fr in zip(c.walks, dr.walks(c), free):
            kinds |= {(n >= 0, k) for n, k in wk}
            placed = [n for n, _ in wk if n >= 0]
            multi = multi or len(set(placed)) < len(placed)
            shapes = max(shapes, len(set(w)))
            be_lands += sum(1 for s, (n, _) in zip(w, wk) if c.shapes[s]["best_effort"] and n >= 0)
            moved += wk != fr
    assert kinds == {(True, 0), (True, 1), (False, 0)} and multi and shapes >= 5 and be_lands > 10 and moved > 10


# a hand case on which each defect must show
DEFECT_CASES = {"drained_not_excluded": "drained-is-the-lowest-fit", "cordon_ignored": "cordon-takes-the-first-fit",
                "exclusion_leaks": "exclusion-is-per-walk",
                "best_effort_resource_test": "best-effort-where-a-request-cannot",
                "best_effort_not_counted": "best-effort-fills-the-last-pod-slot",
                "cursor_across_walks": "cursor-is-per-walk", "idle_everywhere_first": "releasing-before-the-next-node",
                "no_overlay": "releasing-before-the-next-node", "guard_written": "the-only-node",
                "drained_row_as_node": "shard-70-of-200", "exclusion_needs_cap_check": "cap-check-off-still-excludes",
                "stops_at_unplaced": "unplaced-then-smaller"}


def test_defect_list_is_the_issue_s():
    assert set(DEFECT_CASES) == set(dr.DEFECTS) and len(dr.DEFECTS) == 12
    assert set(DEFECT_CASES.values()) <= set(dc.HAND)


@pytest.mark.parametrize("defect", dr.DEFECTS)
def test_comparator_reports_defect(defect):
    c = dc.case(DEFECT_CASES[defect])
    want = dr.walks(c)
    assert not dr.compare(c, want, dr.walks(c))
    assert not dc.compare_raw(c, dc.out_bytes(want))
    if defect != "guard_written":
        assert dr.compare(c, want, dr.walks(c, defect)), f"{defect} goes unnoticed on {c.name}"
    assert dc.compare_raw(c, dc.out_bytes(dr.walks(c, defect), defect))


@pytest.mark.parametrize("defect", [d for d in dr.DEFECTS if d != "guard_written"])
def test_seeded_cases_show_the_defect_too(defect):
    assert any(dr.compare(c, dr.walks(c), dr.walks(c, defect)) for c in map(dc.case, dc.SEEDED))


def test_the_cursor_changes_no_result():
    """The argument of kbg_device.hpp: a walk that starts each step at its
    `prev` step's node, and gives up where that step landed nowhere, is the
    plain walk (requests without a negative dimension; BestEffort shapes too)."""
    linked = 0
    for c in map(dc.case, dc.NAMES):
        for w, want in zip(c.walks, dr.walks(c)):
            prev, land = dr.links(c, w), [n - c.p["tab_lo"] if n >= 0 else -1 for n, _ in want]
            for i, p in enumerate(prev):
                if p >= 0:
                    linked += 1
                    assert land[i] == -1 or 0 <= land[p] <= land[i], (c.name, i)
    assert linked > 100
    c = dc.blank("negative", 2)
    dc.shape(c, 0, [-5.0, 0.0, 0.0])
    assert dr.links(c, [0, 0, 0]) == [-1, -1, -1]


def test_comparator_reports_one_overwritten_sentinel():
    c = dc.case("n65-w2")
    raw = dc.out_bytes(dr.walks(c))
    assert not dc.compare_raw(c, raw)
    bad = raw.copy()
    bad[sum(len(w) for w in c.walks) * 8 + 1234] ^= 0xFF
    assert any("guard" in e for e in dc.compare_raw(c, bad))
    bad = raw.copy()
    bad[4:8] = SENTINEL  # a step's kind left as the probe filled it
    assert dc.compare_raw(c, bad)


def test_layout_round_trip():
    c = dc.case("shard64-93of200")
    walks_, clean = dc.walks_of(c, dc.out_bytes(dr.walks(c)))
    assert clean and walks_ == dr.walks(c)
    assert dc.STEP.itemsize == 8 and dc.FIELDS[-2:] == ("n_walks", "n_steps")
    off, steps = dc.walk_offsets(c), dc.step_records(c)
    assert off.tolist() == [0, 64, 71, 78, 85] and len(steps) == 85 and off.dtype == np.dtype("<i4")
    for j, w in enumerate(c.walks):
        assert steps["shape"][off[j]:off[j + 1]].tolist() == w
        assert steps["prev"][off[j]:off[j + 1]].tolist() == dr.links(c, w)
    x = dc.excl_words(c)
    assert x.dtype == np.dtype("<u8") and len(x) == c.p["W"] == 4
    assert int(x[0]) == 1 << 3 and int(x[1]) == 1 << 1 and int(x[2]) == 1 << (190 - 128) and int(x[3]) >> 8 == (1 << 56) - 1


def test_row_of():
    places = [(7, -1, 0), (8, 2, 0), (9, 2, 1), (10, 5, 0), (11, -1, 0)]
    job = {7: 0, 8: 0, 9: 1, 10: 1, 11: 2}
    row = dr.row_of(places, job, {0: 3, 1: 2, 2: 1}, {0: 3, 1: 2, 2: 3})
    assert row == dict(walked=5, placed_idle=2, placed_releasing=1, unplaced=2, first_unplaced=7, nodes_used=2,
                       jobs_moved=3, jobs_short=1)  # job 0 loses its minimum; job 2 was not ready
    assert dr.row_of(places, job, {0: 4, 1: 2, 2: 1}, {0: 3, 1: 2, 2: 3})["jobs_short"] == 0
