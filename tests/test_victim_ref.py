"""CPU tests of the victim-scan kernel tests: the reference of
tests/victim_ref.py against hand-worked nodes, the claims of its cases (each
branch and edge the cases are meant to hold does occur in the expected
outputs), exactness of every float64 verdict against rational arithmetic, and
the sensitivity of cases and comparator to plausible kernel defects."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import victim_ref as vr
from victim_ref import MI, NONE, PANIC, STOP


@functools.lru_cache(maxsize=None)
def traced(name):
    """(verdict by node, events) of a case."""
    ev = set()
    return vr.verdicts(vr.case(name), events=ev), frozenset(ev)


@functools.lru_cache(maxsize=None)
def exp(name, out_mode, defect=None, prep=True):
    return vr.expected(vr.case(name), out_mode, defect, prep)


def one_node(b):
    c = b.finish("kat", 1)
    victims = []
    return vr.evaluate(c, vr.state(c), 0, victims_out=victims), victims


# ------------------------------------------------------ hand-worked nodes
def test_kat_reclaim_numbers():
    """tests/golden/make_kats.py kat_reclaim: gang keeps a1..a4; proportion's
    running allocation goes 4000 -> 3000 (victim: 2000 <= 3000), 2000
    (victim), 1000 (no), 0 (no); victims [a1, a2]."""
    b = vr.Builder(vr.VM_RECLAIM, vr.VP_GANG | vr.VP_PROP, req=(1000, 0, 0), total=(4000, 8 * 1024 * MI, 0))
    q1 = b.queue(alloc=(4000, 0, 0), deserved=(2000, 0, 0))
    a = b.job(q1, jmin=1, ready=4, alloc=(4000, 0, 0))
    b.node([(a, (1000, 0, 0))] * 4)
    assert one_node(b) == (STOP, [0, 1])


@pytest.mark.parametrize("ready,want", [(4, (STOP, [0, 1, 2, 3])), (3, (STOP, [0, 1, 2, 3])), (2, (NONE, []))])
def test_kat_preempt_numbers(ready, want):
    """kat_preempt: V (MinMember 2) stays >= 2 without a victim while it has
    4, then 3 ready tasks; at 2 gang keeps none."""
    b = vr.Builder(vr.VM_PREEMPT_JOBS, vr.VP_GANG, req=(1000, 0, 0))
    v = b.job(0, jmin=2, ready=ready, alloc=(4000, 0, 0))
    b.node([(v, (1000, 0, 0))] * 4)
    assert one_node(b) == want


def test_hand_made_proportion_nodes():
    b, n = vr.edge_prop()
    c = b.finish("x", 11)
    s = vr.state(c)
    got = {k: vr.evaluate(c, s, i) for k, i in n.items()}
    assert got == dict(skip=STOP, eq_noskip=STOP, prop_panic=PANIC, des_in=STOP, des_out=NONE, val_less=NONE,
                       val_one_dim=STOP, not_running=STOP, panic_class_off=NONE, panic_empty=PANIC, stop_plain=STOP,
                       cap_equal=NONE)
    victims = []
    vr.evaluate(c, s, n["skip"], victims_out=victims)
    assert victims == [1]  # the first was skipped without subtracting


def test_hand_made_drf_and_gang_nodes():
    b, n = vr.edge_drf()
    c = b.finish("x", 12)
    s = vr.state(c)
    assert {k: vr.evaluate(c, s, i) for k, i in n.items()} == dict(
        gpu_left=STOP, lt=STOP, close_in=STOP, close_out=NONE, neg_ok=STOP, neg_panic=PANIC, not_running=STOP)
    b, n = vr.edge_gang()
    c = b.finish("x", 13)
    s = vr.state(c)
    assert {k: vr.evaluate(c, s, i) for k, i in n.items()} == dict(yes=STOP, no=NONE, mixed=STOP)


def test_chunk_scenarios():
    """Every L gives NONE, STOP and PANIC nodes whose verdict rests on the
    last candidate, i.e. on every earlier subtraction."""
    for name in ["edge-chunks-main", "edge-chunks-big"] + [n for n in vr.NAMES if n.startswith("edge-drf-chunks")]:
        v, _ = traced(name)
        assert [v[n] for n in sorted(v)] == [NONE, STOP, PANIC] * (len(v) // 3)


# ------------------------------------------------------------------ claims
# claim (a branch or edge the reference records as it takes it) -> a case that holds it
CLAIMS = {
    "gang_min_eq_ready_minus_1": "edge-gang",
    "gang_min_eq_ready": "edge-gang",
    "drf_ls_lt_rs": "edge-drf",
    "drf_within_share_delta": "edge-drf",
    "drf_just_beyond_share_delta": "edge-drf",
    "drf_zero_total_zero_alloc": "edge-drf",
    "drf_zero_total_nonzero_alloc": "edge-drf",
    "drf_sub_negative_within_tolerance": "edge-drf",
    "drf_sub_panic": "edge-drf",
    "prop_less_skip": "edge-prop-cap1",
    "prop_one_dim_equal_no_skip": "edge-prop-cap1",
    "prop_sub_negative_within_tolerance": "edge-prop-cap1",
    "prop_sub_panic": "edge-prop-cap1",
    "deserved_le_inside_tolerance": "edge-prop-cap1",
    "deserved_le_at_tolerance": "edge-prop-cap1",
    "validate_sum_less": "edge-prop-cap1",
    "validate_one_dim_not_less": "edge-prop-cap1",
    "not_running_shares_job": "edge-drf",
    "not_running_shares_queue": "edge-prop-cap1",
    "filtered_shares_queue": "edge-gang",
    "panic_node_class_off": "edge-prop-cap1",
    "panic_node_empty": "edge-prop-cap1",
    "cap_equal_checked": "edge-prop-cap1",
    "cap_equal_unchecked": "edge-prop-cap0",
}


@pytest.mark.parametrize("claim", sorted(CLAIMS))
def test_claim_occurs(claim):
    """In its hand-made case, and (the cap pair aside) in a seeded one too."""
    assert claim in traced(CLAIMS[claim])[1]
    if not claim.startswith("cap_equal"):
        assert [n for n in vr.NAMES if not n.startswith("edge-") and claim in traced(n)[1]] or claim in (
            "prop_less_skip", "deserved_le_inside_tolerance", "deserved_le_at_tolerance", "drf_within_share_delta",
            "drf_just_beyond_share_delta"), claim


def test_every_mode_and_tier():
    seen = {(vr.case(n).p["mode"], vr.case(n).p["tier_fns"]) for n in vr.NAMES if vr.case(n).p["n_tiers"] == 1}
    assert {(m, f) for m in range(3) for f in range(1, 8)} <= seen
    assert any(vr.case(n).p["n_tiers"] == 0 for n in vr.NAMES)
    # each combination gives stops as well as nodes passed over
    for m in range(3):
        for f in range(1, 8):
            got = set()
            for n in vr.NAMES:
                p = vr.case(n).p
                if (p["mode"], p["tier_fns"], p["n_tiers"]) == (m, f, 1):
                    got |= set(traced(n)[0].values())
            assert {NONE, STOP} <= got, (m, f)


def test_geometry():
    ps = [vr.case(n).p for n in vr.NAMES]
    assert {1, 7, 8, 9, 63, 64, 65, 200} <= {p["n_nodes"] for p in ps}
    shards = {(p["node_lo"], p["node_n"] % 8 != 0) for p in ps}
    assert (64, True) in shards and (128, True) in shards
    assert any(p["W"] > 1 for p in ps) and any(p["cls"] > 0 for p in ps)
    assert any(p["W"] * 64 - p["n_nodes"] >= 64 for p in ps)  # a whole spare word
    counts = set()
    for n in vr.NAMES:
        c = vr.case(n)
        lo = c.p["node_lo"]
        counts |= set(np.diff(c.nt_off)[lo:lo + c.p["node_n"]].tolist())
    assert {0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 1023, 1024, 1025} <= counts
    assert {1, 4, 5} <= {p["n_rows"] for p in ps}
    c = vr.case("big-rows5")
    assert len({(c.p["node_lo"] + r) >> 5 for r in vr.big_rows(c)}) == 1  # five big nodes in one 32-bit word
    for n in vr.NAMES:  # integers below 2^53, the GPU dimension nonzero
        c = vr.case(n)
        if c.p["n_cand"]:
            assert (c.c_req == np.floor(c.c_req)).all() and (c.c_req < 2 ** 53).all()
    assert all((vr.case(n).c_req[:vr.case(n).p["n_cand"], 2] > 0).all() for n in vr.NAMES)
    assert max(vr.case(n).p["n_cand"] for n in vr.NAMES) < 20000


def test_cap_check_pair():
    """ntasks == maxtasks: passed over under cap_check, a stop without it."""
    b, n = vr.edge_prop()
    i = n["cap_equal"]
    assert traced("edge-prop-cap1")[0][i] == NONE and traced("edge-prop-cap0")[0][i] == STOP
    assert (exp("edge-prop-cap1", 0).stop != exp("edge-prop-cap0", 0).stop).any()


def test_panic_and_stop_share_a_byte():
    e = exp("edge-prop-cap1", 0)
    both = [b for b in range(2) if e.panic[b] and e.stop[b] & ~e.panic[b]]
    assert both


@pytest.mark.parametrize("name,h", [("edge-chunks-main", 1), ("edge-chunks-big", 2), ("edge-chunks-big", 15)])
def test_verdict_rests_on_earlier_chunks(name, h):
    """Nodes whose last candidate sits in chunk h (lane 0 and lane 63): with
    the subtractions of the chunks before it left out, the NONE and PANIC
    nodes come out differently."""
    c = vr.case(name)
    cnt = np.diff(c.nt_off)
    good, bad = traced(name)[0], vr.verdicts(c, "earlier_chunks_ignored")
    lanes = set()
    for n in good:
        if (cnt[n] - 1) // 64 == h and good[n] != bad[n]:
            assert good[n] in (NONE, PANIC) and bad[n] != good[n]
            lanes.add((cnt[n] - 1) % 64)
    assert lanes >= ({0} if h == 2 else {0, 63})


@pytest.mark.parametrize("L", [65, 128, 129, 961, 1024])
def test_drf_verdict_rests_on_earlier_chunks(L):
    """The same under drf: the job's running allocation over L mixed requests
    decides the last candidate, and with it the node."""
    c = vr.case(f"edge-drf-chunks-L{L}")
    good, bad = traced(c.name)[0], vr.verdicts(c, "earlier_chunks_ignored")
    assert [good[n] for n in range(3)] == [NONE, STOP, PANIC] and [bad[n] for n in range(3)] == [STOP, STOP, NONE]
    assert [vr.verdicts(c, "last_lane_lost")[n] for n in range(3)] == [NONE, NONE, NONE]


def test_layout():
    c = vr.case("shard64-61of200")
    e = exp(c.name, 1)
    wb = vr.victim_words(200) * 4
    assert len(e.stop) == wb + vr.GUARD_BYTES
    assert (e.stop[:8] == vr.SENTINEL).all() and (e.stop[16:] == vr.SENTINEL).all()  # bytes 8..15 are the range's
    assert not e.stop[15] >> 5 and not e.panic[15] >> 5  # nodes 125..127 are past the range
    assert e.stop[8:16].any() and (e.panic[8:16] & ~e.stop[8:16] == 0).all()
    c = vr.case("big-rows5")
    m, d = exp(c.name, 0), exp(c.name, 1)
    assert len(m.row_out) == 5 + vr.GUARD_BYTES and set(m.row_out[:5].tolist()) <= {0, 1, 3} and m.row_out[:5].any()
    assert (d.row_out == vr.SENTINEL).all()
    assert (m.stop != d.stop).any()  # mapped: the big nodes' bits are only in row_out
    assert traced(c.name)[0][37] == STOP  # (the reference itself has no bound)
    assert not (d.stop[37 >> 3] >> (37 & 7)) & 1  # 1025 candidates: reported nowhere


# --------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", vr.NAMES)
def test_verdicts_are_exact(name):
    """Every Sub / Less / LessEqual / share comparison recomputed with
    rationals gives the same branch: no float64 result of a case sits within
    rounding distance of a threshold."""
    c = vr.case(name)
    ev, exact, floats = set(), {}, {}
    assert vr.verdicts(c, events=ev, num=Fraction, victims=exact) == vr.verdicts(c, victims=floats)
    assert exact == floats  # every candidate's verdict, not only the node's
    assert ev == traced(name)[1]


# ------------------------------------------------------ defect sensitivity
@pytest.mark.parametrize("defect", vr.DEFECTS)
def test_defect_changes_an_expected_output(defect):
    found = []
    for name in vr.NAMES:
        c = vr.case(name)
        for out_mode in (0, 1):
            good, bad = exp(name, out_mode), vr.expected(c, out_mode, defect)
            errs = vr.compare(c, good, bad.stop, bad.panic, bad.row_out)
            same = all((getattr(good, k) == getattr(bad, k)).all() for k in ("stop", "panic", "row_out"))
            assert bool(errs) != same
            if errs:
                found.append((name, out_mode, errs[0]))
        if len(found) >= 2:
            break
    assert found, defect


@pytest.mark.parametrize("defect", ["earlier_chunks_ignored", "before_own_subtraction", "last_lane_lost",
                                    "sum_preemptees", "c_run_ignored"])
def test_defect_shows_on_a_big_node(defect):
    """The big-node kernel has its own walk: these defects change a verdict
    of a node of more than 128 candidates too."""
    hit = False
    for name in vr.NAMES:
        c = vr.case(name)
        if c.p["n_rows"]:
            hit = hit or (exp(name, 0).row_out != vr.expected(c, 0, defect).row_out).any()
    assert hit


def test_comparator_reports_guard_and_outside_bytes():
    c = vr.case("shard64-61of200")
    e = exp(c.name, 1)
    stop = e.stop.copy()
    stop[0] = 0
    stop[-1] = 0
    stop[15] |= 0x80
    errs = vr.compare(c, e, stop, e.panic, e.row_out)
    assert len(errs) == 3 and "outside the range" in errs[0] and "past the range" in errs[1] and "guard" in errs[2]


# -------------------------------------------------------- prep sensitivity
@pytest.mark.parametrize("name", [n for n in vr.NAMES if n.startswith("prep-")])
def test_prep_changes_the_scan(name):
    c = vr.case(name)
    assert (exp(name, 0).stop != exp(name, 0, None, False).stop).any()
    t = vr.prepped_tables(c)
    changed = [(t.block != vr.table_block(c)).any(), (t.c_run != c.c_run).any(), (t.j_ready != c.j_ready).any(),
               (t.j_alloc != c.j_alloc).any(), (t.q_alloc != c.q_alloc).any()]
    assert changed[0] == (c.p["nn"] > 0) and any(changed[1:]) == (c.p["ns"] > 0)


def test_prep_cases_cover_the_paths():
    p = {n: vr.case(n).p for n in vr.NAMES if n.startswith("prep-")}
    assert any(q["prep"] == 1 and q["nn"] == vr.ARG_NODE_DELTAS and q["ns"] == vr.ARG_STATE_DELTAS for q in p.values())
    assert any(q["prep"] == 2 and q["nn"] + q["ns"] > 256 and 0 < q["nn"] < 256 for q in p.values())
    for prep in (1, 2):
        assert any(q["prep"] == prep and q["nn"] == 0 for q in p.values())
        assert any(q["prep"] == prep and q["ns"] == 0 for q in p.values())
    for n, q in p.items():
        if q["ns"] >= 20:
            assert set(vr.case(n).sd["kind"].tolist()) == {0, 1, 2, 3}, n
