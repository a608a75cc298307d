"""What the victim-reasons reference (tests/victim_why_ref.py) says on a
hand-worked table, what the seeded cases (tests/victim_why_cases.py) hold, and
that the comparator notices each of the named defects on some case. CPU only:
the kernels are held to the same reference by
tests/test_victim_why_kernels_gpu.py (device) and
tests/test_hostsim_victim_why.py (hostsim's launchers)."""
import numpy as np
import pytest

import victim_ref as vr
import victim_why_cases as wc
import victim_why_ref as wr

R1 = vr.R1  # 1000 / 1024 Mi / 1000
SMALL = (100, 100 * vr.MI, 100)


def hand_case():
    """Reclaim for job 0 (queue 0), request 300 / 300 Mi / 300, tiers [gang],
    [drf | proportion]. ls = 0.25 of totals 2^24 / 2^44 / 2^24.

    Jobs: `ok` (queue 1, min 3, ready 4: gang keeps it), `held` (queue 1, min
    3, ready 3: gang does not), `rich` (queue 2, allocation a quarter of the
    total and more: drf keeps it), `poor` (queue 3, allocation 2000: its share
    after the subtraction is far below ls, drf drops it). Queue 2 deserves
    nothing (proportion keeps), queue 3 deserves more than it has left
    (proportion drops), queue 1 is never asked in tier 2 with a victim left.

      node  candidates              what happens                                      cause
       0    ok R1                   gang keeps it; 1000 is not Less than 300          VICTIMS
       1    held R1, then rich R1   tier 1: gang drops held and keeps rich (min 1,
                                    ready 5): rich is the victim, 1000 covers 300     VICTIMS
       2    held R1                 tier 1 empty (gang); tier 2: drf: held's job
                                    allocation BIG stays above ls: kept; proportion:
                                    queue 1 deserved 0: kept -> victims               VICTIMS
       3    poor SMALL              queue 3; gang: min 1, ready 1 -> dropped; tier 2:
                                    drf drops (share ~0), proportion drops            NO_VICTIMS, all three fns empty
       4    poor2 SMALL             gang drops (min 2, ready 2); drf keeps (allocation
                                    2^23: share 1/2 > ls); proportion drops (queue 3) NO_VICTIMS, gang and proportion
       5    ok SMALL                gang keeps; 100 Less than 300 in all three        NOT_ENOUGH
       6    job 0's own task        queue 0 is the reclaimer's                        NO_PREEMPTEES
       7    ok R1, not Running      filtered                                          NO_PREEMPTEES
       8    ok R1, pod cap 7 of 7   cap before anything else                          POD_CAP
       9    ok R1, cap and selector both fail                                         POD_CAP
      10    ok R1, selector and unschedulable and taints fail                         SELECTOR
      11    ok R1, unschedulable and taints fail                                      UNSCHEDULABLE
      12    ok R1, taints fail                                                        TAINTS
      13    nil Node, selector fails too                                              PANIC
      14    under: job of queue 2 whose allocation is 20 short of its task: tier 1
            (gang) drops it (min 1, ready 1), tier 2's drf Sub underflows             PANIC
      15    ok R1, dead                                                               not visited
    """
    b = vr.Builder(vr.VM_RECLAIM, 0, req=(300, 300 * vr.MI, 300), ls=0.25)
    q1, q2 = b.queue(), b.queue()
    q3 = b.queue(alloc=(5000, 5000 * vr.MI, 5000), deserved=(4950, 0, 0))
    ok, held = b.job(q1, jmin=3, ready=4), b.job(q1, jmin=3, ready=3)
    rich = b.job(q2, jmin=1, ready=5, alloc=(2 ** 23, 2 ** 43, 2 ** 23))
    poor = b.job(q3, jmin=1, ready=1, alloc=(2000, 2048 * vr.MI, 2000))
    poor2 = b.job(q3, jmin=2, ready=2, alloc=(2 ** 23, 2 ** 43, 2 ** 23))
    under = b.job(q2, jmin=1, ready=1, alloc=(980, 1024 * vr.MI, 1000))
    b.node([(ok, R1)])
    b.node([(held, R1), (rich, R1)])
    b.node([(held, R1)])
    b.node([(poor, SMALL)])
    b.node([(poor2, SMALL)])
    b.node([(ok, SMALL)])
    b.node([(0, R1)])
    b.node([(ok, R1, 0)])
    b.node([(ok, R1)], ntasks=7, maxtasks=7)
    b.node([(ok, R1)], ntasks=8, maxtasks=7)
    for _ in range(3):
        b.node([(ok, R1)])
    b.node([(ok, R1)], panic=1)
    b.node([(under, R1)])
    b.node([(ok, R1)])
    c = b.finish("hand", 1)
    n = c.p["n_nodes"]
    c.live = [True] * 15 + [False]
    c.sel_ok = [[i not in (9, 10, 13) for i in range(n)]]
    c.unsched = [i in (10, 11) for i in range(n)]
    c.taint_ok = [[i not in (10, 11, 12) for i in range(n)]]
    wc.set_class_mask(c)
    c.queries = [dict(mode=vr.VM_RECLAIM, cls=0, cap_check=1, n_tiers=2, tier_fns=[1, 6], job=0, queue=0,
                      req=[300.0, 300.0 * vr.MI, 300.0], ls=0.25)]
    c.p["nq"] = 1
    return c


def test_hand_worked_table():
    c = hand_case()
    (r,) = wr.rows(c)
    want = {wr.VICTIMS: [0, 1, 2], wr.NO_VICTIMS: [3, 4], wr.NOT_ENOUGH: [5], wr.NO_PREEMPTEES: [6, 7],
            wr.POD_CAP: [8, 9], wr.SELECTOR: [10], wr.UNSCHEDULABLE: [11], wr.TAINTS: [12], wr.PANIC: [13, 14]}
    s = wr.state(c, prep=False)
    for k, nodes in want.items():
        for n in nodes:
            assert wr.cause(c, s, c.queries[0], n)[0] == k, (n, wr.CAUSE_NAMES[k])
    assert r["count"] == [2, 1, 0, 1, 1, 0, 2, 2, 1, 3, 2]
    assert r["first_node"] == [8, 10, -1, 11, 12, -1, 6, 3, 5, 0, 13]
    assert r["fn_empty"] == [2, 1, 2]  # gang: nodes 3 and 4; drf: node 3; proportion: nodes 3 and 4
    assert sum(r["count"]) == 15
    # predicates off: the stage nodes and the capped ones hold `ok R1` -> VICTIMS; the nil Node still panics
    c.queries[0]["cap_check"] = 0
    (r,) = wr.rows(c)
    assert r["count"] == [0, 0, 0, 0, 0, 0, 2, 2, 1, 8, 2]
    # no tier: every node with a preemptee is NO_VICTIMS and no fn is named
    c.queries[0].update(n_tiers=0, tier_fns=[])
    (r,) = wr.rows(c)
    assert r["count"][wr.NO_VICTIMS] == 12 and r["count"][wr.PANIC] == 1 and r["fn_empty"] == [0, 0, 0]


def test_intersection_empty_names_no_fn():
    """Gang keeps one task, proportion the other: NO_VICTIMS, and neither fn is empty by itself."""
    b = vr.Builder(vr.VM_RECLAIM, 0)
    qa = b.queue()  # deserves nothing: proportion keeps its tasks
    qb = b.queue(alloc=(5000, 5000 * vr.MI, 5000), deserved=(4950, 0, 0))  # proportion drops
    ja, jb = b.job(qa, jmin=3, ready=3), b.job(qb, jmin=3, ready=4)  # gang drops ja, keeps jb
    b.node([(ja, R1), (jb, R1)])
    c = b.finish("disjoint", 2)
    c.live, c.unsched, c.sel_ok, c.taint_ok = [True], [False], [[True]], [[True]]
    c.queries = [dict(mode=vr.VM_RECLAIM, cls=0, cap_check=1, n_tiers=1, tier_fns=[5], job=0, queue=0,
                      req=[300.0, 300.0 * vr.MI, 300.0], ls=0.0)]
    (r,) = wr.rows(c)
    assert r["count"][wr.NO_VICTIMS] == 1 and r["fn_empty"] == [0, 0, 0]


@pytest.fixture(scope="module")
def all_rows():
    return {name: wr.rows(wc.case(name)) for name in wc.NAMES}


def test_cases_hold_every_cause_and_fn(all_rows):
    seen, fn = set(), [0, 0, 0]
    for rows_ in all_rows.values():
        for r in rows_:
            seen |= {k for k in range(wr.N_CAUSES) if r["count"][k]}
            fn = [a + b for a, b in zip(fn, r["fn_empty"])]
    assert seen >= {0, 1, 3, 4, 6, 7, 8, 9, 10}, sorted(seen)
    assert all(fn), fn


@pytest.mark.parametrize("name", wc.NAMES)
def test_every_live_node_has_one_cause(all_rows, name):
    c = wc.case(name)
    lo, nn = c.p["node_lo"], c.p["node_n"]
    live = sum(c.live[lo:lo + nn])
    for r in all_rows[name]:
        assert sum(r["count"]) == live
        for k in range(wr.N_CAUSES):
            assert (r["first_node"][k] >= 0) == (r["count"][k] > 0)
            if r["count"][k]:
                assert lo <= r["first_node"][k] < lo + nn and c.live[r["first_node"][k]]


def test_cases_cover_the_shapes():
    nodes = {wc.case(n).p["node_n"] for n in wc.NAMES}
    assert nodes >= {1, 15, 16, 17, 63, 64, 65, 200}
    cands = set()
    for n in wc.NAMES:
        cands |= set(np.diff(wc.case(n).nt_off).tolist())
    assert cands >= {0, 1, 63, 64, 65, 127, 128, 129, 1024, 1025}
    assert {len(wc.case(n).queries) for n in wc.NAMES} >= {1, 2, 3, 17}
    assert {q["n_tiers"] for n in wc.NAMES for q in wc.case(n).queries} == {0, 1, 2}
    assert {q["cap_check"] for n in wc.NAMES for q in wc.case(n).queries} == {0, 1}
    for n in wc.NAMES:  # two equal queries wherever there is more than one
        qs = wc.case(n).queries
        assert len(qs) == 1 or any(qs[i] == qs[j] for i in range(len(qs)) for j in range(i))
    g = wc.case("big-group")
    assert sum(128 < L <= 1024 for L in np.diff(g.nt_off)[32:64]) >= 5


@pytest.mark.parametrize("defect", wr.DEFECTS)
def test_comparator_detects(all_rows, defect):
    hits = [name for name in wc.NAMES
            if wr.compare(wc.case(name), all_rows[name], wr.rows(wc.case(name), defect=defect))]
    assert hits, f"no case notices {defect}"


def test_class_mask_is_the_planes_product():
    for name in wc.NAMES:
        c = wc.case(name)
        for cls in range(c.p["classes"]):
            for n in range(c.p["n_nodes"]):
                want = c.sel_ok[cls][n] and c.taint_ok[cls][n] and not c.unsched[n] and c.live[n]
                assert bool(int(c.class_mask[cls, n >> 6]) >> (n & 63) & 1) == want
