"""CPU tests of the kernel tests (tests/test_kernels_gpu.py): that every
first-fit case contains what it claims, that the plain reference of
tests/kernel_ref.py agrees with exact arithmetic and with deliberately naive
loops, and that the comparator rejects a reference output carrying one defect
at a time, naming the shape and the word. No GPU is needed and nothing here
launches a kernel."""
from fractions import Fraction

import numpy as np
import pytest

import kernel_cases as kc
import kernel_ref as kr


# ------------------------------------------------------ coverage conditions
@pytest.mark.parametrize("name", kc.FF_NAMES)
def test_case_holds_what_it_claims(name):
    case = kc.ff_case(name)
    kc.check_claims(case, kr.ff_reference(case))


def test_every_claim_is_made_somewhere():
    claims = set().union(*(kc.ff_case(n).claims for n in kc.FF_NAMES))
    assert claims == {"cut", "uncut", "nofit", "last_word_fit", "rel_only", "rel_words", "garbage_mask"}


def test_matrix_launches_every_instantiation():
    """{int, general} x {complete, full-scan, early-exit} x {16, 24, 32} rows."""
    got = {kc.instantiation(kc.ff_case(n)) for n in kc.FF_NAMES}
    assert got == {(m, w, r) for m in ("int", "general") for w in ("complete", "full-scan", "early-exit")
                   for r in (16, 24, 32)}


def test_geometry_of_the_row_cases():
    assert [kr.firstfit_geometry(G, False) for G in (1, 16, 17, 40, 4096, 4100, 6144, 6200)] == \
        [(16, 16)] * 5 + [(24, 24)] * 2 + [(32, 32)]
    assert [kr.firstfit_geometry(G, True) for G in (40, 600, 4300, 7000)] == [(16, 2), (16, 4), (24, 18), (32, 28)]


def test_want_ends_lists_in_every_place():
    """Cut lists end in the first 64-word chunk of the first round, in its
    second chunk and in a later round."""
    case = kc.ff_case("words300-ee1-gen")
    cov = kr.ff_reference(case).covered[:, 0]
    cut = cov[(cov >= 0) & (cov < 300)]
    assert (cut <= 64).any() and ((cut > 64) & (cut <= 128)).any() and (cut > 128).any()


# ------------------------------------------- reference vs exact arithmetic
def _edge_pairs(int_mode):
    reqs, pools = kc.value_pools(int_mode)
    return [(d, q, a) for d in range(3) for q in reqs[d] for a in pools[d].tolist()]


def test_less_equal_agrees_with_fractions_on_the_tolerance_edges():
    exact = 0
    for d, q, a in _edge_pairs(False):
        fq, fa, mn = Fraction(q), Fraction(a), Fraction(kr.K_MIN[d])
        if Fraction(float(np.float64(a) - np.float64(q))) != fa - fq:
            continue  # the float64 difference rounds: Go rounds it the same way, exact arithmetic does not
        exact += 1
        assert bool(kr.less_equal(q, a, kr.K_MIN[d])) == (fq < fa or abs(fa - fq) < mn), (d, q, a)
    assert exact > 100
    # the edges themselves: |a - r| == min does not fit, one ulp inside does, r below a by one ulp does
    # (requests large enough for the difference to be exact: at 7.25 - 10 the ulp inside rounds back to 10)
    for q, mn in ((64000.0, kr.K_MIN[0]), (4.0 * 2 ** 30, kr.K_MIN[1])):
        assert not kr.less_equal(q, q - mn, mn) and kr.less_equal(q, np.nextafter(q - mn, np.inf), mn)
        assert not kr.less_equal(q, np.nextafter(q - mn, -np.inf), mn)
        assert kr.less_equal(q, q + mn, mn) and kr.less_equal(np.nextafter(q, -np.inf), q, mn)
    assert kr.less_equal(-0.0, 0.0, 10.0) and kr.less_equal(0.0, -0.0, 10.0)


def test_integer_thresholds_agree_with_exact_integers():
    """kbg_device.hpp TaskRec: on exact integers `req <= a` (LessEqual) is
    `a > req - min`, with req - min formed in float64 as the host forms it."""
    for d, q, a in _edge_pairs(True):
        mn = kr.K_MIN_INT[d]
        exact = q < a or abs(a - q) < mn  # Python integers
        assert bool(np.float64(a) > kr.threshold(q, mn)) == exact, (d, q, a)
        assert bool(kr.less_equal_int(np.int64(q), np.int64(a), mn)) == exact
        assert bool(kr.less_equal(float(q), float(a), kr.K_MIN[d])) == exact
    assert max(max(q) for q in kc.value_pools(True)[0]) > 2 ** 50


def test_select_reference_agrees_with_a_naive_loop():
    for name in ("t16-1slot", "t17-3slots", "t64-3slots-inner"):
        for int_mode in (True, False):
            c = kc.scan_case(name, int_mode)
            w_lo, w_hi = c["p"]["w_lo"], c["p"]["w_hi"]
            cand, count = kr.select_reference(c["F"], c["FI"], w_lo, w_hi, c["cap_off"])
            for t in range(c["p"]["n_tasks"]):
                M = int(c["cap_off"][t + 1] - c["cap_off"][t])
                got, more = [], False
                for node in range(w_lo * 64, w_hi * 64):
                    if (int(c["F"][t, node >> 6]) >> (node & 63)) & 1:
                        if len(got) == M:
                            more = True
                            break
                        idle = (int(c["FI"][t, node >> 6]) >> (node & 63)) & 1
                        got.append(node | (0 if idle else kr.CAND_PIPELINE_BIT))
                o = int(c["cap_off"][t])
                assert cand[o:o + len(got)].tolist() == got
                assert (cand[o + len(got):o + M] == 0xA5A5A5A5).all()
                assert int(count[t]) == len(got) | (kr.COUNT_INCOMPLETE_BIT if more else 0)


def test_scan_reference_layout():
    """[slot][plane][quad][row][4]: every (row, word < W) once, the rest sentinel."""
    c = kc.scan_case("t17-3slots", False)
    n, Wl, W = 17, 7, 19
    sw = 8
    for t in (0, 16):
        for w in (0, 6, 7, 18):
            slot, lw = divmod(w, Wl)
            o = slot * 2 * n * sw + ((lw >> 2) * n + t) * 4 + (lw & 3)
            assert c["bits"][o] == c["F"][t, w] and c["bits"][o + n * sw] == c["FI"][t, w]
    assert (c["bits"] != 0xA5A5A5A5A5A5A5A5).sum() <= 2 * n * W


def _fitdelta_naive(c):
    """The same counts by replaying each node's log backwards."""
    tab, out = c["tab"], []
    for q in c["q"]:
        cnt = [0, 0, 0, 0]
        for n in range(tab.tab_lo, min(int(q["end"]), tab.tab_lo + tab.tab_n)):
            if not (int(tab.class_mask[int(q["cls"]), n // 64]) >> (n % 64)) & 1:
                continue
            idle = [float(tab.idle[d][n]) for d in range(3)]
            pods = int(tab.ntasks[n])
            for e in range(int(c["hoff"][n + 1]) - 1, int(c["hoff"][n]) - 1, -1):
                if (int(c["hk"][e]) & 0x7FFFFFFF) < int(q["point"]):
                    break
                pods -= 1
                if int(c["hk"][e]) >= 0:  # an Allocate: the Idle before it
                    idle = [float(x) for x in c["hold"][e]]
            req = [float(x) for x in q["req"]]
            fits = all(kr.less_equal(req[d], idle[d], kr.K_MIN[d]) for d in range(3))
            if (c["p"]["cap_check"] and pods >= int(tab.maxtasks[n])) or (fits and n != int(q["win"])):
                continue
            cnt[0] += 1
            for d in range(3):
                cnt[1 + d] += (idle[d] - (req[d] + kr.K_MIN[d]) if req[d] > 0 else idle[d]) < 0
        out.append(cnt)
    return out


@pytest.mark.parametrize("window,cap", [(None, 1), ((70, 61), 1), (None, 0)])
def test_fitdelta_reference_agrees_with_a_naive_loop(window, cap):
    c = kc.make_fit_case(11 + cap, 150, (1, 64, 70, 150, 131), window=window, cap_check=cap)
    ref = kr.fitdelta_reference(c["tab"], c["hoff"], c["hk"], c["hold"], c["q"], cap)
    nq = c["p"]["nq"]
    assert nq % 2 == 1
    assert ref[:4 * nq].reshape(nq, 4).tolist() == _fitdelta_naive(c)
    assert ref[:4 * nq].any()


def test_fitdelta_cases_hold_what_they_claim():
    c = kc.fit_case("ends")
    per_node = np.diff(c["hoff"])
    alloc = np.add.reduceat((c["hk"] >= 0).astype(int), c["hoff"][:-1][per_node > 0])
    assert (per_node == 0).any() and (alloc == 0).any()          # no decisions; Pipelines only
    e = np.flatnonzero((c["hk"][:-1] < 0) & (c["na"][:-1] > np.arange(len(c["na"]) - 1)))
    assert len(e), "no Allocate after a Pipeline on one node"
    assert {int(x) for x in c["q"]["end"]} >= {1, 63, 64, 65, 1024, 1025, 2100}
    assert len({int(x) for x in c["q"]["end"][0:2]}) == 2          # one workgroup, two ends
    w = kc.fit_case("window")
    assert w["p"]["tab_lo"] > 0 and w["p"]["tab_lo"] + w["p"]["tab_n"] < w["p"]["n_nodes"]


# ------------------------------------------------- comparator sensitivity
@pytest.fixture(scope="module")
def cut():
    """A cut list of a multi-round case: (case, expected, shape, part, first
    word, covered), with a covered last word whose planes differ."""
    case = kc.ff_case("splits3-w300-gen")
    exp = kr.ff_reference(case)
    p = case.p
    for s in np.flatnonzero(case.writers()):
        for k, (lo, hi) in enumerate(case.parts()):
            cov = int(exp.covered[s, k])
            o = (s * p["mw"] + lo + cov - 1 - p["mask_w0"]) * 2
            if 1 < cov < hi - lo and exp.masks[o] != exp.masks[o + 1]:
                return case, exp, int(s), k, lo, cov
    raise AssertionError("no cut list with a Releasing-only fit in its last covered word")


def _defects(case, exp, s, k, lo, cov):
    p = case.p
    last = (s * p["mw"] + lo + cov - 1 - p["mask_w0"]) * 2
    i = s * p["info_stride"] + p["part0"] + k
    word, part = f"shape {s} word {lo + cov - 1} ", f"shape {s} part {k} "

    def masks(f):
        m = exp.masks.copy()
        f(m)
        return exp.info, m

    def info(f):
        n = exp.info.copy()
        n[i] = f(int(n[i]))
        return n, exp.masks

    def setw(o, v):
        def f(m):
            m[o] = v
        return f
    return {
        "bit flipped in the last covered word": (masks(setw(last, exp.masks[last] ^ np.uint64(1 << 17))), word),
        "Idle plane equal to the fit plane": (masks(setw(last + 1, exp.masks[last])), word),
        "covered one too many": (info(lambda v: v + 1), part),
        "covered one too few": (info(lambda v: v - 1), part),
        "incomplete bit dropped": (info(lambda v: v & ~kr.COUNT_INCOMPLETE_BIT), part),
        "any bit dropped": (info(lambda v: v & ~kr.INFO_ANY_BIT), part),
        "sentinel byte overwritten past covered": (masks(setw(last + 2, exp.masks[last + 2] ^ np.uint64(0xFF))),
                                                   f"shape {s} word {lo + cov} "),
        "guard byte overwritten": (masks(setw(len(exp.masks) - 1, exp.masks[-1] ^ np.uint64(0xFF << 56))), "guard"),
        "info guard byte overwritten": ((np.concatenate([exp.info[:-1], exp.info[-1:] ^ np.uint32(1)]), exp.masks),
                                        "guard"),
    }


DEFECTS = ("bit flipped in the last covered word", "Idle plane equal to the fit plane", "covered one too many",
           "covered one too few", "incomplete bit dropped", "any bit dropped", "sentinel byte overwritten past covered",
           "guard byte overwritten", "info guard byte overwritten")


def test_comparator_accepts_the_reference(cut):
    case, exp = cut[:2]
    assert kr.ff_compare(case, exp, exp.info.copy(), exp.masks.copy()) == []
    assert int(exp.info[cut[2] * case.p["info_stride"] + case.p["part0"] + cut[3]]) & kr.COUNT_INCOMPLETE_BIT


@pytest.mark.parametrize("defect", DEFECTS)
def test_comparator_rejects_one_defect(cut, defect):
    (info, masks), names = _defects(*cut)[defect]
    errs = kr.ff_compare(cut[0], cut[1], info, masks)
    assert len(errs) == 1 and names in errs[0], errs
