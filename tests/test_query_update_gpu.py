"""The seven query calls on device sessions after update events:
tests/query_update_session.py's check_rounds on a subset of the hostsim cases
(tests/test_hostsim_query_update.py) that keeps every hand-made case and at
least four seeds per family, one case per test. A session is asked, updated
and asked again; every point asks all seven calls of the one session, in an
order that rotates with the point, and is compared with a fresh session on the
replayed cache and with the references on the fixture after the events and
the oracle's output (kbg_job_fit at limits 2 and 512, kbg_node_drain at both
without a cordon and at 512 with one). The seeded cases run twice: with the
defaults and with query_update_session.HOST_SWITCHES set (KBG_HOST_TASK_WHY,
KBG_HOST_TASK_HEADROOM, KBG_HOST_JOB_FIT, KBG_HOST_NODE_WHY,
KBG_HOST_NODE_DRAIN), so the kernels and the host path must agree with the
same references after an update too."""
import pytest

import query_update_cases as qc
import query_update_session as qs
import query_update_worker as qw
from kbgpu import _abi

pytestmark = pytest.mark.gpu
OPTS = None
HAND = [f"{fam}/{fn.__name__}" for fam, fns in qc.HAND.items() for fn in fns] + [f"in_place/{n}" for n in qc.ue.IN_PLACE]
SEEDED = ["structural/random24", "structural/contended1", "structural/contended35", "structural/ports13",
          "structural/affinity35", "in_place/fuzz15", "in_place/fuzz23", "in_place/fuzz27", "in_place/fuzz45",
          "recompile/relabel4", "recompile/relabel5", "recompile/relabel8", "recompile/relabel18",
          "chain/contended13", "chain/contended108", "chain/contended167"]


@pytest.fixture(scope="module", autouse=True)
def device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


def check(case):
    rec = qw.run_case(case, OPTS)
    assert not rec["errors"], "\n".join(rec["errors"][:20])
    assert rec["skipped"] is None, f"a committed case was skipped: {rec['skipped']}"
    print(f"{case}: {rec['rows']} rows against the fresh session, {rec['rows_ref']} against the references")
    assert rec["ref"] and rec["rows"] > 0 and rec["rows_ref"] > 0, rec
    assert min(rec["answered"]) > 0, rec
    # (the walks' reference has no pod-affinity stage: on such fixtures kbg_node_reasons alone is held to its own)
    for what in ("node",) if any(rec["pod_affinity"]) else ("fit", "node", "drain"):
        assert rec["rows_ref_by"].get(what, 0) > 0, (what, rec["rows_ref_by"])
    return rec


def test_subset_is_of_the_committed_cases():
    cases = qc.all_cases()
    assert set(HAND + SEEDED) <= set(cases)
    assert {f"{fam}/{fn.__name__}" for fam, fns in qc.HAND.items() for fn in fns} <= set(HAND)
    for fam in ("structural", "in_place", "recompile"):
        assert sum(cases[c][0] == fam for c in SEEDED) >= 4, fam


@pytest.mark.parametrize("case", HAND)
def test_hand_made_case(case):
    rec = check(case)
    if case.endswith("pod_group_add_new_class"):  # one more class: larger stage planes behind the same pointers
        assert rec["n_classes"][1] > rec["n_classes"][0], rec["n_classes"]
        assert rec["rebuilds"] == [1]


def test_entry_point_of_one_update():
    errs = qw.run_entry("recompile/relabel_hand", OPTS)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("case", SEEDED)
def test_seeded_case(case):
    check(case)


@pytest.mark.parametrize("case", SEEDED)
def test_seeded_case_on_the_host_paths(case):
    with qs.host_paths():
        check(case)
