"""kbg_node_drain on the device: the session checks of tests/drain_session.py
(expected places from the fixture and the oracle's output without and with a
cordon, the invariants, the two paths, the limits, named nodes and duplicates,
the logs), the hand-worked walks, the Pending-twin check against
kbg_task_reasons, the one-target check against kbg_task_headroom, a resident
session over a churn chain and one structural batch against a fresh session,
and the refusals."""
import pytest

import drain_worker as dw
from kbgpu import _abi

pytestmark = pytest.mark.gpu
OPTS = None
# a subset of the hostsim seeds: the KATs, random8 and the contended seeds are answered by the kernel, random7 and
# ports1 on the host (moved pods with host ports), affinity500 on the host too, held to the invariants (the Python
# reference has no pod-affinity stage)
DEVICE_CASES = ["kat_task_why", "kat_reclaim", "kat_preempt", "random7", "random8", "contended6", "contended7",
                "contended19", "ports1", "affinity500"]
NO_EXPECTED_ROWS = ("affinity500",)


@pytest.fixture(scope="module", autouse=True)
def device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_session_rows_match_the_reference(case):
    errs, seen, skipped = dw.run_session_case(case, OPTS)
    assert not errs, "\n".join(errs[:20])
    assert skipped == (case in NO_EXPECTED_ROWS)


@pytest.mark.parametrize("case", ["kat_drain-hand", "dup-hand", "drain-hand", "drain-dev", "headroom", "twin-contended", "twin-affinity"])
def test_hand_worked_walks_and_the_other_queries(case):
    errs, _, _ = dw.run_session_case(case, OPTS)
    assert not errs, "\n".join(errs)


def test_resident_session():
    """Reset and update between cycles: the rows before and after each round's actions, at limits 2 and 512,
    against a fresh session's, task by uid and node by name."""
    errs, _, _ = dw.run_session_case("resident", OPTS)
    assert not errs, "\n".join(errs[:20])


def test_structural_batch():
    errs, _, _ = dw.run_session_case("structural", OPTS)
    assert not errs, "\n".join(errs[:20])


def test_refusals():
    errs, _, _ = dw.run_session_case("refusals", OPTS)
    assert not errs, "\n".join(errs)
