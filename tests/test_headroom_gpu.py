"""kbg_task_headroom on the device: the session checks of
tests/headroom_session.py (expected rows from the fixture and the oracle's
output, the invariants against kbg_task_reasons, the two paths, the logs),
the hand-derived KATs, the clusters on which the oracle's own allocate places
identical copies until none fits, a resident session over a churn chain (reset and
update between cycles) against a fresh session and the reference, and the refusals."""
import pytest

import headroom_session as hs
import headroom_worker as hw
from kbgpu import _abi

pytestmark = pytest.mark.gpu
OPTS = None
# a subset of the hostsim seeds: every generator, cycles that evict among them, none whose cycle discards a
# statement; the KATs, random8 and the contended seeds hold no host port, pod affinity or nil Node: the kernel answers
DEVICE_CASES = ["kat_task_why", "kat_reclaim", "kat_preempt", "random7", "random8", "contended6", "contended7",
                "contended19", "ports1", "affinity500"]


@pytest.fixture(scope="module", autouse=True)
def device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_session_rows_match_the_reference(case):
    errs, seen, skipped = hw.run_session_case(case, OPTS)
    assert not errs, "\n".join(errs[:20])
    assert not skipped


@pytest.mark.parametrize("name", ["kat_headroom", "kat_headroom_dev"])
def test_hand_derived_kat(name):
    errs = hs.check_kat(hw.session_fixture(name))
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("name", hw.ALLOCATE)
def test_row_is_what_the_oracle_s_allocate_places(name):
    errs = hs.check_allocate(hs.allocate_fixtures()[name])
    assert not errs, "\n".join(errs[:20])


def test_resident_session():
    """Reset and update between cycles: the rows before and after each round's actions, at two limits, against a
    fresh session's and against the reference on the round's fixture and the oracle's output."""
    errs, _, _ = hw.run_session_case("resident", OPTS)
    assert not errs, "\n".join(errs[:20])


def test_refusals():
    errs = hs.check_refusals(hw.session_fixture("kat_task_why"))
    assert not errs, "\n".join(errs)
