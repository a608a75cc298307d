"""kbg_job_fit on the device: the session checks of tests/job_fit_session.py
(expected places from the fixture and the oracle's output, the invariants
against kbg_task_reasons and kbg_task_headroom, the two paths, the limits, the
logs), the hand-derived walks, single jobs against the oracle's own allocate,
a resident session over a churn chain and one structural batch against a fresh
session, and the refusals."""
import pytest

import job_fit_session as js
import job_fit_worker as jw
from kbgpu import _abi

pytestmark = pytest.mark.gpu
OPTS = None
# a subset of the hostsim seeds: every generator; the KATs, random8 and the contended seeds hold no host port, pod
# affinity, nil Node or colliding pod key: the kernel answers
DEVICE_CASES = ["kat_task_why", "kat_reclaim", "kat_preempt", "random7", "random8", "contended6", "contended7",
                "contended19", "ports1", "affinity500"]
ALLOCATE = ["hand", "dev"] + [f"seed{s}" for s in js.ALLOCATE_SEEDS[:6]]


@pytest.fixture(scope="module", autouse=True)
def device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_session_rows_match_the_reference(case):
    errs, seen, skipped = jw.run_session_case(case, OPTS)
    assert not errs, "\n".join(errs[:20])
    assert skipped == (case == "affinity500")


@pytest.mark.parametrize("case", ["kat_job_fit-hand", "gang-hand", "gang-dev"])
def test_hand_derived_walks(case):
    errs, _, _ = jw.run_session_case(case, OPTS)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("name", ALLOCATE)
def test_places_are_the_oracle_s_allocate(name):
    fx = js.allocate_fixtures()[name]
    picks = js.allocate_picks(fx)
    if picks is not None:  # (left out on the CPU: tests/test_hostsim_job_fit.py counts them)
        errs, shown, _ = js.check_allocate(fx, picks)
        assert not errs, "\n".join(errs[:20])


def test_resident_session():
    """Reset and update between cycles: the rows before and after each round's actions, at limits 2 and 512,
    against a fresh session's, task by uid and node by name."""
    errs, _, _ = jw.run_session_case("resident", OPTS)
    assert not errs, "\n".join(errs[:20])


def test_structural_batch():
    errs, _, _ = jw.run_session_case("structural", OPTS)
    assert not errs, "\n".join(errs[:20])


def test_refusals():
    errs, _, _ = jw.run_session_case("refusals", OPTS)
    assert not errs, "\n".join(errs)
