"""Queue and job names that return to a resident session, on the device
(include/kbgpu.h kbg_session_update, KBG_EV_QUEUE_ADD / KBG_EV_JOB_ADD): the
hand-made cases of tests/revival_cases.py, six generated seeds, the raw-ABI
cases over two updates and the refused batch that must leave nothing
recorded. The bodies are tests/revival_session.py (the simulated stream runs
the same ones over the whole seed list, tests/test_revival_hostsim.py): a
round that must be accepted equals a fresh session on the replayed cache and
the oracle where a fixture can say it; a round that must be refused is refused
by the wrapper and by the library, the four renumberings stay empty, the next
cycle equals the one before, and a valid batch sent right after still applies.
Nothing here skips."""
import pytest

from revival_cases import CASES, EXPECT, GPU_SEEDS

pytestmark = pytest.mark.gpu

kbgpu = pytest.importorskip("kbgpu")
import revival_session  # noqa: E402


@pytest.mark.parametrize("case", sorted(CASES))
def test_revival_case(case):
    want = revival_session.run_case(case)
    assert [v.round for v in want if v is not None] == ([] if EXPECT[case] is None else [EXPECT[case][0]])


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_revival_fuzz(seed):
    revival_session.run_seed(seed, {"batch_tasks": 1 + seed % 7, "full_scan": seed % 2})


@pytest.mark.parametrize("what", sorted(revival_session.SPECIALS))
def test_revival_session(what):
    revival_session.SPECIALS[what]()
