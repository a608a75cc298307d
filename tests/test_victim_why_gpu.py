"""kbg_victim_reasons on the device: the session checks of
tests/test_hostsim_victim_why.py (tests/victim_why_session.py: rows against
the reference on tables built from the fixture, the Python cache mirror and
the oracle's output of the same actions; the cycle with the calls in between
against the oracle's; the host-port twins that take host_why; the node of
1025 Running candidates; a resident session updated between cycles; the
refusals) through libkbgpu.so on the MI355X, at the same small sizes, and the
hand-derived rows of tests/golden/kat_victim_why.json
(tests/golden/make_kat_victim_why.py holds the derivation)."""
import pytest

import victim_why_worker as ww
from kbgpu import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


@pytest.mark.parametrize("case", ww.SESSION_CASES)
def test_session_rows_match_the_reference(case):
    errs, _ = ww.run_session_case(case)
    assert not errs, "\n".join(errs[:20])


def test_abi_structure_matches_the_header():
    """kbg_victim_why is 32 int32 words: valid, task, visited, queue_overused, count[11], first_node[11],
    fn_empty[3], reserved[3]."""
    import ctypes
    assert ctypes.sizeof(_abi.kbg_victim_why) == (4 + 11 + 11 + 3 + 3) * 4
    assert _abi.kbg_victim_why.count.offset == 16 and _abi.kbg_victim_why.fn_empty.offset == 16 + 88
