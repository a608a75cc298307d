"""The in-order commit's dead masks through the device path: the
saturated and the hand-made sessions of tests/dead_masks_cases.py, production
and full-scan mode with batch_tasks=64, with the masks and with
KBG_DEAD_MASKS=0 — equal to each other and to the kbref oracle, the re-checks
of the saturated sessions at least halved (tests/test_dead_masks.py is the
same on hostsim, with more cases)."""
import pytest

import dead_masks_cases as dm
from helpers import compare_outputs, run_oracle
from test_dead_masks import check_edges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_device():
    from kbgpu import _abi
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")


@pytest.mark.parametrize("case", dm.GPU_CASES, ids=[c["id"] for c in dm.GPU_CASES])
def test_masks_change_no_output_on_the_device(case):
    rec = dm.run_case(case)
    on, off = rec["on"], rec["off"]
    assert "error" not in on and "error" not in off, (on.get("error"), off.get("error"))
    assert on["out"] == off["out"]
    compare_outputs(run_oracle(dm.make_fixture(case)), on["out"])
    if case["gen"] == "edges":
        check_edges(on["out"])
    else:
        print(case["id"], "re-checks", off["stats"]["resolve_rechecks"], "->", on["stats"]["resolve_rechecks"])
        assert off["stats"]["resolve_rechecks"] > 0, (on["stats"], off["stats"])
        assert on["stats"]["resolve_rechecks"] <= 0.5 * off["stats"]["resolve_rechecks"], (on["stats"], off["stats"])
