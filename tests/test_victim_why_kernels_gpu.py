"""Kernel-level differential tests of kbg_victim_reasons' launches:
kbg_victim_why_kernel and kbg_victim_why_big_kernel run alone on flat arrays
through kbg_tool_probe_victim_why (kube-arbitrator_amd/tools/kernel_probe.cpp)
and the raw result rows, the guard region behind them and the input tables are
compared, bit for bit, with the plain reference of tests/victim_why_ref.py on
every case of tests/victim_why_cases.py. tests/test_victim_why_ref.py shows on
the CPU what the cases hold and that the comparison notices a subtly wrong
kernel. Every launch is a legal one: the probe rejects anything else on the
host."""
import pytest

import victim_why_cases as wc
from test_kernels_gpu import check_rc, params, probe, ptr  # noqa: F401  (probe is a fixture)
from victim_why_worker import check_illegal, illegal_launches

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", wc.NAMES)
def test_victim_why(probe, name):
    rc, errs = wc.check_probe(probe, wc.case(name), ptr, params)
    check_rc(probe, rc)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("ident", [x[0] for x in illegal_launches()])
def test_victim_why_probe_rejects_illegal_launches(probe, ident):
    """Nothing kbg_victim_reasons would never launch reaches the device."""
    errs = check_illegal(probe, ptr, params, ident)
    assert not errs, errs
