"""kbg_drain_kernel on the device: every case of tests/drain_cases.py through
kbg_tool_probe_drain, the raw places and the guard region compared with the
plain reference (tests/drain_ref.py), the node block and the stage planes
unchanged, and the launches the probe refuses."""
import ctypes

import pytest

import drain_cases as dc
from helpers import build_tools
from kbgpu import _abi
from test_kernels_gpu import params, ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    L = ctypes.CDLL(build_tools())
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    return L


@pytest.mark.parametrize("name", dc.NAMES)
def test_kernel_matches_the_reference(probe, name):
    errs = dc.check_probe(probe, dc.case(name), ptr, params)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("ident", [x[0] for x in dc.illegal_launches()])
def test_probe_refuses(probe, ident):
    errs = dc.check_illegal(probe, ptr, params, ident)
    assert not errs, "\n".join(errs)
