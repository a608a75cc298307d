"""kbg_task_headroom_kernel on the device: every case of
tests/headroom_cases.py through kbg_tool_probe_task_headroom, the raw rows and
the guard region compared with the plain reference (tests/headroom_ref.py),
and the launches the probe refuses."""
import ctypes

import pytest

import headroom_cases as hc
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


@pytest.mark.parametrize("name", hc.NAMES)
def test_kernel_matches_the_reference(probe, name):
    errs = hc.check_probe(probe, hc.case(name), ptr, params)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("ident", [x[0] for x in hc.illegal_launches()])
def test_probe_refuses(probe, ident):
    errs = hc.check_illegal(probe, ptr, params, ident)
    assert not errs, "\n".join(errs)
