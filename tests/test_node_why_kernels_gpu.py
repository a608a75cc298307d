"""kbg_node_why_kernel on the device: every case of tests/node_why_cases.py
through kbg_tool_probe_node_why, the raw planes, their words past the listed
slots and the guard region compared with the plain reference
(tests/node_why_ref.py), the node table unchanged, and the launches the probe
refuses."""
import ctypes

import pytest

import node_why_cases as nc
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


@pytest.mark.parametrize("name", nc.NAMES)
def test_kernel_matches_the_reference(probe, name):
    errs = nc.check_probe(probe, nc.case(name), ptr, params)
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("ident", [x[0] for x in nc.illegal_launches()])
def test_probe_refuses(probe, ident):
    errs = nc.check_illegal(probe, ptr, params, ident)
    assert not errs, "\n".join(errs)
