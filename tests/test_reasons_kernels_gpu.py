"""kbg_stage_mask_kernel and kbg_reasons_kernel launched alone through the
probes of the tool library (kube-arbitrator_amd/tools/kernel_probe.cpp) and
compared, word for word, with the plain references of
tests/reasons_kernel_ref.py (checked on the CPU by
tests/test_reasons_kernel_ref.py), guard regions included. Node counts at the
word edge (63, 64, 65), at the 1024-lane pass edge (1024, 1025) and past two
passes (2100); 1, 2, 3, 5 queries (odd groups of the kernel's queries per
workgroup); visited ranges ending inside a word, at node 0 and empty; a reason
at the last lane of the last word only, a reason nowhere; nodes with 40
decisions; the pod cap check on and off."""
import ctypes

import numpy as np
import pytest

import kernel_ref as kr
import reasons_kernel_ref as rr
from helpers import build_tools

pytestmark = pytest.mark.gpu

kbgpu = pytest.importorskip("kbgpu")
from kbgpu import _abi  # noqa: E402

FIT_FIELDS = ("n_nodes", "W", "stride", "classes", "tab_lo", "tab_n", "nq", "cap_check", "n_dec")
STAGE_FIELDS = ("n_nodes", "W", "classes", "label_words", "taint_words", "n_numcols", "n_reqs", "n_terms",
                "mask_pool_words", "tol_pool_words")


def params(fields, p):
    return (ctypes.c_int32 * len(fields))(*[int(p[f]) for f in fields])


def ptr(a):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def probe():
    L = ctypes.CDLL(build_tools())
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    L.kbg_tool_probe_stage_mask.restype = ctypes.c_int32
    L.kbg_tool_probe_reasons.restype = ctypes.c_int32
    assert L.kbg_tool_probe_guard_bytes() == kr.GUARD_BYTES and L.kbg_tool_probe_sentinel() == kr.SENTINEL
    return L


def check_rc(probe, rc):
    """A HIP error ends the run: nothing more is launched on a device that
    reported one."""
    if rc == -3:
        pytest.exit(f"HIP error in a kernel probe: {probe.kbg_tool_probe_error()}", returncode=3)
    assert rc == 0, (rc, probe.kbg_tool_probe_error())


@pytest.mark.parametrize("n_nodes", rr.NODE_COUNTS)
def test_stage_mask(probe, n_nodes):
    t = rr.stage_case(9000 + n_nodes, n_nodes)
    sel, tol, uns, live, cm = rr.stage_reference(t)
    C, W = len(t["classes"]), t["W"]
    p = dict(t, classes=C, n_reqs=len(t["reqs"]), n_terms=len(t["terms"]), mask_pool_words=len(t["mask_pool"]),
             tol_pool_words=len(t["tol_pool"]))
    guard = kr.GUARD_BYTES // 8
    planes = np.zeros((2 * C + 2) * W + guard, dtype="<u8")
    mask = np.zeros(C * W + guard, dtype="<u8")
    rc = probe.kbg_tool_probe_stage_mask(params(STAGE_FIELDS, p), ptr(t["label_bits"]), ptr(t["taint_bits"]),
                                         ptr(t["num_vals"]), ptr(t["num_ok"]), ptr(t["name_id"]), ptr(t["node_flags"]),
                                         ptr(t["mask_pool"]), ptr(t["tol_pool"]), ptr(t["reqs"]), ptr(t["terms"]),
                                         ptr(t["classes"]), ptr(planes), ptr(mask))
    check_rc(probe, rc)
    want = np.concatenate([sel.ravel(), tol.ravel(), uns, live])
    bad = np.flatnonzero(planes[:len(want)] != want)
    assert not len(bad), f"plane word {int(bad[0])}: {int(planes[bad[0]]):#x} != {int(want[bad[0]]):#x}"
    assert (planes[len(want):].view(np.uint8) == kr.SENTINEL).all(), "plane guard overwritten"
    # kbg_mask_kernel on the same tables: unchanged, and the identity holds on the device's own words
    assert (mask[:C * W] == cm.ravel()).all()
    assert (mask[C * W:].view(np.uint8) == kr.SENTINEL).all(), "mask guard overwritten"
    g_sel, g_tol = planes[:C * W].reshape(C, W), planes[C * W:2 * C * W].reshape(C, W)
    g_uns, g_live = planes[2 * C * W:2 * C * W + W], planes[2 * C * W + W:2 * C * W + 2 * W]
    for c, cp in enumerate(t["classes"]):
        if not cp["always"]:
            assert (mask[c * W:(c + 1) * W] == g_sel[c] & g_tol[c] & ~g_uns & g_live).all()


def run_reasons(probe, c, **override):
    p = dict(c["p"], **override)
    out = np.zeros(p["nq"] * rr.REASON_OUT + kr.GUARD_BYTES // 4, dtype="<i4")
    rc = probe.kbg_tool_probe_reasons(params(FIT_FIELDS, p), c["block"], ptr(c["planes"]), ptr(c["hoff"]),
                                      ptr(c["hk"]), ptr(c["q"]), ptr(out))
    return rc, out


@pytest.mark.parametrize("name", sorted(rr.REASON_CASES))
def test_reasons(probe, name):
    c = rr.reasons_case(**rr.REASON_CASES[name])
    ref = rr.reasons_reference(c)
    rc, out = run_reasons(probe, c)
    check_rc(probe, rc)
    nq = c["p"]["nq"]
    n = nq * rr.REASON_OUT
    assert out[:n].reshape(nq, rr.REASON_OUT).tolist() == ref[:n].reshape(nq, rr.REASON_OUT).tolist()
    assert (out[n:] == ref[n:]).all(), "guard overwritten"


@pytest.mark.parametrize("override,what", [(dict(tab_n=10 ** 6), "window"), (dict(classes=0), "empty"),
                                           (dict(n_dec=3), "hoff")])
def test_reasons_probe_rejects_illegal_launches(probe, override, what):
    """Nothing the session would never produce reaches the device: the probe
    answers -2 and leaves the output alone."""
    c = rr.reasons_case(**rr.REASON_CASES["n65-q2-cap1"])
    rc, out = run_reasons(probe, c, **override)
    assert rc == -2 and what in probe.kbg_tool_probe_error().decode()
    assert not out.any()
    q = c["q"].copy()
    q["end"][1] = c["p"]["n_nodes"] + 1
    rc, out = run_reasons(probe, dict(c, q=q))
    assert rc == -2 and not out.any()
