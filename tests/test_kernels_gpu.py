"""Kernel-level differential tests: each HIP kernel of the allocate path is
launched alone on flat arrays through the probes of the tool library
(kube-arbitrator_amd/tools/kernel_probe.cpp) and its raw device output is
compared, bit for bit, with the plain reference of tests/kernel_ref.py — the
covered mask words, the info words, and the sentinel in every byte the kernel
must not touch (guard regions included). The seeded cases are those of
tests/kernel_cases.py; tests/test_kernel_ref.py shows on the CPU that each
case holds what it claims and that the comparator rejects a subtly wrong
output. Every launch is a legal one: the probes reject anything else on the
host."""
import ctypes
import functools

import numpy as np
import pytest

import kernel_cases as kc
import kernel_ref as kr
from helpers import build_tools, compare_outputs, run_oracle

pytestmark = pytest.mark.gpu

kbgpu = pytest.importorskip("kbgpu")
from kbgpu import _abi  # noqa: E402
from kbgpu.fixture import run_fixture  # noqa: E402

FF_FIELDS = ("G", "n_shapes", "mw", "n_nodes", "W", "w_lo", "w_hi", "tab_lo", "tab_n", "cap_check", "early_exit",
             "complete", "splits", "split_words", "rows", "info_stride", "part0", "mask_w0", "runs", "stride",
             "classes", "int_mode")
SCAN_FIELDS = ("n_nodes", "W", "Wl", "slots", "tab_lo", "stride", "classes", "n_tasks", "cap_check", "int_mode",
               "w_lo", "w_hi")
FIT_FIELDS = ("n_nodes", "W", "stride", "classes", "tab_lo", "tab_n", "nq", "cap_check", "n_dec")


def params(fields, p):
    return (ctypes.c_int32 * len(fields))(*[int(p[f]) for f in fields])


def ptr(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def probe():
    L = ctypes.CDLL(build_tools())
    if _abi.lib().kbg_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback)")
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    for f in ("firstfit", "scan_select", "fitdelta", "apply"):
        getattr(L, "kbg_tool_probe_" + f).restype = ctypes.c_int32
    assert L.kbg_tool_probe_guard_bytes() == kr.GUARD_BYTES and L.kbg_tool_probe_sentinel() == kr.SENTINEL
    return L


def check_rc(probe, rc):
    """A HIP error ends the run: nothing more is launched on a device that
    reported one."""
    if rc == -3:
        pytest.exit(f"HIP error in a kernel probe: {probe.kbg_tool_probe_error()}", returncode=3)
    assert rc == 0, (rc, probe.kbg_tool_probe_error())


def run_firstfit(probe, case, exp, **override):
    p = dict(case.p, **override)
    info = np.zeros_like(exp.info)
    masks = np.zeros_like(exp.masks)
    table = case.tab.block()
    shapes = case.shapes()
    rc = probe.kbg_tool_probe_firstfit(params(FF_FIELDS, p), table, ptr(case.tab.class_mask), ptr(shapes),
                                       ptr(case.row_shape), ptr(case.run_end), ptr(info), ptr(masks))
    return rc, info, masks


@pytest.mark.parametrize("name", kc.FF_NAMES)
def test_firstfit(probe, name):
    case = kc.ff_case(name)
    exp = kr.ff_reference(case)
    rc, info, masks = run_firstfit(probe, case, exp)
    check_rc(probe, rc)
    errs = kr.ff_compare(case, exp, info, masks)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("override,what", [
    (dict(rows=0), "rows"), (dict(rows=17), "rows"), (dict(complete=1), "complete"), (dict(w_hi=10 ** 6), "w_lo"),
    (dict(tab_n=10 ** 6), "window"), (dict(mw=3), "mw"), (dict(split_words=1), "splits"),
])
def test_firstfit_probe_rejects_illegal_launches(probe, override, what):
    """Nothing launch_firstfit or device_launch would never produce reaches
    the device: the probe answers -2 and leaves the buffers alone."""
    case = kc.ff_case("words130-ee1-int")
    exp = kr.ff_reference(case)
    rc, info, masks = run_firstfit(probe, case, exp, **override)
    assert rc == -2 and what in probe.kbg_tool_probe_error().decode()
    assert not info.any() and not masks.any()


@pytest.mark.parametrize("int_mode", [True, False], ids=["int", "gen"])
@pytest.mark.parametrize("name", sorted(kc.SCAN_CASES))
def test_scan_select(probe, name, int_mode):
    c = kc.scan_case(name, int_mode)
    bits = np.zeros_like(c["bits"])
    cand_ref, count_ref = kr.select_reference(c["F"], c["FI"], c["p"]["w_lo"], c["p"]["w_hi"], c["cap_off"])
    cand, count = np.zeros_like(cand_ref), np.zeros_like(count_ref)
    rc = probe.kbg_tool_probe_scan_select(params(SCAN_FIELDS, c["p"]), c["tab"].block(), ptr(c["tab"].class_mask),
                                          ptr(c["recs"]), ptr(c["cap_off"]), ptr(bits), ptr(cand), ptr(count))
    check_rc(probe, rc)
    bad = np.flatnonzero(bits != c["bits"])
    assert not len(bad), f"bitmap word {int(bad[0])}: {int(bits[bad[0]]):#x} != {int(c['bits'][bad[0]]):#x}"
    bad = np.flatnonzero(count != count_ref)
    assert not len(bad), f"row {int(bad[0])}: count {int(count[bad[0]]):#x} != {int(count_ref[bad[0]]):#x}"
    bad = np.flatnonzero(cand != cand_ref)
    assert not len(bad), f"candidate slot {int(bad[0])}: {int(cand[bad[0]]):#x} != {int(cand_ref[bad[0]]):#x}"
    # Releasing-only candidates are among them
    n = int(c["cap_off"][-1])
    assert (cand_ref[:n][cand_ref[:n] != np.uint32(0xA5A5A5A5)] & np.uint32(kr.CAND_PIPELINE_BIT)).any()


@pytest.mark.parametrize("name", sorted(kc.FIT_CASES))
def test_fitdelta(probe, name):
    c = kc.fit_case(name)
    ref = kr.fitdelta_reference(c["tab"], c["hoff"], c["hk"], c["hold"], c["q"], c["p"]["cap_check"])
    out = np.zeros_like(ref)
    rc = probe.kbg_tool_probe_fitdelta(params(FIT_FIELDS, c["p"]), c["tab"].block(), ptr(c["tab"].class_mask),
                                       ptr(c["hoff"]), ptr(c["hk"]), ptr(c["hold"]), ptr(c["na"]), ptr(c["q"]),
                                       ptr(out))
    check_rc(probe, rc)
    nq = c["p"]["nq"]
    assert out[:4 * nq].reshape(nq, 4).tolist() == ref[:4 * nq].reshape(nq, 4).tolist()
    assert (out[4 * nq:] == ref[4 * nq:]).all(), "guard overwritten"


def run_apply_case(probe):
    """One run of the apply probe: the table after kbg_apply_kernel, the mask
    after kbg_mask_apply_kernel, kbg_copy16_kernel's copy, and numpy's."""
    rng = np.random.default_rng(9001)
    stride, words = 1500, 77
    f = rng.random((6, stride)) * 1e6
    f[:, ::7] = np.nextafter(f[:, ::7], np.inf)
    i = rng.integers(0, 1 << 30, size=(2, stride)).astype(np.int32)
    mask = rng.integers(0, 1 << 63, size=words, dtype=np.uint64)
    nd = np.zeros(300, dtype=kr.NODE_DELTA)  # distinct nodes, first, last and a 256-thread block boundary among them
    nd["node"] = np.concatenate([[0, stride - 1, 255, 256],
                                 rng.permutation(np.setdiff1d(np.arange(stride), [0, stride - 1, 255, 256]))[:296]])
    nd["ntasks"] = rng.integers(0, 100, size=300)
    nd["maxtasks"] = rng.integers(0, 100, size=300)
    nd["idle"] = rng.random((300, 3)) * 1e9
    nd["rel"] = -rng.random((300, 3))
    md = np.zeros(40, dtype=kr.MASK_DELTA)
    md["index"] = np.concatenate([[0, words - 1], rng.permutation(np.arange(1, words - 1))[:38]])
    md["value"] = rng.integers(0, 1 << 63, size=40, dtype=np.uint64)
    ef, ei, em = f.copy(), i.copy(), mask.copy()
    ef[0:3, nd["node"]] = nd["idle"].T
    ef[3:6, nd["node"]] = nd["rel"].T
    ei[0, nd["node"]] = nd["ntasks"]
    ei[1, nd["node"]] = nd["maxtasks"]
    em[md["index"]] = md["value"]
    table = np.frombuffer(f.tobytes() + i.tobytes(), dtype=np.uint8).copy()
    copy = np.zeros(len(table) + kr.GUARD_BYTES, dtype=np.uint8)
    got_mask = mask.copy()
    rc = probe.kbg_tool_probe_apply(stride, ptr(table), ptr(nd), len(nd), ptr(got_mask), words, ptr(md), len(md),
                                    ptr(copy))
    check_rc(probe, rc)
    want = np.frombuffer(ef.tobytes() + ei.tobytes(), dtype=np.uint8)
    return dict(table=table, want=want, mask=got_mask, want_mask=em, copy=copy)


@pytest.fixture(scope="module")
def applied(probe):
    return run_apply_case(probe)


def test_apply(applied):
    assert (applied["table"] == applied["want"]).all()


def test_mask_apply(applied):
    assert (applied["mask"] == applied["want_mask"]).all()


def test_copy16(applied):
    n = len(applied["want"])
    assert (applied["copy"][:n] == applied["want"]).all()
    assert (applied["copy"][n:] == kr.SENTINEL).all(), "guard overwritten"


# ------------------------------------------------ the consumer of cut lists
# Sessions whose walk is more than one round (8193 nodes are 129 words), so
# that the host consumes cut and split lists (kbg_session.cpp device_wait):
# most of the first nodes are too small for any task, the fits start deep in
# the table and a shape's list is cut long before the table ends.
def deep_fixture(n_nodes, releasing=False):
    import random
    rng = random.Random(n_nodes)
    nodes, pods, pgs = [], [], []
    for i in range(n_nodes):
        small = i < n_nodes * 6 // 10 and i % 97 != 0
        cpu, mem = ("250m", "256Mi") if small else (rng.choice(["1", "2", "4"]), rng.choice(["2Gi", "4Gi", "8Gi"]))
        nodes.append({"name": f"node-{i:05d}", "labels": {"zone": f"z{i % 4}"},
                      "allocatable": {"cpu": cpu, "memory": mem, "nvidia.com/gpu": "0", "pods": "110"}})
        if releasing and not small and i % 5 == 0:  # a pod being deleted: its request is the node's Releasing
            pods.append({"uid": f"run-{i:05d}", "namespace": "ns0", "name": f"run-{i:05d}", "phase": "Running",
                         "nodeName": nodes[-1]["name"], "deletionTimestamp": "2026-01-01T00:00:00Z",
                         "containers": [{"requests": {"cpu": "500m", "memory": "1Gi"}}]})
    for j in range(40):
        pg = f"pg-{j:03d}"
        req = {"cpu": rng.choice(["500m", "1", "2"]), "memory": rng.choice(["1Gi", "2Gi", "4Gi"])}
        spec = {"nodeSelector": {"zone": f"z{rng.randrange(4)}"}} if rng.random() < 0.3 else {}
        pgs.append({"namespace": "ns0", "name": pg, "minMember": rng.choice([1, 8]), "queue": ("q1", "q2")[j % 2],
                    "creationTimestamp": (1_700_000_000 + j) * 1_000_000_000})
        for t in range(8):
            pods.append(dict({"uid": f"uid-{j:03d}-{t}", "namespace": "ns0", "name": f"{pg}-{t}", "phase": "Pending",
                              "annotations": {"scheduling.k8s.io/group-name": pg},
                              "containers": [{"requests": dict(req)}]}, **spec))
    return {"name": f"deep{n_nodes}", "tiers": None, "nodes": nodes, "pods": pods, "podGroups": pgs,
            "queues": [{"name": "q1", "weight": 1}, {"name": "q2", "weight": 2}]}


DEEP = {"8193": (8193, False), "8300": (8300, False), "16500": (16500, False), "8300-releasing": (8300, True)}


@functools.lru_cache(maxsize=None)
def deep_oracle(key):
    fx = deep_fixture(*DEEP[key])
    return fx, run_oracle(fx)


@pytest.mark.parametrize("general", [0, 1], ids=["int", "gen"])
@pytest.mark.parametrize("full_scan", [0, 1])
@pytest.mark.parametrize("key", sorted(DEEP))
def test_session_consumes_cut_and_split_lists(key, full_scan, general, monkeypatch):
    if general:
        monkeypatch.setenv("KBG_FORCE_GENERAL_SCAN", "1")
    fx, ref = deep_oracle(key)
    assert ref["status"] == "ok" and len(ref["decisions"]) > 250
    got, ssn = run_fixture(fx, {"full_scan": full_scan})
    assert ssn.stats().int_scan == 1 - general
    compare_outputs(ref, got)
    ssn.close()
