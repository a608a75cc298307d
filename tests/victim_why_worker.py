"""A child process of tests/test_hostsim_victim_why.py: the only kbg library it
loads is kube-arbitrator_amd/tools/libkbg_hostsim.so (KBG_LIB_PATH), under
the schedule its parent put in KBG_HOSTSIM_SCHEDULE.

    python tests/victim_why_worker.py kernels OUT.json
    python tests/victim_why_worker.py sessions OUT.json

kernels: every case of tests/victim_why_cases.py through hostsim's
kbg_tool_probe_victim_why, compared with tests/victim_why_ref.py, and the
launches the probe must refuse. sessions: every case of SESSION_CASES through
tests/victim_why_session.py. OUT.json maps a case id to its list of
differences (sessions: and the causes its reference rows held)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")

# contended_fixture seeds (tests/test_parity_gpu.py's generators) whose oracle
# cycle ends ok without a discarded statement, found with the oracle alone
# (victim_why_session.discard_free); the sizes are those of
# test_contended_reclaim_preempt_parity and test_contended_large_parity
CONTENDED = (1, 4, 7, 19, 23)
CONTENDED_LARGE = (0, 7)
# seeds whose oracle cycle does discard a statement after evicting: no oracle tables, the device-shaped path
# against host_why on the same session (victim_why_session.check_discard)
DISCARD = (12, 14, 17, 28)
DISCARD_LARGE = (3,)
SESSION_CASES = (["kat_victim_why", "kat_victim_why-hand", "kat_reclaim", "kat_preempt", "kat_reclaim-twin",
                  "kat_preempt-twin", "huge", "huge-twin", "refusals", "resident"] +
                 [f"contended{s}" for s in CONTENDED] + [f"contended{s}-twin" for s in CONTENDED[:2]] +
                 [f"contended-large{s}" for s in CONTENDED_LARGE] +
                 [f"discard{s}" for s in DISCARD] + [f"discard-large{s}" for s in DISCARD_LARGE])


def session_fixture(case):
    import victim_why_session as ws
    from kbgpu import synth
    name, twin = (case[:-5], True) if case.endswith("-twin") else (case, False)
    if name.startswith("kat_"):
        with open(os.path.join(HERE, "golden", name + ".json")) as f:
            fx = json.load(f)
    elif name == "huge":
        fx = ws.huge_fixture()
    elif name.startswith("contended-large") or name.startswith("discard-large"):
        fx = synth.contended_fixture(5000 + int(name.rsplit("large", 1)[1]), nodes=40, jobs=30, tasks=10, queues=3)
    elif name.startswith("discard"):
        fx = synth.contended_fixture(int(name[7:]))
    else:
        fx = synth.contended_fixture(int(name[9:]))
    return ws.port_twin(fx) if twin else fx


def run_session_case(case):
    """(errors, seen) of one session case on whatever library KBG_LIB_PATH names."""
    import victim_why_session as ws
    if case == "kat_victim_why-hand":
        return ws.check_kat(session_fixture("kat_victim_why")), None
    if case.startswith("discard"):
        return ws.check_discard(session_fixture(case))
    if case == "refusals":
        return ws.check_refusals(session_fixture("kat_reclaim")), None
    if case == "resident":
        fx = dict(session_fixture("contended4"), actions=["reclaim", "allocate", "backfill", "preempt"])
        return ws.check_resident(fx, seed=4, rounds=2), None
    return ws.check_fixture(session_fixture(case))


def illegal_launches():
    """(id, p_over, mutate, what the message names) of launches kbg_victim_reasons never makes."""
    def q(field, value):
        def m(a):
            a["queries"][1][field] = value
        return m

    def nt_off(a):
        a["nt_off"][3] = a["nt_off"][2] - 1

    return [("node_lo", dict(node_lo=32), None, "node_lo"), ("range", dict(node_n=0), None, "node range"),
            ("n_nodes", dict(n_nodes=10 ** 6), None, "n_nodes"), ("n_rows", dict(n_rows=99), None, "n_rows"),
            ("nq0", dict(nq=0), None, "nq"), ("nt_off", None, nt_off, "nt_off"),
            ("q-cls", None, q("cls", 3), "cls"), ("q-mode", None, q("mode", 3), "mode"),
            ("q-tiers", None, q("n_tiers", 9), "n_tiers"), ("q-fns", None, q("tier_fns", 8), "tier_fns"),
            ("q-job", None, q("job", 10), "job or queue"), ("q-geometry", None, q("node_n", 5), "geometry")]


def check_illegal(lib, ptr, params, ident):
    import numpy as np

    import victim_why_cases as wc
    from kernel_ref import SENTINEL
    _, over, mutate, what = next(x for x in illegal_launches() if x[0] == ident)
    c = wc.case("n65-q17-cap1")
    rc, a, raw = wc.run_probe(lib, c, ptr, params, over, mutate)
    msg = lib.kbg_tool_probe_error().decode()
    errs = []
    if rc != -2 or what not in msg:
        errs.append(f"expected -2 naming {what}: got {rc} {msg!r}")
    if not (raw == SENTINEL).all():
        errs.append("a rejected launch wrote its output")
    if not (a["c_run"] == np.ascontiguousarray(c.c_run)).all():
        errs.append("a rejected launch wrote a table")
    return errs


def kernels(out_path):
    import victim_why_cases as wc
    from test_kernels_gpu import params, ptr
    L = ctypes.CDLL(LIB)
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    res = {}
    for name in wc.NAMES:
        res["case/" + name] = wc.check_probe(L, wc.case(name), ptr, params)[1]
    for ident, *_ in illegal_launches():
        res["reject/" + ident] = check_illegal(L, ptr, params, ident)
    with open(out_path, "w") as f:
        json.dump(res, f)


def sessions(out_path):
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    res = {}
    for case in SESSION_CASES:
        try:
            errs, seen = run_session_case(case)
        except Exception as e:  # the case fails in the parent; the others still run
            errs, seen = [f"{type(e).__name__}: {e}"], None
        res[case] = {"errors": errs, "seen": seen}
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    (kernels if sys.argv[1] == "kernels" else sessions)(sys.argv[2])
