"""A child process of tests/test_hostsim_node_why.py: the only kbg library it
loads is kube-arbitrator_amd/tools/libkbg_hostsim.so (KBG_LIB_PATH), under
the schedule its parent put in KBG_HOSTSIM_SCHEDULE.

    python tests/node_why_worker.py kernels OUT.json
    python tests/node_why_worker.py sessions OUT.json

kernels: every case of tests/node_why_cases.py through hostsim's
kbg_tool_probe_node_why, compared with tests/node_why_ref.py, and the launches
the probe must refuse. sessions: every case of SESSION_CASES through
tests/node_why_session.py, then hostsim's launch counter around calls that
must and must not reach the launcher. OUT.json maps a case id to its
differences (sessions: and the causes its expected rows held, whether it was
skipped and whether an overused queue showed in a row)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")

# seeds of tests/task_why_worker.py's lists (picked there with the oracle alone: every action prefix ends ok,
# Pending tasks are left), three a generator; affinity509 discards a statement after evicting
SEEDS = {"random": (1, 5, 8), "contended": (6, 7, 19), "ports": (0, 1, 13), "affinity": (500, 506, 509)}
KATS = ("kat_task_why", "kat_reclaim", "kat_preempt")
# (recompile/relabel_hand: kbg_node_reasons is the only call asked, so the first to need the stage planes after a
# NODE_SET recompile; tests/query_update_session.py asks it among the other six)
RESIDENT = ("structural/w_grows", "in_place/regrow_keys", "recompile/relabel_hand")
SESSION_CASES = (["kat_node_why-hand", "refusals"] + ["resident:" + c for c in RESIDENT] + list(KATS) +
                 [f"{kind}{s}" for kind, seeds in SEEDS.items() for s in seeds])


def session_fixture(case):
    import task_why_worker as tw
    return tw.session_fixture(case)


def run_session_case(case, opts=None):
    """(errors, seen, skipped, differs) of one session case on whatever library KBG_LIB_PATH names."""
    import node_why_session as ns
    if case.endswith("-hand"):
        return ns.check_kat(session_fixture(case[:-5])), None, False, False
    if case == "refusals":
        return ns.check_refusals(session_fixture("kat_task_why")), None, False, False
    if case.startswith("resident:"):
        return ns.check_resident(case[len("resident:"):], opts), None, False, False
    return ns.check_fixture(session_fixture(case), opts)


def kernels(out_path):
    import node_why_cases as nc
    from test_kernels_gpu import params, ptr
    L = ctypes.CDLL(LIB)
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    res = {}
    for name in nc.NAMES:
        res["case/" + name] = nc.check_probe(L, nc.case(name), ptr, params)
    for ident, *_ in nc.illegal_launches():
        res["reject/" + ident] = nc.check_illegal(L, ptr, params, ident)
    with open(out_path, "w") as f:
        json.dump(res, f)


def launches():
    """{what: launches of the node_why counter}: a session the device path
    answers (all nodes, one node, KBG_HOST_NODE_WHY=1) and the host-only KAT."""
    import node_why_session as ns
    import victim_why_session as ws
    H = ctypes.CDLL(LIB)
    H.kbg_hostsim_launch_count_names.restype = ctypes.c_char_p
    names = H.kbg_hostsim_launch_count_names().decode().split(",")

    def count():
        counts = (ctypes.c_int64 * len(names))()
        assert H.kbg_hostsim_launch_counts(counts, len(names)) == len(names)
        return counts[names.index("node_why")]

    out = {}
    for what, fixture, ask in (("device, all nodes", "kat_task_why", lambda s: s.node_reasons()),
                               ("device, one node", "kat_task_why", lambda s: s.node_reasons([3])),
                               ("forced host", "kat_task_why", lambda s: ns.host_rows(s)),
                               ("host only", "kat_node_why", lambda s: s.node_reasons())):
        ssn, _ = ws.open_with_reasons(session_fixture(fixture))
        try:
            c0 = count()
            rows = ask(ssn)
            out[what] = count() - c0 if rows and all(r["valid"] for r in rows) else -1
        finally:
            ssn.close()
    return out


def sessions(out_path):
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    res = {}
    for case in SESSION_CASES:
        try:
            errs, seen, skipped, differs = run_session_case(case)
        except Exception as e:  # the case fails in the parent; the others still run
            errs, seen, skipped, differs = [f"{type(e).__name__}: {e}"], None, False, False
        res[case] = {"errors": errs, "seen": seen, "skipped": skipped, "differs": differs}
    res["launches"] = launches()
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    (kernels if sys.argv[1] == "kernels" else sessions)(sys.argv[2])
