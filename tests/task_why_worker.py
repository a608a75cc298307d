"""A child process of tests/test_hostsim_task_why.py: the only kbg library it
loads is kube-arbitrator_amd/tools/libkbg_hostsim.so (KBG_LIB_PATH), under
the schedule its parent put in KBG_HOSTSIM_SCHEDULE.

    python tests/task_why_worker.py kernels OUT.json
    python tests/task_why_worker.py sessions OUT.json

kernels: every case of tests/task_why_cases.py through hostsim's
kbg_tool_probe_task_why, compared with tests/task_why_ref.py, and the launches
the probe must refuse. sessions: every case of SESSION_CASES through
tests/task_why_session.py. OUT.json maps a case id to its differences
(sessions: and the causes its expected rows held, and whether it was skipped)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")

# seeds of each generator, picked with the oracle alone: every action prefix
# of task_why_session.PREFIXES ends ok, Pending tasks are left, several cycles
# evict; one seed (affinity 509) discards a statement after evicting, which is
# within the quarter of a generator's seeds that may go without expected rows
SEEDS = {"random": (1, 2, 5, 7, 8, 15), "contended": (6, 7, 15, 18, 19, 21), "ports": (0, 1, 3, 6, 7, 9, 13, 19),
         "affinity": (500, 503, 505, 506, 509, 515, 522, 523)}
KATS = ("kat_task_why", "kat_reclaim", "kat_preempt")
SESSION_CASES = (["kat_task_why-hand", "kat_task_why_host-hand", "refusals", "resident"] + list(KATS) +
                 [f"{kind}{s}" for kind, seeds in SEEDS.items() for s in seeds])


def kind_of(case):
    return next((k for k in SEEDS if case.startswith(k)), None)


def session_fixture(case):
    import task_why_session as ts
    if case.startswith("kat_"):
        with open(os.path.join(HERE, "golden", case + ".json")) as f:
            return json.load(f)
    kind = kind_of(case)
    return ts.seeded_fixture(kind, int(case[len(kind):]))


def run_session_case(case, opts=None):
    """(errors, seen, skipped) of one session case on whatever library KBG_LIB_PATH names."""
    import task_why_session as ts
    from kbgpu import synth
    if case.endswith("-hand"):
        return ts.check_kat(session_fixture(case[:-5])), None, False
    if case == "refusals":
        return ts.check_refusals(session_fixture("kat_task_why")), None, False
    if case == "resident":
        fx = dict(synth.contended_fixture(7), actions=["reclaim", "allocate", "backfill", "preempt"])
        return ts.check_resident(fx, seed=7, rounds=2, opts=opts), None, False
    return ts.check_fixture(session_fixture(case), opts)


def kernels(out_path):
    import task_why_cases as tc
    from test_kernels_gpu import params, ptr
    L = ctypes.CDLL(LIB)
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    res = {}
    for name in tc.NAMES:
        res["case/" + name] = tc.check_probe(L, tc.case(name), ptr, params)
    for ident, *_ in tc.illegal_launches():
        res["reject/" + ident] = tc.check_illegal(L, ptr, params, ident)
    with open(out_path, "w") as f:
        json.dump(res, f)


def sessions(out_path):
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    res = {}
    for case in SESSION_CASES:
        try:
            errs, seen, skipped = run_session_case(case)
        except Exception as e:  # the case fails in the parent; the others still run
            errs, seen, skipped = [f"{type(e).__name__}: {e}"], None, False
        res[case] = {"errors": errs, "seen": seen, "skipped": skipped}
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    (kernels if sys.argv[1] == "kernels" else sessions)(sys.argv[2])
