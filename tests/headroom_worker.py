"""A child process of tests/test_hostsim_headroom.py: the only kbg library it
loads is kube-arbitrator_amd/tools/libkbg_hostsim.so (KBG_LIB_PATH), under
the schedule its parent put in KBG_HOSTSIM_SCHEDULE.

    python tests/headroom_worker.py kernels OUT.json
    python tests/headroom_worker.py sessions OUT.json

kernels: every case of tests/headroom_cases.py through hostsim's
kbg_tool_probe_task_headroom, compared with tests/headroom_ref.py, and the
launches the probe must refuse. sessions: every case of SESSION_CASES through
tests/headroom_session.py. OUT.json maps a case id to its differences
(sessions: and the largest expected values, and whether it was skipped)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")

# seeds of tests/task_why_worker.py's lists (picked there with the oracle:
# every action prefix ends ok, Pending tasks are left, several cycles evict);
# affinity 509 discards a statement after evicting, one of its generator's four
SEEDS = {"random": (1, 5, 7, 8), "contended": (6, 7, 19, 21), "ports": (0, 1, 13, 19),
         "affinity": (500, 503, 506, 509)}
KATS = ("kat_task_why", "kat_reclaim", "kat_preempt")
ALLOCATE = ("hand", "seed17", "seed70")
SESSION_CASES = (["kat_headroom-hand", "kat_headroom_dev-hand", "refusals", "resident"] + [f"allocate-{a}" for a in ALLOCATE] +
                 list(KATS) + [f"{kind}{s}" for kind, seeds in SEEDS.items() for s in seeds])


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
    import headroom_session as hs
    if case.startswith("allocate-"):
        return hs.check_allocate(hs.allocate_fixtures()[case[9:]]), None, False
    if case.endswith("-hand"):
        return hs.check_kat(session_fixture(case[:-5])), None, False
    if case == "refusals":
        return hs.check_refusals(session_fixture("kat_task_why")), None, False
    if case == "resident":  # the chain of tests/task_why_worker.py's resident case
        from kbgpu import synth
        fx = dict(synth.contended_fixture(7), actions=["reclaim", "allocate", "backfill", "preempt"])
        errs, said = hs.check_resident(fx, seed=7, rounds=2, opts=opts)
        print(f"resident: {said} rows compared with the fresh session's and the reference's")
        return errs + ([] if said else ["no row compared"]), None, False
    return hs.check_fixture(session_fixture(case), opts)


def kernels(out_path):
    import headroom_cases as hc
    from test_kernels_gpu import params, ptr
    L = ctypes.CDLL(LIB)
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    res = {}
    for name in hc.NAMES:
        res["case/" + name] = hc.check_probe(L, hc.case(name), ptr, params)
    for ident, *_ in hc.illegal_launches():
        res["reject/" + ident] = hc.check_illegal(L, ptr, params, ident)
    with open(out_path, "w") as f:
        json.dump(res, f)


def sessions(out_path):
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    # hostsim's launch counters (tools/hostsim_kernels.cpp), per case
    H = ctypes.CDLL(LIB)
    H.kbg_hostsim_launch_count_names.restype = ctypes.c_char_p
    names = H.kbg_hostsim_launch_count_names().decode().split(",")
    counts = (ctypes.c_int64 * len(names))()
    res = {}
    for case in SESSION_CASES:
        H.kbg_hostsim_launch_counts_reset()
        try:
            errs, seen, skipped = run_session_case(case)
        except Exception as e:  # the case fails in the parent; the others still run
            errs, seen, skipped = [f"{type(e).__name__}: {e}"], None, False
        assert H.kbg_hostsim_launch_counts(counts, len(names)) == len(names)
        res[case] = {"errors": errs, "seen": seen, "skipped": skipped,
                     "launches": dict(zip(names, counts)).get("task_headroom")}
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    (kernels if sys.argv[1] == "kernels" else sessions)(sys.argv[2])
