"""A child process of tests/test_hostsim_drain.py: the only kbg library it
loads is kube-arbitrator_amd/tools/libkbg_hostsim.so (KBG_LIB_PATH), under
the schedule its parent put in KBG_HOSTSIM_SCHEDULE.

    python tests/drain_worker.py kernels OUT.json
    python tests/drain_worker.py sessions OUT.json

kernels: every case of tests/drain_cases.py through hostsim's
kbg_tool_probe_drain, compared with tests/drain_ref.py, and the launches the
probe must refuse. sessions: every case of SESSION_CASES through
tests/drain_session.py, then every case of ALLOCATE_CASES against the oracle's
own allocate. OUT.json maps a case id to its differences (sessions:
and what the expected rows show, whether it was skipped, and hostsim's `drain`
launch count)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")

from job_fit_worker import KATS, SEEDS, kind_of, session_fixture  # noqa: E402  (the seed lists of the issue)

ALLOCATE_CASES = ["allocate-hand", "allocate-dev"] + [f"allocate-{kind}{s}" for kind, seeds in
                                                       __import__("drain_session").ALLOCATE_SEEDS.items() for s in seeds]
AFTER_CASES = [c.replace("allocate-", "allocate-after-") for c in ALLOCATE_CASES[2:]]
SESSION_CASES = (["kat_drain-hand", "dup-hand", "drain-hand", "drain-dev", "headroom", "refusals", "resident", "structural", "twin-random",
                  "twin-contended", "twin-affinity", "oracle-twin-contended", "oracle-twin-ports",
                  "oracle-twin-affinity"] + list(KATS) + [f"{kind}{s}" for kind, seeds in SEEDS.items() for s in seeds])


def run_session_case(case, opts=None):
    """(errors, seen, skipped) of one session case on whatever library KBG_LIB_PATH names."""
    import drain_session as ds
    if case == "kat_drain-hand":
        return ds.check_kat(session_fixture("kat_drain")), None, False
    if case == "dup-hand":
        return ds.check_dup(), None, False
    if case in ("drain-hand", "drain-dev"):
        return ds.check_hand(case == "drain-hand"), None, False
    if case == "headroom":
        return ds.check_headroom(), None, False
    if case == "refusals":
        return ds.check_refusals(ds.drain_fixture(ports=False)), None, False
    if case.startswith("oracle-twin-"):
        kind = case[len("oracle-twin-"):]
        errs, said = [], 0
        for s in SEEDS[kind]:
            e, n = ds.check_twin_oracle(session_fixture(f"{kind}{s}"))
            errs += e
            said += n
        return errs + ([] if said >= 4 else [f"{said} walks compared"]), None, False
    if case.startswith("twin-"):
        kind = case[5:]
        errs, said = [], 0
        for s in SEEDS[kind]:
            e, n = ds.check_twin(session_fixture(f"{kind}{s}"), opts)
            errs += e
            said += n
        return errs + ([] if said else ["no walk compared"]), None, False
    if case == "resident":  # the chain of tests/headroom_worker.py's resident case
        from kbgpu import synth
        fx = dict(synth.contended_fixture(7), actions=["reclaim", "allocate", "backfill", "preempt"])
        errs, said = ds.check_resident(fx, seed=7, rounds=2, opts=opts)
        return errs + ([] if said else ["no row compared"]), None, False
    if case == "structural":
        errs, said = ds.check_structural()
        return errs + ([] if said else ["no row compared"]), None, False
    return ds.check_fixture(session_fixture(case), opts)


def run_allocate_case(case):
    """(errors, walks compared, walks left out or None for a fixture left out) of drain_session.check_allocate."""
    import drain_session as ds
    if case.startswith("allocate-after-"):
        return ds.check_allocate_after(session_fixture(case[len("allocate-after-"):]))
    name = case[len("allocate-"):]
    fx = ds.drain_fixture(ports=name == "hand") if name in ("hand", "dev") else session_fixture(name)
    return ds.check_allocate(fx)


def kernels(out_path):
    import drain_cases as dc
    from test_kernels_gpu import params, ptr
    L = ctypes.CDLL(LIB)
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    res = {}
    for name in dc.NAMES:
        res["case/" + name] = dc.check_probe(L, dc.case(name), ptr, params)
    for ident, *_ in dc.illegal_launches():
        res["reject/" + ident] = dc.check_illegal(L, ptr, params, ident)
    with open(out_path, "w") as f:
        json.dump(res, f)


def sessions(out_path):
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    H = ctypes.CDLL(LIB)
    H.kbg_hostsim_launch_count_names.restype = ctypes.c_char_p
    names = H.kbg_hostsim_launch_count_names().decode().split(",")
    counts = (ctypes.c_int64 * len(names))()
    res = {"names": names}

    def counted(fn):
        H.kbg_hostsim_launch_counts_reset()
        try:
            rec = fn()
        except Exception as e:  # the case fails in the parent; the others still run
            import traceback
            rec = {"errors": [f"{type(e).__name__}: {e}", traceback.format_exc()], "seen": None, "skipped": False}
        assert H.kbg_hostsim_launch_counts(counts, len(names)) == len(names)
        rec["launches"] = dict(zip(names, counts)).get("drain")
        return rec

    for case in SESSION_CASES:
        res[case] = counted(lambda: dict(zip(("errors", "seen", "skipped"), run_session_case(case))))
    # the oracle's own allocate of the moved pods: what is left out is decided here, on the CPU
    for case in ALLOCATE_CASES + AFTER_CASES:
        res[case] = counted(lambda: dict(zip(("errors", "compared", "left"), run_allocate_case(case))))
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    (kernels if sys.argv[1] == "kernels" else sessions)(sys.argv[2])
