"""A child process of tests/test_hostsim_job_fit.py: the only kbg library it
loads is kube-arbitrator_amd/tools/libkbg_hostsim.so (KBG_LIB_PATH), under
the schedule its parent put in KBG_HOSTSIM_SCHEDULE.

    python tests/job_fit_worker.py kernels OUT.json
    python tests/job_fit_worker.py sessions OUT.json

kernels: every case of tests/job_fit_cases.py through hostsim's
kbg_tool_probe_job_fit, compared with tests/job_fit_ref.py, and the launches
the probe must refuse. sessions: every case of SESSION_CASES through
tests/job_fit_session.py. OUT.json maps a case id to its differences
(sessions: and what the expected rows show, whether it was skipped, and
hostsim's `job_fit` launch count)."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")

# seeds of tests/headroom_worker.py's lists (every action prefix ends ok, Pending tasks are left)
SEEDS = {"random": (1, 5, 7, 8), "contended": (6, 7, 19, 21), "ports": (0, 1, 13, 19),
         "affinity": (500, 503, 506, 509)}
KATS = ("kat_task_why", "kat_reclaim", "kat_preempt")
SESSION_CASES = (["kat_job_fit-hand", "gang-hand", "gang-dev", "refusals", "resident", "structural"] + list(KATS) +
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


def check_gang_hand(ports=True):
    """The hand-worked walks of job_fit_session.gang_fixture, at open, on both paths."""
    import job_fit_session as js
    import victim_why_session as ws
    ssn, _ = ws.open_with_reasons(js.gang_fixture(ports))
    claims = {k: v for k, v in js.GANG_CLAIMS.items() if ports or k != "ns/H"}
    errs = []
    try:
        names, tasks = ssn.flat.node_names, ssn.flat.task_objs
        for rows in (ssn.job_fit(), js.host_rows(ssn)):
            got = {ssn.jobs[r["job"]].uid: [(tasks[t].uid, names[n] if n >= 0 else None, k) for t, n, k in r["places"]]
                   for r in rows if r["valid"]}
            if got != claims:
                errs.append(f"walks {got}, hand-worked {claims}")
            by = {ssn.jobs[r["job"]].uid: r["ready_after"] for r in rows if r["valid"]}
            if by != {k: v for k, v in (("ns/G", 5), ("ns/N", -1), ("ns/H", 2)) if k in claims}:
                errs.append(f"ready_after {by}, hand-worked 5, -1, 2")
    finally:
        ssn.close()
    return errs


def run_session_case(case, opts=None):
    """(errors, seen, skipped) of one session case on whatever library KBG_LIB_PATH names."""
    import job_fit_session as js
    if case in ("gang-hand", "gang-dev"):
        return check_gang_hand(case == "gang-hand"), None, False
    if case.endswith("-hand"):
        return js.check_kat(session_fixture(case[:-5])), None, False
    if case == "refusals":
        return js.check_refusals(js.gang_fixture()), None, False
    if case == "resident":  # the chain of tests/headroom_worker.py's resident case
        from kbgpu import synth
        fx = dict(synth.contended_fixture(7), actions=["reclaim", "allocate", "backfill", "preempt"])
        errs, said = js.check_resident(fx, seed=7, rounds=2, opts=opts)
        return errs + ([] if said else ["no row compared"]), None, False
    if case == "structural":
        errs, said = js.check_structural()
        return errs + ([] if said else ["no row compared"]), None, False
    return js.check_fixture(session_fixture(case), opts)


def run_allocate(name, fx, picks):
    import job_fit_session as js
    errs, shown, snap = js.check_allocate(fx, picks)
    return {"errors": errs, "seen": sorted(js.features(shown, snap)), "jobs": len(shown)}


def kernels(out_path):
    import job_fit_cases as jc
    from test_kernels_gpu import params, ptr
    L = ctypes.CDLL(LIB)
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    res = {}
    for name in jc.NAMES:
        res["case/" + name] = jc.check_probe(L, jc.case(name), ptr, params)
    for ident, *_ in jc.illegal_launches():
        res["reject/" + ident] = jc.check_illegal(L, ptr, params, ident)
    with open(out_path, "w") as f:
        json.dump(res, f)


def sessions(out_path):
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    import job_fit_session as js
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
            rec = {"errors": [f"{type(e).__name__}: {e}"], "seen": None, "skipped": False}
        assert H.kbg_hostsim_launch_counts(counts, len(names)) == len(names)
        rec["launches"] = dict(zip(names, counts)).get("job_fit")
        return rec

    for case in SESSION_CASES:
        res[case] = counted(lambda: dict(zip(("errors", "seen", "skipped"), run_session_case(case))))
    # the oracle's own allocate: the fixtures left out are decided here, on the CPU
    for name, fx in js.allocate_fixtures().items():
        picks = js.allocate_picks(fx)
        if picks is None:
            res["allocate-" + name] = {"errors": [], "seen": [], "left_out": True, "launches": 0}
        else:
            res["allocate-" + name] = counted(lambda: run_allocate(name, fx, picks))
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    (kernels if sys.argv[1] == "kernels" else sessions)(sys.argv[2])
