"""A child process of tests/test_hostsim_query_update.py: the only kbg library
it loads is kube-arbitrator_amd/tools/libkbg_hostsim.so (KBG_LIB_PATH), under
the schedule its parent put in KBG_HOSTSIM_SCHEDULE.

    python tests/query_update_worker.py OUT.json

Every case of tests/query_update_cases.py through
tests/query_update_session.py's check_rounds, with hostsim's launch counters
(tools/hostsim_kernels.cpp) read around the updated session's own calls.
OUT.json maps a case id to its record: the differences, the rows compared
with the fresh session and with the references, whether an update was
refused, and the counters."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")
KEEP = ("errors", "rows", "rows_ref", "skipped", "rebuilds", "by_uid_only", "n_classes", "answered", "launches",
        "stage_mask", "host_only", "evicted0", "ref", "rows_ref_by", "round_launches", "drain_plain_walk",
        "pod_affinity", "first_asked")


def run_case(case, opts=None, probe=None):
    """The record of one case on whatever library KBG_LIB_PATH names."""
    import query_update_cases as qc
    import query_update_session as qs
    cases = qc.all_cases()
    fx0, rounds_of, flags = cases[case][1]()
    # the ordinal of the case's first asked point: its place in its family, so that the cases of a family start the
    # rotation of the seven calls at different calls
    first = [c for c, (fam, _) in cases.items() if fam == cases[case][0]].index(case)
    res = qs.check_rounds(fx0, rounds_of, opts, probe=probe, first_point=first, **flags)
    return {k: res.get(k) for k in KEEP}


def run_entry(case, opts=None):
    """check_queries_after_update's differences for a case of one update."""
    import query_update_cases as qc
    import query_update_session as qs
    fx0, (changes_of,), flags = qc.all_cases()[case][1]()
    assert not flags
    return qs.check_queries_after_update(fx0, lambda s: changes_of(s, fx0), opts)


def main(out_path):
    import query_update_cases as qc
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    H = ctypes.CDLL(LIB)
    H.kbg_hostsim_launch_count_names.restype = ctypes.c_char_p
    names = H.kbg_hostsim_launch_count_names().decode().split(",")
    counts = (ctypes.c_int64 * len(names))()

    def probe():
        assert H.kbg_hostsim_launch_counts(counts, len(names)) == len(names)
        return dict(zip(names, counts))

    out = {}
    for case in qc.all_cases():
        try:
            out[case] = run_case(case, probe=probe)
        except Exception as e:  # the case fails in the parent; the others still run
            out[case] = {"errors": [f"{type(e).__name__}: {e}"], "rows": 0, "rows_ref": 0, "skipped": None}
    try:  # the issue's entry point, on one case
        out["entry/relabel_hand"] = run_entry("recompile/relabel_hand")
    except Exception as e:
        out["entry/relabel_hand"] = [f"{type(e).__name__}: {e}"]
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1])
