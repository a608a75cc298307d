"""A child process of the hostsim tests (tests/test_hostsim_kernels.py,
tests/test_hostsim_parity.py): the only kbg library it loads is
kube-arbitrator_amd/tools/libkbg_hostsim.so — the unchanged session code on a
simulated HIP stream with host launchers — under the schedule its parent put
in KBG_HOSTSIM_SCHEDULE (the simulator reads it once per process).

    python tests/hostsim_worker.py kernels OUT.json
    python tests/hostsim_worker.py parity CASES.json OUT.json
    python tests/hostsim_worker.py snapshots CASES.json DIR

kernels: every seeded case of tests/kernel_cases.py and tests/victim_ref.py
(both output modes, and the launches the victim probe must refuse) through
the probes (tools/kernel_probe.cpp compiled against the simulator), compared
here with tests/kernel_ref.py's and tests/victim_ref.py's comparators;
OUT.json maps a case id to its list of differences. parity: every case of
CASES.json (test_hostsim_parity.py's specs, reclaim / preempt sessions
included) through the product path (kbgpu.fixture.run_fixture with
KBG_LIB_PATH pointing at the library); OUT.json maps a case id to the outputs
in the oracle's schema, which the parent compares with the oracle's, the
session's victim counters of kbg_stats and the launches hostsim counted per
victim launcher during the case. snapshots: the kbg_snapshot of every case
saved as DIR/<id>.kbgs (kbg_snapshot_save) with DIR/manifest.json naming each
one's actions (any of reclaim, allocate, backfill, preempt), for
tools/hostsim_main (tests/test_hostsim_sanitizers.py).
"""
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

LIB = os.path.join(ROOT, "kube-arbitrator_amd", "tools", "libkbg_hostsim.so")


# ------------------------------------------------------------------ kernels
def kernels(out_path):
    import numpy as np

    import kernel_cases as kc
    import kernel_ref as kr
    from test_kernels_gpu import FIT_FIELDS, SCAN_FIELDS, params, ptr, run_apply_case, run_firstfit

    L = ctypes.CDLL(LIB)
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    for f in ("firstfit", "scan_select", "fitdelta", "apply"):
        getattr(L, "kbg_tool_probe_" + f).restype = ctypes.c_int32
    assert L.kbg_tool_probe_guard_bytes() == kr.GUARD_BYTES and L.kbg_tool_probe_sentinel() == kr.SENTINEL
    res = {}

    def rc_errs(rc):
        return [] if rc == 0 else [f"probe returned {rc}: {L.kbg_tool_probe_error().decode()}"]

    for name in kc.FF_NAMES:
        case = kc.ff_case(name)
        exp = kr.ff_reference(case)
        rc, info, masks = run_firstfit(L, case, exp)
        res["firstfit/" + name] = rc_errs(rc) or kr.ff_compare(case, exp, info, masks)

    case = kc.ff_case("words130-ee1-int")
    exp = kr.ff_reference(case)
    for override, what in [(dict(rows=0), "rows"), (dict(rows=17), "rows"), (dict(complete=1), "complete"),
                           (dict(w_hi=10 ** 6), "w_lo"), (dict(tab_n=10 ** 6), "window"), (dict(mw=3), "mw"),
                           (dict(split_words=1), "splits")]:
        rc, info, masks = run_firstfit(L, case, exp, **override)
        msg = L.kbg_tool_probe_error().decode()
        errs = []
        if rc != -2 or what not in msg:
            errs.append(f"expected -2 naming {what}: got {rc} {msg!r}")
        if info.any() or masks.any():
            errs.append("a rejected launch wrote its buffers")
        res["reject/" + "-".join(f"{k}{v}" for k, v in override.items())] = errs

    for name in sorted(kc.SCAN_CASES):
        for int_mode in (True, False):
            c = kc.scan_case(name, int_mode)
            bits = np.zeros_like(c["bits"])
            cand_ref, count_ref = kr.select_reference(c["F"], c["FI"], c["p"]["w_lo"], c["p"]["w_hi"], c["cap_off"])
            cand, count = np.zeros_like(cand_ref), np.zeros_like(count_ref)
            rc = L.kbg_tool_probe_scan_select(params(SCAN_FIELDS, c["p"]), c["tab"].block(), ptr(c["tab"].class_mask),
                                              ptr(c["recs"]), ptr(c["cap_off"]), ptr(bits), ptr(cand), ptr(count))
            errs = rc_errs(rc)
            if not errs:
                for what, got, want in (("bitmap word", bits, c["bits"]), ("count of row", count, count_ref),
                                        ("candidate slot", cand, cand_ref)):
                    bad = np.flatnonzero(got != want)
                    if len(bad):
                        i = int(bad[0])
                        errs.append(f"{what} {i}: {int(got[i]):#x} != {int(want[i]):#x} ({len(bad)} differ)")
            res[f"scan_select/{name}-{'int' if int_mode else 'gen'}"] = errs

    for name in sorted(kc.FIT_CASES):
        c = kc.fit_case(name)
        ref = kr.fitdelta_reference(c["tab"], c["hoff"], c["hk"], c["hold"], c["q"], c["p"]["cap_check"])
        out = np.zeros_like(ref)
        rc = L.kbg_tool_probe_fitdelta(params(FIT_FIELDS, c["p"]), c["tab"].block(), ptr(c["tab"].class_mask),
                                       ptr(c["hoff"]), ptr(c["hk"]), ptr(c["hold"]), ptr(c["na"]), ptr(c["q"]),
                                       ptr(out))
        errs = rc_errs(rc)
        bad = np.flatnonzero(out != ref)
        if not errs and len(bad):
            i = int(bad[0])
            errs.append(f"word {i} (query {i // 4}, guard from {4 * c['p']['nq']}): {int(out[i])} != {int(ref[i])}")
        res["fitdelta/" + name] = errs

    # the second tier (kbg_options.reasons): the bodies of tests/test_reasons_kernels_gpu.py on this library
    import reasons_kernel_ref as rr
    import test_reasons_kernels_gpu as trk
    L.kbg_tool_probe_stage_mask.restype = ctypes.c_int32
    L.kbg_tool_probe_reasons.restype = ctypes.c_int32

    def failures(test, *args):
        try:
            test(L, *args)
        except AssertionError as e:
            return [str(e) or "assertion failed"]
        except Exception as e:  # (check_rc ends a pytest run on a probe's HIP error: here it is the case's failure)
            return [f"{type(e).__name__}: {e}"]
        return []

    for n in rr.NODE_COUNTS:
        res[f"stage_mask/n{n}"] = failures(trk.test_stage_mask, n)
    for name in sorted(rr.REASON_CASES):
        res["reasons/" + name] = failures(trk.test_reasons, name)

    # the victim launchers (prep, scan, big-node launch) in both output modes, and the launches the
    # probe must refuse: the bodies of tests/test_victim_kernels_gpu.py on this library
    import test_victim_kernels_gpu as tvk
    import victim_ref as vr
    for name in vr.NAMES:
        for out_mode, mode in enumerate(("mapped", "device")):
            res[f"victim/{name}-{mode}"] = failures(tvk.test_victim_scan, name, out_mode)
    for i, (over, mutate, null, what) in enumerate(tvk.ILLEGAL):
        res[f"victim_reject/{i:02d}-{what.replace(' ', '_')}"] = \
            failures(tvk.test_victim_probe_rejects_illegal_launches, over, mutate, null, what)

    a = run_apply_case(L)  # the case of test_kernels_gpu.py's `applied` fixture
    n = len(a["want"])
    res["apply"] = [] if (a["table"] == a["want"]).all() else ["the table differs after launch_apply"]
    res["mask_apply"] = [] if (a["mask"] == a["want_mask"]).all() else ["the mask differs after launch_mask_apply"]
    res["copy16"] = ([] if (a["copy"][:n] == a["want"]).all() else ["launch_copy16's copy differs"]) + \
                    ([] if (a["copy"][n:] == kr.SENTINEL).all() else ["launch_copy16 wrote past the copy"])
    with open(out_path, "w") as f:
        json.dump(res, f)


# ------------------------------------------------------------------- parity
def staged_rows_fixture(nodes=24, same=20, other=4):
    """A hand-built reclaim session whose staged prep matters to the next scan.
    Every node (4 CPUs, 3 pods at most) runs two 2000m tasks of queue q1. Queue
    q2 holds `same` Pending one-task jobs of one shape (2000m): the first is
    scanned, the others are answered from the kept stop maps (gang decides, so
    the maps survive), each evicting one task of the next node and pipelining
    onto it — which brings that node to its pod cap. Then `other` jobs of
    another shape (1000m) force a new scan: victim_push now holds `same`
    touched rows, more than the inline arguments take, and with a small
    batch_tasks it stages them in several chunks. A chunk whose staging is
    rewritten before its launch read it leaves earlier rows below their cap
    on the device, the scan stops at node 0 again, and the eviction log
    differs from the oracle's."""
    nds = [{"name": f"n{i:02d}", "allocatable": {"cpu": "4", "memory": "16Gi", "pods": "3"}, "labels": {}}
           for i in range(nodes)]
    pods, pgs = [], []

    def job(name, queue, ts, n_tasks, cpu, placed):
        pgs.append({"namespace": "ns", "name": name, "minMember": 1, "queue": queue,
                    "creationTimestamp": ts * 1_000_000_000})
        for t in range(n_tasks):
            node = placed[t] if placed else ""
            pods.append({"uid": f"{name}-{t:02d}", "namespace": "ns", "name": f"{name}-{t:02d}",
                         "phase": "Running" if placed else "Pending", "nodeName": node,
                         "annotations": {"scheduling.k8s.io/group-name": name},
                         "containers": [{"requests": {"cpu": f"{cpu}m", "memory": "1Gi"}}]})

    for j in range(0, nodes, 4):  # a running job holds both slots of four nodes
        job(f"run{j:02d}", "q1", 0, 8, 2000, [nds[j + k // 2]["name"] for k in range(8)])
    for j in range(same):
        job(f"same{j:02d}", "q2", 100 + j, 1, 2000, None)
    for j in range(other):
        job(f"other{j:02d}", "q2", 500 + j, 1, 1000, None)
    return {"name": "staged-rows", "tiers": None, "nodes": nds, "pods": pods, "podGroups": pgs,
            "queues": [{"name": "q1", "weight": 1}, {"name": "q2", "weight": 1}], "actions": ["reclaim"]}


def make_fixture(c):
    """The fixture of a case spec (test_hostsim_parity.py CASES); the parent
    builds the same one for the oracle."""
    from kbgpu import synth
    g, a, kw = c["gen"], c.get("arg"), c.get("kw", {})
    if g == "golden":
        with open(os.path.join(HERE, "golden", a)) as f:
            fx = json.load(f)
    elif g == "config":
        fx = synth.config_fixture(a)
    elif g == "random":
        fx = synth.random_fixture(a, **kw)
    elif g == "affinity":
        fx = synth.affinity_fixture(a)
    elif g == "dupkey":
        fx = synth.dupkey_fixture(a)
    elif g == "contended":
        fx = synth.contended_fixture(a, **kw)
    elif g == "contended_dupkey":
        fx = synth.contended_dupkey_fixture(a, **kw)
    elif g == "contended_config":
        fx = synth.contended_config(**kw)
    elif g == "staged_rows":
        fx = staged_rows_fixture(**kw)
    elif g == "saturated":
        fx = synth.saturated_config(**kw)
    elif g == "deep":
        from test_kernels_gpu import deep_fixture
        fx = deep_fixture(a, **kw)
    else:
        raise ValueError(g)
    if c.get("no_nodes"):
        fx["nodes"] = []
    if c.get("heap_rule"):
        fx["options"] = {"heapDownRule": "go1.13"}
    if "actions" in c:
        fx["actions"] = c["actions"]
    if c.get("only_allocate_backfill"):  # (the cases from before the victim launchers were simulated)
        fx["actions"] = [a for a in (fx.get("actions") or ["allocate"]) if a in ("allocate", "backfill")] or ["allocate"]
    return fx


def victim_stats(ssn):
    st = ssn.stats()
    return {k: int(getattr(st, k)) for k in ("victim_scans", "victim_tries", "victim_host_evals")}


def run_chain(c, stats):
    """A resident session over churn rounds (helpers.churn_chain): each
    snapshot opened fresh, and the session opened at S_0 and updated round by
    round (kbg_session_update) must make the fresh open's cycle. Returns the
    fresh outputs per round; `stats` receives the resident session's
    victim_stats after each round, summed."""
    from helpers import churn_chain
    from kbgpu import _abi
    from kbgpu.fixture import run_fixture
    from test_update_gpu import _open, _same_cycle, abi_cycle
    fx0 = make_fixture(c)
    actions = fx0.get("actions") or ["allocate"]
    state, outs = {}, []

    def run(fx, changes):
        fresh, fssn = run_fixture(fx, c.get("opts"))
        if fssn:
            fssn.close()
        if not changes:
            state["ssn"] = _open(fx, c.get("opts"))
            got = abi_cycle(state["ssn"], actions)
        else:
            _abi.check(_abi.lib().kbg_session_reset(state["ssn"].handle))
            try:
                state["ssn"].update(changes)
                got = abi_cycle(state["ssn"], actions)
            except _abi.KbgError as e:
                assert e.status == "ref_panic", e
                got = {"status": "ref_panic"}
        for k, v in victim_stats(state["ssn"]).items():
            stats[k] = stats.get(k, 0) + v
        _same_cycle(got, fresh)
        return fresh

    try:
        for r, changes, fx, out in churn_chain(fx0, c["seed"], c["rounds"], run):
            outs.append(out)
    finally:
        if "ssn" in state:
            state["ssn"].close()
    return outs


class _Env:
    """monkeypatch's setenv / delenv, for test bodies run outside pytest."""

    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k, raising=True):
        os.environ.pop(k, None)


def run_reasons(c):
    """A session opened with kbg_options.reasons (the second tier:
    launch_build_stage_planes, launch_reasons): the bodies of
    tests/test_reasons_gpu.py — the simulated device path against the host
    path byte for byte, the oracle's decisions, the accounting identity and
    tests/reasons_ref.py — raise on the first difference."""
    import test_reasons_gpu as trg
    if c["kind"] == "hand":
        trg.test_hand_written_case(c["arg"], _Env)
    else:
        trg.test_seeded_session(c["kind"], c["arg"], _Env)


def parity(cases_path, out_path):
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    from kbgpu import _abi
    from kbgpu.fixture import run_fixture
    with open(cases_path) as f:
        cases = json.load(f)
    # hostsim's launch counters of the victim launchers (tools/hostsim_kernels.cpp), per case
    H = ctypes.CDLL(LIB)
    H.kbg_hostsim_launch_count_names.restype = ctypes.c_char_p
    names = H.kbg_hostsim_launch_count_names().decode().split(",")
    counts = (ctypes.c_int64 * len(names))()
    res = {}
    for c in cases:
        t0 = time.time()
        if c.get("general"):
            os.environ["KBG_FORCE_GENERAL_SCAN"] = "1"
        else:
            os.environ.pop("KBG_FORCE_GENERAL_SCAN", None)
        H.kbg_hostsim_launch_counts_reset()
        try:
            if c["gen"] == "chain":
                stats = {}
                rec = {"chain": run_chain(dict(c, gen=c["base"]), stats), "stats": stats}
            elif c["gen"] == "reasons":
                run_reasons(c)
                rec = {}
            else:
                got, ssn = run_fixture(make_fixture(c), c.get("opts"))
                rec = {"out": got}
                if ssn:
                    rec["int_scan"] = ssn.stats().int_scan
                    rec["stats"] = victim_stats(ssn)
                    ssn.close()
        except Exception as e:  # the case fails in the parent; the other cases still run
            # (a wrong decision can also end the host replay: kbgpu.api.RefPanic on a full node)
            rec = {"error": f"{type(e).__name__}: {e}"}
        assert H.kbg_hostsim_launch_counts(counts, len(names)) == len(names)
        rec["launches"] = {k: int(v) for k, v in zip(names, counts) if v}
        rec["s"] = round(time.time() - t0, 3)
        res[c["id"]] = rec
    with open(out_path, "w") as f:
        json.dump(res, f)


def snapshots(cases_path, out_dir):
    from kbgpu import _abi
    from kbgpu.cache import FakeBinder, cache_from_fixture
    from kbgpu.fixture import _OrderedCache, fixture_tiers
    from kbgpu.snapshot import FlatSnapshot
    with open(cases_path) as f:
        cases = json.load(f)
    manifest = []
    for c in cases:
        fx = make_fixture(c)
        snap = _OrderedCache(cache_from_fixture(fx, FakeBinder()), fx).snapshot()
        flat = FlatSnapshot(snap.nodes, snap.jobs, snap.queues, snap.others, fixture_tiers(fx))
        path = os.path.join(out_dir, c["id"] + ".kbgs")
        _abi.check(_abi.lib().kbg_snapshot_save(ctypes.byref(flat.snap), path.encode()))
        manifest.append({"id": c["id"], "path": path, "actions": fx.get("actions") or ["allocate"]})
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f)


def revival(cases_path, out_path):
    """Queue and job names that return to a resident session
    (tests/revival_session.py, the bodies tests/test_revival_gpu.py runs on
    the device): every comparison runs here and raises on the first
    difference; the parent reads each case's record."""
    assert os.environ.get("KBG_LIB_PATH") == LIB, "the parent sets KBG_LIB_PATH to the hostsim library"
    import revival_session
    with open(cases_path) as f:
        cases = json.load(f)
    res = {}
    for c in cases:
        t0 = time.time()
        rec = {}
        try:
            if c["kind"] == "case":
                want = revival_session.run_case(c["arg"], c.get("opts"))
            elif c["kind"] == "seed":
                want = revival_session.run_seed(c["arg"], c.get("opts"))
            else:
                want = revival_session.SPECIALS[c["arg"]]() or []
            rec["refused"] = [v.round for v in want if v is not None]
        except BaseException as e:  # (pytest.raises fails with an exception outside Exception)
            if isinstance(e, (KeyboardInterrupt, SystemExit)):
                raise
            import traceback
            rec = {"error": f"{type(e).__name__}: {e}\n{traceback.format_exc(limit=6)}"}
        rec["s"] = round(time.time() - t0, 3)
        res[c["id"]] = rec
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    if sys.argv[1] == "kernels":
        kernels(sys.argv[2])
    elif sys.argv[1] == "parity":
        parity(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "revival":
        revival(sys.argv[2], sys.argv[3])
    else:
        snapshots(sys.argv[2], sys.argv[3])
