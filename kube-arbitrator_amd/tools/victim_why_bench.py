"""Developer tool: what kbg_victim_reasons costs on BASELINE C5 (10k nodes x
200k tasks, synth.contended_config), against kbg_victim_kernel in the same
process. One resident session opened with reasons runs the four actions for
`cycles` + 1 cycles (kbg_session_reset between them; the first cycle warms
up and is dropped). Per cycle:

  - the library times the cycle's first kbg_victim_kernel launch with HIP
    events around the kernel alone (try_task samples every 16th scan of a
    cycle and the counters start again with the cycle), so after reclaim
    victim_kernel_ms / victim_scans is that one sample: a reclaim-mode scan;
  - right after reclaim, kbg_victim_reasons in reclaim mode for one job (one
    key: the same mode, class, queue and request as that scan) and for every
    job, then in the two preempt modes, and again after preempt. With
    KBG_PROFILE_VICTIM the library prints the HIP-event time of its
    kbg_victim_why_kernel launches (the events bracket the kernel alone) and
    the distinct keys they answered.

Prints one JSON line: medians (and ranges) over the timed cycles of the
victim kernel's sample, of the why kernel's time per key for each kind of
call, and of the calls' wall time.
python kube-arbitrator_amd/tools/victim_why_bench.py [cycles] [generator overrides as k=v ...]"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

ENTRY = {"allocate": "kbg_allocate", "backfill": "kbg_backfill", "reclaim": "kbg_reclaim", "preempt": "kbg_preempt"}
MODES = {"reclaim": 2, "preempt_jobs": 0, "preempt_tasks": 1}


def child(cycles, over):
    import ctypes
    from kbgpu import _abi, synth
    from kbgpu.cache import FakeBinder, cache_from_fixture
    from kbgpu.fixture import _OrderedCache, fixture_tiers
    from kbgpu.framework import open_session
    fx = synth.contended_config(**over)
    ssn = open_session(_OrderedCache(cache_from_fixture(fx, FakeBinder()), fx), fixture_tiers(fx), {"device": 0},
                       reasons=True)
    L = _abi.lib()
    cap = len(ssn.flat.task_objs) + 1
    buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
    out = []
    for cyc in range(cycles + 1):
        rec = {"calls": []}
        for name in fx["actions"]:
            _abi.check(getattr(L, ENTRY[name])(ssn.handle, buf, cap, ctypes.byref(n)))
            if name not in ("reclaim", "preempt"):
                continue
            st = ssn.stats()
            if name == "reclaim":
                rec["victim_kernel_us"] = st.victim_kernel_ms / st.victim_scans * 1e3 if st.victim_scans else None
                rec["victim_scans_reclaim"] = st.victim_scans
            else:
                rec["victim_scans_cycle"] = st.victim_scans
            whole = ssn.victim_reasons(MODES["reclaim"])
            one = next((j for j, w in enumerate(whole) if w.valid), None)
            calls = [("reclaim_one_job", MODES["reclaim"], [one])] if one is not None else []
            calls += [(k, m, None) for k, m in MODES.items()]
            for kind, mode, jobs in calls:
                sys.stderr.write(f"[bench] cycle {cyc} after {name} {kind}\n")
                sys.stderr.flush()
                t0 = time.perf_counter()
                rows = ssn.victim_reasons(mode, jobs)
                rec["calls"].append({"after": name, "kind": kind, "wall_ms": (time.perf_counter() - t0) * 1e3,
                                     "rows": sum(r.valid for r in rows)})
        out.append(rec)
        _abi.check(L.kbg_session_reset(ssn.handle))
    ssn.close()
    print(json.dumps({"nodes": len(fx["nodes"]), "tasks": len(fx["pods"]), "cycles": out}), flush=True)


def spread(v):
    v = [x for x in v if x is not None]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} if v else None


def main():
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    over = sys.argv[2:]
    env = dict(os.environ, KBG_PROFILE_VICTIM="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(cycles), *over], env=env,
                       capture_output=True, text=True, check=True)
    data = json.loads(p.stdout.strip().splitlines()[-1])
    # the library's line after each of the child's markers
    kern, mark = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[bench\] cycle (\d+) after (\w+) (\w+)", line)
        if m:
            mark = (int(m.group(1)), m.group(2), m.group(3))
            continue
        m = re.match(r"\[kbg victim\] reasons mode \d+: \d+ jobs, (\d+) keys, why kernel ([\d.]+) ms", line)
        if m and mark:
            kern[mark] = (int(m.group(1)), float(m.group(2)) * 1e3)
            mark = None
    timed = data["cycles"][1:]
    res = {"nodes": data["nodes"], "tasks": data["tasks"], "timed_cycles": len(timed),
           "victim_kernel_us_per_launch": spread([c.get("victim_kernel_us") for c in timed]),
           "victim_kernel_us_first_cycle": data["cycles"][0].get("victim_kernel_us"),
           "victim_scans_per_cycle": timed[0].get("victim_scans_cycle") if timed else None, "calls": {}}
    for after in ("reclaim", "preempt"):
        for kind in ["reclaim_one_job"] + list(MODES):
            ks = [kern.get((c, after, kind)) for c in range(1, cycles + 1)]
            ks = [k for k in ks if k]
            walls = [x["wall_ms"] for c in timed for x in c["calls"] if x["after"] == after and x["kind"] == kind]
            if not ks:
                continue
            res["calls"][f"after_{after}/{kind}"] = {
                "keys": ks[0][0], "why_kernel_us": spread([k[1] for k in ks]),
                "why_kernel_us_per_key": spread([k[1] / k[0] for k in ks]), "wall_ms": spread(walls)}
    base = res["victim_kernel_us_per_launch"]
    one = res["calls"].get("after_reclaim/reclaim_one_job")
    if base and one:
        res["ratio_one_key_to_victim_scan"] = one["why_kernel_us_per_key"]["median"] / base["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        kv = {}
        for a in sys.argv[3:]:
            k, v = a.split("=")
            kv[k] = int(v)
        child(int(sys.argv[2]), kv)
    else:
        main()
