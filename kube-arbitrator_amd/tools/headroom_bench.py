"""Developer tool: what kbg_task_headroom costs on BASELINE C3 (5k nodes x 100k
tasks, synth.config_fixture(3)). One resident session opened with reasons runs
allocate for `cycles` + 1 cycles (kbg_session_reset between them; the first
cycle warms up and is dropped), all in one process. Before each allocate (the
snapshot: every task still Pending) and after it, it asks for the rows of
every task that was Pending at open (the placed ones come back with valid ==
0) at limit 128 and at limit 1024, once on the device-shaped path and once
with KBG_HOST_TASK_HEADROOM=1, and once for kbg_task_reasons, the figure to
set the kernel's time beside. With KBG_PROFILE_TASK_HEADROOM (and
KBG_PROFILE_TASK_WHY) the library prints the distinct keys of a call and the
HIP-event time of its kernel launches (the events bracket the kernel alone).

Prints one JSON line: the tasks asked, the rows still Pending, the distinct
keys, and medians (and ranges) over the timed cycles of the kernel time, of
the call's wall time and of the host path's wall time. No threshold is set.
python kube-arbitrator_amd/tools/headroom_bench.py [cycles] [config]"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
LIMITS = (128, 1024)


def child(cycles, config):
    import ctypes
    from kbgpu import _abi, synth
    from kbgpu.api import PENDING
    from kbgpu.cache import FakeBinder, cache_from_fixture
    from kbgpu.fixture import _OrderedCache, fixture_tiers
    from kbgpu.framework import open_session
    fx = synth.config_fixture(config)
    ssn = open_session(_OrderedCache(cache_from_fixture(fx, FakeBinder()), fx), fixture_tiers(fx), {"device": 0},
                       reasons=True)
    L = _abi.lib()
    cap = len(ssn.flat.task_objs) + 1
    buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
    tasks = [t for t, obj in enumerate(ssn.flat.task_objs) if obj is not None and obj.status == PENDING]
    arr = (ctypes.c_int32 * max(1, len(tasks)))(*tasks)
    rows = (_abi.kbg_task_room * max(1, len(tasks)))()
    why = (_abi.kbg_task_why * max(1, len(tasks)))()
    out = []
    for cyc in range(cycles + 1):
        rec = {}
        for when in ("open", "allocated"):  # the snapshot (every task Pending), then what allocate left
            if when == "allocated":
                _abi.check(L.kbg_allocate(ssn.handle, buf, cap, ctypes.byref(n)))
                rec["decisions"] = n.value
            sys.stderr.write(f"[bench] cycle {cyc} {when}_why\n")
            sys.stderr.flush()
            _abi.check(L.kbg_task_reasons(ssn.handle, arr, len(tasks), why))
            for limit in LIMITS:
                for kind in ("device", "host"):
                    if kind == "host":
                        os.environ["KBG_HOST_TASK_HEADROOM"] = "1"
                    key = f"{when}_{limit}_{kind}"
                    sys.stderr.write(f"[bench] cycle {cyc} {key}\n")
                    sys.stderr.flush()
                    t0 = time.perf_counter()  # the C call alone (Session.task_headroom adds a dict per row)
                    _abi.check(L.kbg_task_headroom(ssn.handle, arr, len(tasks), limit, rows))
                    rec[f"{key}_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    os.environ.pop("KBG_HOST_TASK_HEADROOM", None)
                    rec[f"{key}_rows"] = sum(r.valid for r in rows)
                    rec[f"{key}_digest"] = hash(bytes(rows))
                    if kind == "device":
                        rec[f"{when}_{limit}_copies"] = [max((r.copies_idle for r in rows if r.valid), default=0),
                                                         max((r.max_node_copies for r in rows if r.valid), default=0),
                                                         sum(1 for r in rows if r.valid and r.limit_hit)]
                rec[f"{when}_{limit}_paths_equal"] = rec.pop(f"{when}_{limit}_device_digest") == \
                    rec.pop(f"{when}_{limit}_host_digest")
        out.append(rec)
        _abi.check(L.kbg_session_reset(ssn.handle))
    ssn.close()
    print(json.dumps({"nodes": len(fx["nodes"]), "tasks_asked": len(tasks), "cycles": out}), flush=True)


def spread(v):
    v = [x for x in v if x is not None]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} if v else None


def main():
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    config = sys.argv[2] if len(sys.argv) > 2 else "3"
    env = dict(os.environ, KBG_PROFILE_TASK_HEADROOM="1", KBG_PROFILE_TASK_WHY="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(cycles), config], env=env,
                       capture_output=True, text=True, check=True)
    data = json.loads(p.stdout.strip().splitlines()[-1])
    kern, mark = {}, None  # the library's line after each of the child's markers
    for line in p.stderr.splitlines():
        m = re.match(r"\[bench\] cycle (\d+) (\w+)", line)
        if m:
            mark = (int(m.group(1)), m.group(2))
            continue
        m = re.match(r"\[kbg task (?:why|headroom)\] \d+ tasks, (\d+) keys, .*kernel ([\d.]+) ms", line)
        if m and mark:
            kern[mark] = (int(m.group(1)), float(m.group(2)) * 1e3)
            mark = None
    timed = data["cycles"][1:]
    res = {"config": int(config), "nodes": data["nodes"], "tasks_asked": data["tasks_asked"], "timed_cycles": len(timed)}
    for when in ("open", "allocated"):
        ws = [k for k in (kern.get((c, f"{when}_why")) for c in range(1, cycles + 1)) if k]
        res[when] = {"why_kernel_us": spread([k[1] for k in ws])}
        for limit in LIMITS:
            ks = [k for k in (kern.get((c, f"{when}_{limit}_device")) for c in range(1, cycles + 1)) if k]
            res[when][f"limit_{limit}"] = {
                "pending_rows": timed[0][f"{when}_{limit}_device_rows"] if timed else None,
                "keys": ks[0][0] if ks else 0,
                "max_copies_idle, max_node_copies, rows_with_limit_hit": timed[0][f"{when}_{limit}_copies"] if timed else None,
                "paths_equal": all(c[f"{when}_{limit}_paths_equal"] for c in data["cycles"]),
                "headroom_kernel_us": spread([k[1] for k in ks]),
                "call_wall_ms": spread([c[f"{when}_{limit}_device_wall_ms"] for c in timed]),
                "host_path_wall_ms": spread([c[f"{when}_{limit}_host_wall_ms"] for c in timed])}
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
