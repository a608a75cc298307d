"""Developer tool: what kbg_node_reasons costs on BASELINE C3 (5k nodes x 100k
tasks, synth.config_fixture(3)). One resident session opened with reasons runs
allocate for `cycles` + 1 cycles (kbg_session_reset between them; the first
cycle warms up and is dropped). Before each allocate (the snapshot: every
task still Pending) and after it, it asks for the rows of every node on the
device-shaped path and with KBG_HOST_NODE_WHY=1, then for 1 and for 16 named
nodes (16 nodes of 16 different words), and, as the yardstick, for
kbg_task_reasons of every task that was Pending at open: the same (node,
shape) pairs reduced the other way. With KBG_PROFILE_NODE_WHY and
KBG_PROFILE_TASK_WHY the library prints the distinct keys of a call and the
HIP-event time of its kernel launches (the events bracket the kernel alone).

Prints one JSON line: the nodes, the Pending tasks, the distinct keys and the
words of each call, and medians (and ranges) over the timed cycles of the
kernel times and of the calls' wall times. No threshold is set.
python kube-arbitrator_amd/tools/node_why_bench.py [cycles] [config]"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

CALLS = ("all_device", "all_host", "named1", "named16", "task_why")


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
    N = len(ssn.flat.node_names)
    tasks = [t for t, obj in enumerate(ssn.flat.task_objs) if obj is not None and obj.status == PENDING]
    tarr = (ctypes.c_int32 * max(1, len(tasks)))(*tasks)
    trows = (_abi.kbg_task_why * max(1, len(tasks)))()
    rows = (_abi.kbg_node_why * N)()
    step = max(64, N // 16 // 64 * 64)
    named = {"named1": [N // 2], "named16": [min(N - 1, 7 + k * step) for k in range(16)]}
    out = []
    for cyc in range(cycles + 1):
        rec = {}
        for when in ("open", "allocated"):  # the snapshot (every task Pending), then what allocate left
            if when == "allocated":
                _abi.check(L.kbg_allocate(ssn.handle, buf, cap, ctypes.byref(n)))
                rec["decisions"] = n.value
            for call in CALLS:
                if call == "all_host":
                    os.environ["KBG_HOST_NODE_WHY"] = "1"
                sys.stderr.write(f"[bench] cycle {cyc} {when}_{call}\n")
                sys.stderr.flush()
                if call == "task_why":
                    t0 = time.perf_counter()
                    _abi.check(L.kbg_task_reasons(ssn.handle, tarr, len(tasks), trows))
                    rec[f"{when}_{call}_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    continue
                pick = named.get(call)
                arr = (ctypes.c_int32 * len(pick))(*pick) if pick else None
                res = (_abi.kbg_node_why * len(pick))() if pick else rows
                t0 = time.perf_counter()  # the C call alone (Session.node_reasons adds a dict per row)
                _abi.check(L.kbg_node_reasons(ssn.handle, arr, len(pick) if pick else N, res))
                rec[f"{when}_{call}_wall_ms"] = (time.perf_counter() - t0) * 1e3
                os.environ.pop("KBG_HOST_NODE_WHY", None)
                if pick is None:
                    rec[f"{when}_{call}_digest"] = hash(bytes(res))
                    rec[f"{when}_pending"] = res[0].pending
                    if call == "all_device":
                        whole = bytes(res)
                else:
                    size = ctypes.sizeof(_abi.kbg_node_why)
                    rec[f"{when}_{call}_equal"] = all(bytes(res)[k * size:(k + 1) * size] == whole[i * size:(i + 1) * size]
                                                      for k, i in enumerate(pick))
            rec[f"{when}_paths_equal"] = rec.pop(f"{when}_all_device_digest") == rec.pop(f"{when}_all_host_digest")
        out.append(rec)
        _abi.check(L.kbg_session_reset(ssn.handle))
    ssn.close()
    print(json.dumps({"nodes": N, "tasks_asked": len(tasks), "cycles": out}), flush=True)


def spread(v):
    v = [x for x in v if x is not None]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} if v else None


def main():
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    config = sys.argv[2] if len(sys.argv) > 2 else "3"
    env = dict(os.environ, KBG_PROFILE_NODE_WHY="1", KBG_PROFILE_TASK_WHY="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(cycles), config], env=env,
                       capture_output=True, text=True, check=True)
    data = json.loads(p.stdout.strip().splitlines()[-1])
    kern, mark = {}, None  # the library's line after each of the child's markers: (keys, words, kernel us)
    for line in p.stderr.splitlines():
        m = re.match(r"\[bench\] cycle (\d+) (\w+)", line)
        if m:
            mark = (int(m.group(1)), m.group(2))
            continue
        m = re.match(r"\[kbg node why\] \d+ tasks, (\d+) keys, (\d+) words, why kernel ([\d.]+) ms", line)
        if m and mark:
            kern[mark] = (int(m.group(1)), int(m.group(2)), float(m.group(3)) * 1e3)
            mark = None
            continue
        m = re.match(r"\[kbg task why\] \d+ tasks, (\d+) keys, why kernel ([\d.]+) ms", line)
        if m and mark:
            kern[mark] = (int(m.group(1)), None, float(m.group(2)) * 1e3)
            mark = None
    timed = data["cycles"][1:]
    res = {"config": int(config), "nodes": data["nodes"], "tasks_asked": data["tasks_asked"], "timed_cycles": len(timed)}
    for when in ("open", "allocated"):
        rec = {"pending": timed[0][f"{when}_pending"] if timed else None,
               "paths_equal": all(c[f"{when}_paths_equal"] for c in data["cycles"]),
               "named_equal": all(c[f"{when}_{k}_equal"] for c in data["cycles"] for k in ("named1", "named16"))}
        for call in CALLS:
            ks = [kern.get((c, f"{when}_{call}")) for c in range(1, cycles + 1)]
            ks = [k for k in ks if k]
            rec[call] = {"keys": ks[0][0] if ks else None, "words": ks[0][1] if ks else None,
                         "kernel_us": spread([k[2] for k in ks]),
                         "call_wall_ms": spread([c[f"{when}_{call}_wall_ms"] for c in timed])}
        res[when] = rec
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
