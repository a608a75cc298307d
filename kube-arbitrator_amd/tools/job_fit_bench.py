"""Developer tool: what kbg_job_fit costs on BASELINE C3 (5k nodes x 100k
tasks, synth.config_fixture(3)). One resident session opened with reasons runs
allocate for `cycles` + 1 cycles (kbg_session_reset between them; the first
cycle warms up and is dropped), all in one process. Before each allocate (the
snapshot: every task still Pending) and after it, it asks kbg_job_fit for
every job at limit 50 and at limit 512, once on the device-shaped path and once
with KBG_HOST_JOB_FIT=1, and kbg_task_headroom (limit 1024, both paths) for
every task that was Pending at open: the yardstick. With KBG_PROFILE_JOB_FIT
(and KBG_PROFILE_TASK_HEADROOM) the library prints the jobs, steps and shapes
of a call and the HIP-event time of its kernel launches.

The cursor (kbg_device.hpp JobFitArgs `prev`): after the last cycle's allocate
the tool rebuilds the call's launch for the probe (kbg_tool_probe_job_fit)
from the session's node states, the fixture's nodes and pods (the stage planes
per distinct pod spec through tests/reasons_ref.py) and the walks the call
reported, checks that the probe's places are the call's, and times the same
kernel with the links and with prev = -1 everywhere. A switch of this tool,
not of the product.

Prints one JSON line: medians (and ranges) over the timed cycles of the kernel
time, the call's wall time and the host path's wall time, whether both paths
returned the same bytes, and the cursor figures. No threshold is set.
python kube-arbitrator_amd/tools/job_fit_bench.py [cycles] [config]"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
LIMITS = (50, 512)


def mark(text):
    sys.stderr.write(f"[bench] {text}\n")
    sys.stderr.flush()


def cursor_figures(ssn, fx, rows, places):
    """The after-allocate launch at limit 512 through the probe, with and without the cursor links."""
    import ctypes
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import reasons_ref as rr
    # (KBG_TOOLS_PATH: another library holding the probe, such as the hostsim one for a CPU run of this tool)
    L = ctypes.CDLL(os.environ.get("KBG_TOOLS_PATH") or os.path.join(HERE, "libkbg_tools.so"))
    L.kbg_tool_probe_job_fit.restype = ctypes.c_int32
    L.kbg_tool_probe_job_fit_ms.restype = ctypes.c_double
    L.kbg_tool_probe_error.restype = ctypes.c_char_p
    N, W = len(ssn.nodes), (len(ssn.nodes) + 63) // 64
    st = [ssn.node_state(n) for n in range(N)]
    f = np.array([[getattr(getattr(s, which), d) for s in st] for which in ("idle", "releasing")
                  for d in ("milli_cpu", "memory", "milli_gpu")], dtype="<f8")
    i = np.array([[s.num_tasks for s in st], [n.allocatable.max_task_num for n in ssn.nodes]], dtype="<i4")
    block = np.frombuffer(f.tobytes() + i.tobytes(), dtype=np.uint8).copy()
    # classes: the distinct pod specs of the walked tasks; shapes: (class, request)
    tasks = ssn.flat.task_objs
    cls_of, shape_of, shapes, jobs = {}, {}, [], []
    for r in rows:
        if not r.valid:
            continue
        walk = []
        for p in places[r.place_off:r.place_off + r.walked]:
            t = tasks[p.task]
            spec = json.dumps({k: t.pod.get(k) for k in ("nodeSelector", "affinity", "tolerations")}, sort_keys=True)
            c = cls_of.setdefault(spec, (len(cls_of), t.pod))[0]
            req = tuple(float(v) for v in t.resreq.as_tuple())
            s = shape_of.setdefault((c, req), len(shape_of))
            if s == len(shapes):
                shapes.append((c, req))
            walk.append((s, p.node, p.kind))
        jobs.append(walk)
    K = len(cls_of)
    if not jobs:  # allocate left nothing Pending: nothing to time
        return {"jobs": 0}
    bits = np.ones((2 * K + 2, W * 64), dtype=bool)
    for c, pod in cls_of.values():
        bits[c, :N] = [rr.selector_ok(pod, n.node) for n in ssn.nodes]
        bits[K + c, :N] = [rr.taints_ok(pod, n.node) for n in ssn.nodes]
    bits[2 * K, :N] = [bool(n.node.get("unschedulable")) for n in ssn.nodes]
    bits[2 * K + 1, :N] = True
    planes = np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u8").reshape(-1)
    sh = np.zeros(len(shapes), dtype=[("cls", "<i4"), ("flags", "<i4"), ("req", "<f8", (3,))])
    for k, (c, req) in enumerate(shapes):
        sh[k] = (c, 0, req)
    n_steps = sum(len(w) for w in jobs)
    off = np.cumsum([0] + [len(w) for w in jobs]).astype("<i4")
    want = np.array([[n, k] for w in jobs for _, n, k in w], dtype="<i4").reshape(-1, 2)

    def steps(cursor):
        recs = np.zeros(n_steps, dtype=[("shape", "<i4"), ("prev", "<i4")])
        k = 0
        for w in jobs:
            last = {}
            for idx, (s, _, _) in enumerate(w):
                recs[k] = (s, last.get(s, -1) if cursor else -1)
                last[s] = idx
                k += 1
        return recs

    fields = [N, W, 0, N, N, K, len(shapes), 1, len(jobs), n_steps]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    res = {"jobs": len(jobs), "steps": n_steps, "shapes": len(shapes), "classes": K}
    for name, cursor in (("cursor", True), ("no_cursor", False)):
        ms, same = [], True
        recs = steps(cursor)
        for _ in range(4):
            raw = np.zeros(n_steps * 8 + 4096, dtype=np.uint8)
            blk = block.copy()
            mark(f"probe {name}")
            rc = L.kbg_tool_probe_job_fit((ctypes.c_int32 * len(fields))(*fields), ptr(blk), ptr(planes), ptr(sh),
                                          ptr(recs), ptr(off), ptr(raw))
            if rc != 0:
                raise RuntimeError(f"probe: {rc} {L.kbg_tool_probe_error()}")
            ms.append(L.kbg_tool_probe_job_fit_ms() * 1e3)
            got = np.frombuffer(raw[:n_steps * 8].tobytes(), dtype="<i4").reshape(-1, 2)
            same = same and bool((got == want).all())
        res[name] = {"kernel_us": ms[1:], "places_equal_the_call_s": same}  # (the first launch warms up)
    return res


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
    room = (_abi.kbg_task_room * max(1, len(tasks)))()
    nj = len(ssn.jobs)
    rows = (_abi.kbg_job_fit * max(1, nj))()
    places = (_abi.kbg_fit_place * cap)()
    need = ctypes.c_int32(0)
    out, cursor = [], None
    for cyc in range(cycles + 1):
        rec = {}
        for when in ("open", "allocated"):  # the snapshot (every task Pending), then what allocate left
            if when == "allocated":
                _abi.check(L.kbg_allocate(ssn.handle, buf, cap, ctypes.byref(n)))
                rec["decisions"] = n.value
            for kind in ("device", "host"):
                os.environ.pop("KBG_HOST_TASK_HEADROOM", None)
                if kind == "host":
                    os.environ["KBG_HOST_TASK_HEADROOM"] = "1"
                mark(f"cycle {cyc} {when}_room_{kind}")
                t0 = time.perf_counter()
                _abi.check(L.kbg_task_headroom(ssn.handle, arr, len(tasks), 1024, room))
                rec[f"{when}_room_{kind}_wall_ms"] = (time.perf_counter() - t0) * 1e3
            os.environ.pop("KBG_HOST_TASK_HEADROOM", None)
            for limit in LIMITS:
                for kind in ("device", "host"):
                    if kind == "host":
                        os.environ["KBG_HOST_JOB_FIT"] = "1"
                    key = f"{when}_{limit}_{kind}"
                    mark(f"cycle {cyc} {key}")
                    t0 = time.perf_counter()  # the C call alone (Session.job_fit adds a dict per row)
                    _abi.check(L.kbg_job_fit(ssn.handle, None, nj, limit, rows, places, cap, ctypes.byref(need)))
                    rec[f"{key}_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    os.environ.pop("KBG_HOST_JOB_FIT", None)
                    rec[f"{key}_digest"] = hash(bytes(rows) + bytes(places)[:need.value * 16])
                    if kind == "device":
                        valid = [r for r in rows if r.valid]
                        rec[f"{when}_{limit}_rows"] = [len(valid), need.value, sum(r.placed_idle for r in valid),
                                                       sum(r.placed_releasing for r in valid),
                                                       sum(r.ready_after >= 0 for r in valid)]
                rec[f"{when}_{limit}_paths_equal"] = rec.pop(f"{when}_{limit}_device_digest") == \
                    rec.pop(f"{when}_{limit}_host_digest")
        if cyc == cycles:  # (rows and places hold the host path's answer at limit 512, the same bytes)
            cursor = dict(cursor_figures(ssn, fx, rows, places), state="after allocate")
            if not cursor["jobs"]:  # allocate left nothing Pending: the snapshot's launch instead
                _abi.check(L.kbg_session_reset(ssn.handle))
                _abi.check(L.kbg_job_fit(ssn.handle, None, nj, 512, rows, places, cap, ctypes.byref(need)))
                cursor = dict(cursor_figures(ssn, fx, rows, places), state="at open")
        out.append(rec)
        _abi.check(L.kbg_session_reset(ssn.handle))
    ssn.close()
    print(json.dumps({"nodes": len(fx["nodes"]), "jobs": nj, "tasks_asked": len(tasks), "cycles": out,
                      "cursor": cursor}), flush=True)


def spread(v):
    v = [x for x in v if x is not None]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} if v else None


def main():
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    config = sys.argv[2] if len(sys.argv) > 2 else "3"
    env = dict(os.environ, KBG_PROFILE_JOB_FIT="1", KBG_PROFILE_TASK_HEADROOM="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(cycles), config], env=env,
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(p.returncode)
    data = json.loads(p.stdout.strip().splitlines()[-1])
    kern, at = {}, None  # the library's line after each of the child's markers
    for line in p.stderr.splitlines():
        m = re.match(r"\[bench\] cycle (\d+) (\w+)", line)
        if m:
            at = (int(m.group(1)), m.group(2))
            continue
        m = re.match(r"\[kbg job fit\] (\d+) jobs, (\d+) steps, (\d+) shapes, .*kernel ([\d.]+) ms", line) or \
            re.match(r"\[kbg task headroom\] (\d+) tasks, (\d+) keys, ()limit.*kernel ([\d.]+) ms", line)
        if m and at:
            kern[at] = (m.group(2), m.group(3), float(m.group(4)) * 1e3)
            at = None
    timed = data["cycles"][1:]
    cur = data["cursor"]
    for k in ("cursor", "no_cursor") if cur.get("jobs") else ():
        cur[k]["kernel_us"] = spread(cur[k]["kernel_us"])
    res = {"config": int(config), "nodes": data["nodes"], "jobs": data["jobs"], "tasks_asked": data["tasks_asked"],
           "timed_cycles": len(timed), "cursor_limit_512": cur}
    for when in ("open", "allocated"):
        ks = [k for k in (kern.get((c, f"{when}_room_device")) for c in range(1, cycles + 1)) if k]
        res[when] = {"task_headroom_limit_1024": {
            "keys": int(ks[0][0]) if ks else 0, "kernel_us": spread([k[2] for k in ks]),
            "call_wall_ms": spread([c[f"{when}_room_device_wall_ms"] for c in timed]),
            "host_path_wall_ms": spread([c[f"{when}_room_host_wall_ms"] for c in timed])}}
        for limit in LIMITS:
            ks = [k for k in (kern.get((c, f"{when}_{limit}_device")) for c in range(1, cycles + 1)) if k]
            res[when][f"limit_{limit}"] = {
                "jobs_valid, steps, placed_idle, placed_releasing, jobs_ready_within": timed[0][f"{when}_{limit}_rows"] if timed else None,
                "shapes": int(ks[0][1]) if ks else 0,
                "paths_equal": all(c[f"{when}_{limit}_paths_equal"] for c in data["cycles"]),
                "fit_kernel_us": spread([k[2] for k in ks]),
                "call_wall_ms": spread([c[f"{when}_{limit}_device_wall_ms"] for c in timed]),
                "host_path_wall_ms": spread([c[f"{when}_{limit}_host_wall_ms"] for c in timed])}
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
