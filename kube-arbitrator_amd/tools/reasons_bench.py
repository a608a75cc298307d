"""Developer tool: what kbg_options.reasons costs on a config (default C3).
Two child processes run the same allocate cycles on one resident session,
with the option off and on; the one with it on sets KBG_PROFILE_REASONS, so
the library reports, per cycle, the HIP-event time around kbg_fitdelta_kernel
and around kbg_reasons_kernel (launched back to back on the session's stream)
and, once, the build of the stage planes (kernel, download and wait). Prints
one JSON line: medians over the timed cycles of the two kernels' times and of
the allocate wall time with the option off and on.
python kube-arbitrator_amd/tools/reasons_bench.py [config] [cycles]"""
import json
import os
import re
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def child(cid, cycles, reasons):
    import ctypes
    from kbgpu import _abi, synth
    from kbgpu.cache import FakeBinder, cache_from_fixture
    from kbgpu.fixture import _OrderedCache, fixture_tiers
    from kbgpu.framework import open_session
    fx = synth.config_fixture(cid)
    ssn = open_session(_OrderedCache(cache_from_fixture(fx, FakeBinder()), fx), fixture_tiers(fx), {"device": 0},
                       reasons=bool(reasons))
    L = _abi.lib()
    cap = len(ssn.flat.task_objs) + 1
    buf, n = (_abi.kbg_decision * cap)(), ctypes.c_int32(0)
    ms, reported = [], 0
    for _ in range(cycles + 1):  # the first cycle warms up (and builds the planes)
        _abi.check(L.kbg_allocate(ssn.handle, buf, cap, ctypes.byref(n)))
        ms.append(ssn.stats().allocate_ms)
        if reasons:
            reported = sum(ssn.job_reasons(j).valid for j in range(len(ssn.jobs)))
        _abi.check(L.kbg_session_reset(ssn.handle))
    ssn.close()
    print(json.dumps({"allocate_ms": ms[1:], "decisions": n.value, "reported_jobs": reported}), flush=True)


def run(cid, cycles, reasons):
    env = dict(os.environ)
    env.pop("KBG_PROFILE_REASONS", None)
    if reasons:
        env["KBG_PROFILE_REASONS"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(cid), str(cycles), str(reasons)],
                       env=env, capture_output=True, text=True, check=True)
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def main():
    cid = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    off, _ = run(cid, cycles, 0)
    on, err = run(cid, cycles, 1)
    kern = re.findall(r"\[kbg reasons\] (\d+) queries x (\d+) nodes: fitdelta kernel ([\d.]+) us, reasons kernel ([\d.]+) us",
                      err)
    planes = re.findall(r"\[kbg reasons\] stage planes (\d+) classes x (\d+) words: ([\d.]+) us "
                        r"\(alloc ([\d.]+), kernel ([\d.]+), download ([\d.]+)\)", err)
    med = statistics.median
    res = {"config": cid, "cycles": cycles, "decisions": on["decisions"], "reported_jobs": on["reported_jobs"],
           "allocate_ms_off": round(med(off["allocate_ms"]), 3), "allocate_ms_on": round(med(on["allocate_ms"]), 3),
           "allocate_ms_off_range": [round(min(off["allocate_ms"]), 3), round(max(off["allocate_ms"]), 3)],
           "allocate_ms_on_range": [round(min(on["allocate_ms"]), 3), round(max(on["allocate_ms"]), 3)]}
    if kern:
        timed = kern[1:] or kern  # without the warm-up cycle
        res.update(queries=int(kern[0][0]), nodes=int(kern[0][1]),
                   fitdelta_kernel_us=round(med(float(k[2]) for k in timed), 1),
                   reasons_kernel_us=round(med(float(k[3]) for k in timed), 1))
    if planes:
        res.update(classes=int(planes[0][0]), plane_words=int(planes[0][1]),
                   plane_build_us=[{"total": float(x[2]), "alloc": float(x[3]), "kernel": float(x[4]),
                                    "download": float(x[5])} for x in planes])
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
