"""Developer tool: what kbg_node_drain costs on BASELINE C3 (5k nodes x 100k
tasks, synth.config_fixture(3)). One resident session opened with reasons runs
allocate for `cycles` + 1 cycles (kbg_session_reset between them; the first
cycle warms up and is dropped). After each allocate (the nodes hold what the
cycle allocated) it drains every node alone at limit 512 and at limit 16 on the
device-shaped path, the same with KBG_HOST_NODE_DRAIN=1 in the last cycle only
(the host walk of every node takes seconds), and one node (the one holding the
most pods) at limit 512. With KBG_PROFILE_NODE_DRAIN the library prints the
walks, steps and shapes of a call and the HIP-event time of its kernel
launches (the events bracket the kernel alone).

Every walk is one wave and one serial chain. For the all-nodes calls the tool
counts every chain's step-words from the places and sets the kernel time over
the sum of the longest chain of each launch (4096 walks a launch, about 1000
waves resident at four workgroups per CU): the loaded figure, as
kbg_job_fit_kernel's is (1452 chains in one launch). The one-node call is one
walk alone on the device: its step-words (per
step the 64-node words from its shape's cursor to the word it lands in, every
word from the cursor on where it lands nowhere) are counted here from the
places, and the kernel time over them is the figure to set beside
kbg_job_fit_kernel's microseconds per word of one chain (tools/job_fit_bench.py).

Prints one JSON line; no threshold is set.
python kube-arbitrator_amd/tools/drain_bench.py [cycles] [config]"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

CALLS = (("all_512", None, 512), ("all_16", None, 16), ("one_512", "one", 512))


def step_words(ssn, places, n_nodes):
    """The 64-node words one walk's steps scan under the per-shape cursor."""
    tasks = ssn.flat.task_objs
    words, total, cursor = (n_nodes + 63) // 64, 0, {}
    for p in places:
        t = tasks[p.task]
        key = (json.dumps({k: t.pod.get(k) for k in ("nodeSelector", "affinity", "tolerations")}, sort_keys=True),
               tuple(float(v) for v in t.resreq.as_tuple()))
        start = cursor.get(key, 0)
        if start < 0:  # its shape's previous step landed nowhere: no scan
            continue
        total += (p.node // 64 if p.node >= 0 else words - 1) - start // 64 + 1
        cursor[key] = p.node
    return total


def child(cycles, config):
    import ctypes
    from kbgpu import _abi, synth
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
    rows = (_abi.kbg_node_drain * N)()
    places = (_abi.kbg_fit_place * cap)()
    need = ctypes.c_int32(0)
    out, one = [], None
    for cyc in range(cycles + 1):
        rec = {}
        _abi.check(L.kbg_allocate(ssn.handle, buf, cap, ctypes.byref(n)))
        rec["decisions"] = n.value
        for call, pick, limit in CALLS:
            for kind in ("device", "host"):
                if kind == "host" and cyc != cycles:
                    continue
                if pick and one is None:  # the node holding the most pods (from the whole call before)
                    one = max(range(N), key=lambda i: rows[i].tasks if rows[i].valid else -1)
                arr = (ctypes.c_int32 * 1)(one) if pick else None
                if kind == "host":
                    os.environ["KBG_HOST_NODE_DRAIN"] = "1"
                sys.stderr.write(f"[bench] cycle {cyc} {call}_{kind}\n")
                sys.stderr.flush()
                t0 = time.perf_counter()  # the C call alone (Session.node_drain adds a dict per row)
                st = L.kbg_node_drain(ssn.handle, arr, 1 if pick else N, None, 0, limit, rows, places, cap,
                                      ctypes.byref(need))
                rec[f"{call}_{kind}_wall_ms"] = (time.perf_counter() - t0) * 1e3
                os.environ.pop("KBG_HOST_NODE_DRAIN", None)
                if st != _abi.KBG_OK:
                    rec[f"{call}_{kind}_status"] = int(st)
                    continue
                used = rows[:1] if pick else rows
                rec[f"{call}_{kind}_digest"] = hash(bytes(rows)[:len(used) * 64] + bytes(places)[:need.value * 16])
                if kind == "device":
                    valid = [r for r in used if r.valid]
                    rec[f"{call}_rows"] = dict(nodes=len(valid), steps=need.value,
                                               placed_idle=sum(r.placed_idle for r in valid),
                                               placed_releasing=sum(r.placed_releasing for r in valid),
                                               unplaced=sum(r.unplaced for r in valid),
                                               jobs_short=sum(r.jobs_short for r in valid))
                    if pick:
                        rec["one_step_words"] = step_words(ssn, places[:need.value], N)
                    elif cyc == 1:  # the loaded launches: every walk's chain, per launch of 4096 walks its longest
                        chains = [step_words(ssn, places[r.place_off:r.place_off + r.walked], N) if r.valid else 0
                                  for r in rows]
                        rec[f"{call}_chains"] = dict(
                            step_words=sum(chains), longest_per_launch=[max(chains[i:i + 4096])
                                                                        for i in range(0, len(chains), 4096)])
        out.append(rec)
        _abi.check(L.kbg_session_reset(ssn.handle))
    ssn.close()
    print(json.dumps({"nodes": N, "tasks": cap - 1, "cycles": out}), flush=True)


def spread(v):
    v = [x for x in v if x is not None]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} if v else None


def main():
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    config = sys.argv[2] if len(sys.argv) > 2 else "3"
    env = dict(os.environ, KBG_PROFILE_NODE_DRAIN="1")
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
        m = re.match(r"\[kbg node drain\] (\d+) walks, (\d+) steps, (\d+) shapes, limit \d+, (\d+) launches, "
                     r"drain kernel ([\d.]+) ms", line)
        if m and at:
            kern[at] = (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)) * 1e3)
            at = None
    timed = data["cycles"][1:]
    res = {"config": int(config), "nodes": data["nodes"], "tasks": data["tasks"], "timed_cycles": len(timed),
           "state": "after allocate"}
    for call, _, _ in CALLS:
        ks = [k for k in (kern.get((c, f"{call}_device")) for c in range(1, cycles + 1)) if k]
        last = data["cycles"][-1]
        res[call] = {
            "rows": timed[0].get(f"{call}_rows") if timed else None,
            "walks, steps, shapes, launches": list(ks[0][:4]) if ks else None,
            "drain_kernel_us": spread([k[4] for k in ks]),
            "call_wall_ms": spread([c.get(f"{call}_device_wall_ms") for c in timed]),
            "host_path_wall_ms": last.get(f"{call}_host_wall_ms"),
            "paths_equal": last.get(f"{call}_device_digest") == last.get(f"{call}_host_digest"),
            "status": last.get(f"{call}_device_status", 0)}
        ch = timed[0].get(f"{call}_chains") if timed else None
        if ch and res[call]["drain_kernel_us"]:
            # the launches of a call run one after the other; each lasts at least as long as its longest chain
            res[call]["chains"] = ch
            res[call]["us_per_step_word_of_the_longest_chains"] = \
                res[call]["drain_kernel_us"]["median"] / max(1, sum(ch["longest_per_launch"]))
    words = timed[0].get("one_step_words") if timed else None
    us = res["one_512"]["drain_kernel_us"]
    res["one_512"]["step_words"] = words
    res["one_512"]["us_per_step_word"] = us["median"] / words if us and words else None
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
