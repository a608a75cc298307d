"""The cases of the dead-mask tests (tests/test_dead_masks.py on hostsim,
tests/test_dead_masks_gpu.py on the device) and their runner: every case runs
twice in one process, with the in-order commit's dead masks and
with KBG_DEAD_MASKS=0 (the walk without them; the library reads the switch at
the start of every allocate cycle).

    python tests/dead_masks_cases.py CASES.json OUT.json

is the hostsim child (KBG_LIB_PATH names tools/libkbg_hostsim.so, the schedule
is in KBG_HOSTSIM_SCHEDULE): OUT.json maps a case id to {"on": record, "off":
record}, a record being the outputs in the oracle's schema and the cycle's
resolve counters."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))
sys.path.insert(0, HERE)

SATURATED = [dict(id="saturated130", gen="saturated", kw=dict(nodes=130, jobs=60, tasks_per_job=10)),
             dict(id="saturated65", gen="saturated", kw=dict(nodes=65, jobs=40, tasks_per_job=8, seed=3))]
EDGES = [dict(id=f"edges{n}", gen="edges", kw=dict(nodes=n)) for n in (64, 65)]
RANDOM = [dict(id=f"random{s}", gen="random", arg=s, only_allocate_backfill=True) for s in range(60)]
# pod affinity switches the masks off; the fixture keeps its own reclaim / preempt actions, whose
# resolvers never have them
AFFINITY = [dict(id=f"affinity{s}", gen="contended", arg=s, kw=dict(nodes=40, jobs=30, tasks=10, queues=3, aff=0.5))
            for s in (7004, 7010)]  # (their allocate evaluates 58 and 59 tasks and re-checks candidates)
MODES = (("prod", {"batch_tasks": 64}), ("full", {"batch_tasks": 64, "full_scan": 1}))


def with_modes(cases):
    return [dict(c, id=f"{c['id']}-{m}", opts=o) for c in cases for m, o in MODES]


HOST_CASES = with_modes(SATURATED + EDGES + RANDOM + AFFINITY)
GPU_CASES = with_modes(SATURATED + EDGES)


def edges_fixture(nodes=65):
    """A hand-made session for the edges of the masks. Every node has 4 CPUs,
    8 GiB and 2 GPUs; one queue, gang jobs of minMember 1 in drf order, so
    tasks of many shapes share a batch of 64 and re-check the nodes the tasks
    before them filled.

    * cpu-tol asks 2004m: the second task on a node meets Idle 1996m, short by
      less than the 10m tolerance, and must still be placed there (Idle -8m);
      cpu-exact asks 2005m: short by exactly 10m, which does not fit.
    * mem-tol asks 4100Mi (the second meets 4092Mi, 8Mi short of 10Mi; a
      taint keeps nodes 4-10 for it, two tasks each, so the case is sure to
      arise); gpu-tol asks 1004m of a GPU (the second meets 996m).
    * nodes 3, 20 and the last one run a deleting pod of 3 CPUs and 6 GiB:
      Idle is short for a 2-CPU task, Releasing fits it (Pipeline).
    * zero-mem and zero-all-but-cpu ask nothing in one or two dimensions;
      best-effort asks 5m (below every tolerance: backfill places it, on
      node 2, which a taint keeps for it: the reference panics when such a
      pod lands on a node whose Idle a tolerance placement left negative).
    * nodes 1, 21 and the last but one take 2 pods; with the predicates
      plugin they are full after two tasks whatever their resources.
    * small (250m, 256Mi; more tasks than fit) sweeps what the others left
      on every node up to the last one, past the full nodes.
    * 64 or 65 nodes: the last node is bit 63 of word 0 or bit 0 of word 1.
    """
    G = "nvidia.com/gpu"
    capped = {1, 21, nodes - 2}
    releasing = {3, 20, nodes - 1}
    nds = [{"name": f"n{i:02d}", "labels": {},
            "allocatable": {"cpu": "4", "memory": "8Gi", G: "2", "pods": "2" if i in capped else "110"}}
           for i in range(nodes)]
    nds[2]["labels"]["be"] = "yes"
    nds[2]["taints"] = [{"key": "dedicated", "value": "be", "effect": "NoSchedule"}]
    for i in range(4, 11):
        nds[i]["taints"] = [{"key": "dedicated", "value": "mem", "effect": "NoSchedule"}]
    pods, pgs = [], []
    for i in sorted(releasing):
        pods.append({"uid": f"leaving-{i:02d}", "namespace": "ns", "name": f"leaving-{i:02d}", "phase": "Running",
                     "nodeName": nds[i]["name"], "deletionTimestamp": "2026-01-01T00:00:00Z",
                     "containers": [{"requests": {"cpu": "3", "memory": "6Gi"}}]})
    jobs = [("cpu-tol", {"cpu": "2004m", "memory": "1Gi"}, 14), ("cpu-exact", {"cpu": "2005m", "memory": "1Gi"}, 14),
            ("mem-tol", {"cpu": "500m", "memory": "4100Mi"}, 14), ("gpu-tol", {"cpu": "500m", "memory": "512Mi", G: "1004m"}, 14),
            ("pipe", {"cpu": "2", "memory": "2Gi"}, 20), ("zero-mem", {"cpu": "1"}, 20),
            ("zero-cpu", {"memory": "1Gi", G: "1"}, 16), ("small", {"cpu": "250m", "memory": "256Mi"}, 160),
            ("big", {"cpu": "3", "memory": "6Gi", G: "2"}, 12), ("best-effort", {"cpu": "5m"}, 6),
            ("wide", {"cpu": "3500m", "memory": "7Gi"}, 70)]
    for j, (name, req, n) in enumerate(jobs):
        pgs.append({"namespace": "ns", "name": name, "minMember": 1, "queue": "q1",
                    "creationTimestamp": (100 + j) * 1_000_000_000})
        for t in range(n):
            pods.append({"uid": f"{name}-{t:02d}", "namespace": "ns", "name": f"{name}-{t:02d}", "phase": "Pending",
                         "nodeName": "", "annotations": {"scheduling.k8s.io/group-name": name},
                         "containers": [{"requests": dict(req)}]})
            if name == "mem-tol":
                pods[-1]["tolerations"] = [{"key": "dedicated", "operator": "Equal", "value": "mem", "effect": "NoSchedule"}]
            if name == "best-effort":
                pods[-1].update(nodeSelector={"be": "yes"}, tolerations=[
                    {"key": "dedicated", "operator": "Equal", "value": "be", "effect": "NoSchedule"}])
    return {"name": f"dead-mask-edges-{nodes}", "tiers": None, "nodes": nds, "pods": pods, "podGroups": pgs,
            "queues": [{"name": "q1", "weight": 1}], "actions": ["allocate", "backfill"]}


def make_fixture(c):
    if c["gen"] == "edges":
        return edges_fixture(**c.get("kw", {}))
    from hostsim_worker import make_fixture as mk
    return mk(c)


def run_case(c, extra_opts=None):
    """{"on": record, "off": record} of one case in this process."""
    from kbgpu.fixture import run_fixture
    fx = make_fixture(c)
    rec = {}
    for key in ("on", "off"):
        if key == "off":
            os.environ["KBG_DEAD_MASKS"] = "0"
        else:
            os.environ.pop("KBG_DEAD_MASKS", None)
        try:
            got, ssn = run_fixture(fx, dict(c.get("opts") or {}, **(extra_opts or {})))
            r = {"out": got}
            if ssn:
                st = ssn.stats()
                r["stats"] = {k: int(getattr(st, k)) for k in ("resolve_rechecks", "resolve_steps", "task_evaluations")}
                ssn.close()
        except Exception as e:  # the case fails in the parent; the others still run
            r = {"error": f"{type(e).__name__}: {e}"}
        finally:
            os.environ.pop("KBG_DEAD_MASKS", None)
        rec[key] = r
    return rec


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        cases = json.load(f)
    with open(sys.argv[2], "w") as f:
        json.dump({c["id"]: run_case(c) for c in cases}, f)
