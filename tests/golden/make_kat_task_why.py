"""Hand-derived known-answer fixture for kbg_task_reasons
(tests/golden/kat_task_why.json, checked by tests/test_hostsim_task_why.py and
tests/test_task_why_gpu.py). Every expected number below was derived by
reading the cited reference code, not by running any implementation.

Run: python tests/golden/make_kat_task_why.py

The session is described as it is at open (the call is legal before the
cycle's first action). One tier [gang, drf, proportion, predicates]. Queue qb
holds the Running job X, queue qa the Pending job P: qa has allocated nothing
and deserves something, so it is not Overused (proportion.go:188-194).

Nodes n00..n06: 5 CPUs, 16Gi, no GPU; role=w everywhere but n01.
  n00  pods: 1, holds x0                      MaxTaskNum <= len(pods)   (predicates.go:125-127)
  n01  role=x and unschedulable
  n02  unschedulable and tainted (NoSchedule)
  n03  tainted (NoSchedule); no Pending pod tolerates it
  n04  empty                                  Idle (5000, 16Gi, 0), Releasing 0
  n05  x1 Running 4000m                       Idle (1000, 16Gi, 0), Releasing 0
  n06  x2 4000m / 2Gi, being deleted: Releasing (node_info.go:120-135)
                                              Idle (1000, 14Gi, 0), Releasing (4000, 2Gi, 0)

t-sel: 2000m, 1Gi, nodeSelector role=w (allocate.go:119-162)
  n00 POD_CAP; n01 the selector fails before unschedulable: SELECTOR; n02
  unschedulable before taints: UNSCHEDULABLE; n03 TAINTS; n04 LessEqual Idle:
  FITS_IDLE; n05 2000 is neither < 1000 nor within 10 of it, Releasing 0:
  SHORT; n06 not Idle, 2000 < 4000 and 1Gi < 2Gi and |0 - 0| < 10:
  FITS_RELEASING. FitDelta on n05 and n06 (resource_info.go:116-129): cpu
  1000 - 2010 < 0 on both, memory 16Gi / 14Gi - (1Gi + 10Mi) > 0, no GPU
  request: idle_short (2, 0, 0).
t-gpu: 500m and one GPU, no selector
  n00 POD_CAP; n01 and n02 UNSCHEDULABLE; n03 TAINTS; n04, n05, n06: 1000 GPU
  against Idle 0 and Releasing 0: SHORT. FitDelta: cpu 5000 / 1000 / 1000 -
  510 > 0, GPU 0 - 1010 < 0: idle_short (0, 0, 3).
t-be: no requests, Resreq.IsEmpty(): backfill's task, predicates only
  (backfill.go:47-60)
  n00 POD_CAP; n01, n02 UNSCHEDULABLE; n03 TAINTS; n04, n05, n06 FITS_IDLE.

No host-port, pod-affinity or nil-Node cause there: a session holding any takes
the host path for the whole table, and that fixture is for the device kernel
too. The second fixture, tests/golden/kat_task_why_host.json, holds the
host-port and pod-affinity causes (host_task_why answers it on every session).

kat_task_why_host: the same tier and queues. Nodes m0..m3: 5 CPUs, 16Gi; m0
and m1 in zone a, m2 and m3 in zone b; label host = the node's name.
  m0  w0 Running, 1000m, labels app=web, hostPort 8080/TCP   Idle (4000, 16Gi, 0)
  m1  empty
  m2  d0 Running, 1000m, labels app=db                       Idle (4000, 16Gi, 0)
  m3  empty
All pods are in namespace ns, so every term selects within it (vendor
predicates.go:1155-1466); only pods with a node count (the Pending ones do not).

h-port: 1000m, hostPort 8080/TCP
  m0 holds the port: HOST_PORTS (predicates.go:143-155); m1, m2, m3 FITS_IDLE.
h-aff: 1000m, required podAffinity app=web over the zone
  w0 is in zone a: m0 and m1 pass; m2 and m3 hold no app=web pod in their
  zone: POD_AFFINITY (predicates.go:185-198).
h-anti: 1000m, required podAntiAffinity app=db over the host
  m2 holds d0: POD_AFFINITY; m0, m1, m3 FITS_IDLE.
h-big: 10 CPUs, required podAntiAffinity app=web over the zone
  m0 and m1 share w0's zone: POD_AFFINITY, before any resource test; m2 and
  m3 pass the stages, 10000 against Idle 4000 / 5000 and Releasing 0: SHORT,
  FitDelta cpu 4000 / 5000 - 10010 < 0: idle_short (2, 0, 0)."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
TAINT = [{"key": "dedicated", "value": "x", "effect": "NoSchedule"}]


def node(i, pods="110", role="w", **kw):
    n = {"name": f"n{i:02d}", "allocatable": {"cpu": "5", "memory": "16Gi", "pods": pods}, "labels": {"role": role}}
    n.update(kw)
    return n


def pod(uid, group, req, node_name="", **kw):
    p = {"uid": uid, "namespace": "ns", "name": uid, "phase": "Running" if node_name else "Pending",
         "nodeName": node_name, "annotations": {"scheduling.k8s.io/group-name": group},
         "containers": [{"requests": req}]}
    p.update(kw)
    return p


def pg(name, min_member, queue, created):
    return {"namespace": "ns", "name": name, "minMember": min_member, "queue": queue,
            "creationTimestamp": created * 1_000_000_000}


CAP, UNS, TNT = "can not allow more task running on it", "set to unschedulable", "does not tolerate node taints"

FIXTURE = {
    "name": "kat_task_why",
    "actions": ["allocate"],
    "tiers": [[{"name": "gang"}, {"name": "drf"}, {"name": "proportion"}, {"name": "predicates"}]],
    "nodes": [node(0, pods="1"), node(1, role="x", unschedulable=True), node(2, unschedulable=True, taints=TAINT),
              node(3, taints=TAINT), node(4), node(5), node(6)],
    "queues": [{"name": "qa", "weight": 1}, {"name": "qb", "weight": 1}],
    "podGroups": [pg("P", 1, "qa", 100), pg("X", 1, "qb", 1)],
    "pods": [
        pod("t-sel", "P", {"cpu": "2", "memory": "1Gi"}, nodeSelector={"role": "w"}),
        pod("t-gpu", "P", {"cpu": "500m", "nvidia.com/gpu": "1"}),
        pod("t-be", "P", {}),
        pod("x0", "X", {"cpu": "1"}, "n00"), pod("x1", "X", {"cpu": "4"}, "n05"),
        pod("x2", "X", {"cpu": "4", "memory": "2Gi"}, "n06", deletionTimestamp="2026-01-01T00:00:00Z"),
    ],
    "expected": {
        # kbg_task_reasons at open; causes in KBG_WHY_* / KBG_TWHY_* order
        "task_why": [
            {"task": "t-sel", "best_effort": False, "queue_overused": False,
             "count": [1, 1, 0, 1, 1, 0, 1, 1, 1, 0],
             "first_node": ["n00", "n01", None, "n02", "n03", None, "n04", "n06", "n05", None],
             "idle_short": [2, 0, 0],
             "message": "2/7 nodes are available, 1 of them once resources are released."},
            {"task": "t-gpu", "best_effort": False, "queue_overused": False,
             "count": [1, 0, 0, 2, 1, 0, 0, 0, 3, 0],
             "first_node": ["n00", None, None, "n01", "n03", None, None, None, "n04", None],
             "idle_short": [0, 0, 3],
             "message": f"0/7 nodes are available: 1 {CAP}, 1 {TNT}, 2 {UNS}, 3 insufficient GPU."},
            {"task": "t-be", "best_effort": True, "queue_overused": False,
             "count": [1, 0, 0, 2, 1, 0, 3, 0, 0, 0],
             "first_node": ["n00", None, None, "n01", "n03", None, "n04", None, None, None],
             "idle_short": [0, 0, 0],
             "message": "3/7 nodes are available."},
        ],
    },
}


AFF = "affinity/anti-affinity failed"


def mnode(i, zone):
    return {"name": f"m{i}", "allocatable": {"cpu": "5", "memory": "16Gi", "pods": "110"},
            "labels": {"zone": zone, "host": f"m{i}"}}


def term(app, key):
    return {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": key}]}


PORT = [{"hostPort": 8080, "protocol": "TCP"}]


def ported(p):
    p["containers"][0]["ports"] = PORT
    return p


HOST_FIXTURE = {
    "name": "kat_task_why_host",
    "actions": ["allocate"],
    "tiers": [[{"name": "gang"}, {"name": "drf"}, {"name": "proportion"}, {"name": "predicates"}]],
    "nodes": [mnode(0, "a"), mnode(1, "a"), mnode(2, "b"), mnode(3, "b")],
    "queues": [{"name": "qa", "weight": 1}, {"name": "qb", "weight": 1}],
    "podGroups": [pg("P", 1, "qa", 100), pg("X", 1, "qb", 1)],
    "pods": [
        ported(pod("h-port", "P", {"cpu": "1"}, labels={"app": "client"})),
        pod("h-aff", "P", {"cpu": "1"}, labels={"app": "client"}, affinity={"podAffinity": term("web", "zone")}),
        pod("h-anti", "P", {"cpu": "1"}, labels={"app": "client"}, affinity={"podAntiAffinity": term("db", "host")}),
        pod("h-big", "P", {"cpu": "10"}, labels={"app": "client"}, affinity={"podAntiAffinity": term("web", "zone")}),
        ported(pod("w0", "X", {"cpu": "1"}, "m0", labels={"app": "web"})),
        pod("d0", "X", {"cpu": "1"}, "m2", labels={"app": "db"}),
    ],
    "expected": {
        "task_why": [
            {"task": "h-port", "best_effort": False, "queue_overused": False,
             "count": [0, 0, 1, 0, 0, 0, 3, 0, 0, 0],
             "first_node": [None, None, "m0", None, None, None, "m1", None, None, None],
             "idle_short": [0, 0, 0], "message": "3/4 nodes are available."},
            {"task": "h-aff", "best_effort": False, "queue_overused": False,
             "count": [0, 0, 0, 0, 0, 2, 2, 0, 0, 0],
             "first_node": [None, None, None, None, None, "m2", "m0", None, None, None],
             "idle_short": [0, 0, 0], "message": "2/4 nodes are available."},
            {"task": "h-anti", "best_effort": False, "queue_overused": False,
             "count": [0, 0, 0, 0, 0, 1, 3, 0, 0, 0],
             "first_node": [None, None, None, None, None, "m2", "m0", None, None, None],
             "idle_short": [0, 0, 0], "message": "3/4 nodes are available."},
            {"task": "h-big", "best_effort": False, "queue_overused": False,
             "count": [0, 0, 0, 0, 0, 2, 0, 0, 2, 0],
             "first_node": [None, None, None, None, None, "m0", None, None, "m2", None],
             "idle_short": [2, 0, 0],
             "message": f"0/4 nodes are available: 2 {AFF}, 2 insufficient cpu."},
        ],
    },
}


def main():
    for fx in (FIXTURE, HOST_FIXTURE):
        with open(os.path.join(HERE, fx["name"] + ".json"), "w") as f:
            json.dump(fx, f, indent=1)
            f.write("\n")
        print(f"wrote {fx['name']}.json")


if __name__ == "__main__":
    main()
