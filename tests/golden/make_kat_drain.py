"""Hand-derived known-answer fixture for kbg_node_drain
(tests/golden/kat_drain.json, checked by tests/test_hostsim_drain.py and
tests/test_drain_gpu.py). Every expected number below was derived by reading
the cited reference code, not by running any implementation.

Run: python tests/golden/make_kat_drain.py

The session is described as it is at open; no pod is Pending, so the fixture's
own cycle decides nothing. Tiers [priority, gang], [drf, predicates,
proportion]. Nodes d00..d03 of 4000m / 8192Mi / 110 pods, d00 and d01 with the
label zone=a, d02 and d03 with zone=b; every pod is Running and asks for 64Mi:
  d00  a0 1000m, a1 1000m (job A, MinMember 2), e0 without a request (job E:
       Resreq.IsEmpty(), backfill's pod), p0 and p1 of 100m, each with host port
       8080/TCP (job P, MinMember 1)                          Idle 1800m
  d01  x0 3500m, label app=anchor                             Idle 500m
  d02  y0 1800m with a required podAntiAffinity to app=anchor over the zone,
       y1 1500m with a deletionTimestamp: Releasing           Idle 700m, Releasing 1500m
  d03  z0 3000m (job Z, MinMember 1)                          Idle 1000m
  ""   g0, Succeeded, names the node `ghost`, which no Node object describes:
       a NodeInfo with a nil Node and no task (event_handlers.go:49-58); under
       the predicates plugin it takes nothing (predicates.go:122-123) and every
       row has panic_nodes 1.

Draining d00 moves, in NodeInfo.Tasks order, a0, a1, e0, p0, p1 (all Running:
AllocatedStatus, api/helpers.go:63-70); d00 itself takes nothing.
  a0 1000m  d01 Idle 500m: no, Releasing 0: no. d02 Idle 700m: no; Releasing
            1500m: LessEqual (allocate.go:148-162)                 -> d02 Pipeline
  a1 1000m  d01 no. d02 Idle 700m no, Releasing 500m left: no. d03 Idle 1000m:
            LessEqual (allocate.go:136-146)                        -> d03 Allocate
  e0 empty  no resource test, the first node past the predicates
            (backfill.go:47-64)                                    -> d01 Allocate
  p0 100m   d01 Idle 500m                                          -> d01 Allocate
  p1 100m   d01: p0's port 8080 joined the node's in the row's view
            (predicates.go:143-155): no. d02 Idle 700m             -> d02 Allocate
The two pods that share a port land on two nodes. Nothing is unplaced, no gang
is short.
Draining d02: y1 is Releasing and is not moved (other_pods 1). y0 1800m: pod
affinity as it is now (predicates.go:185-198, vendor predicates.go:1155-1466;
every row has affinity_now 1): x0, app=anchor, runs in zone a, so y0's anti
term fails d00 and d01; d03 Idle 1000m: no. Nowhere, where d00's Idle 1800m
would have taken it; job Y (ready 1: y1 is Releasing; MinMember 1) breaks. No
other moved pod has a term or is selected by one: y0's term selects app=anchor
pods only (x0 is not moved here), and the other walks are as without it.
Draining d03: z0 3000m: d00 1800m, d01 500m, d02 700m / 1500m: nowhere. Job Z
is ready now (1 >= MinMember 1, gang.go:44-78) and is not without z0:
jobs_short 1.
Draining d00 with d02 cordoned: a0: d01 no, d03 Idle 1000m         -> d03 Allocate
  a1: d01 no, d03 Idle 0: nowhere; job A (ready 2, MinMember 2) breaks.
  e0 -> d01, p0 -> d01 as before. p1: d01 holds the port, d02 is cordoned, d03
  has 0m left: |0 - 100| is not below 10: nowhere; job P (ready 2, MinMember 1)
  keeps its minimum. jobs_short 1."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def pod(uid, group, cpu, node_name, ports=None, **kw):
    c = {"requests": {"cpu": f"{cpu}m", "memory": "64Mi"}} if cpu else {}
    if ports:
        c["ports"] = ports
    return dict({"uid": uid, "namespace": "ns", "name": uid, "phase": "Running", "nodeName": node_name,
                 "annotations": {"scheduling.k8s.io/group-name": group}, "containers": [c]}, **kw)


PORT = [{"hostPort": 8080, "protocol": "TCP"}]
A, P = "allocate", "pipeline"
AFF = " (pod affinity as it is now)"


def row(node, cordon, places, message, **fields):
    placed = [p for p in places if p[1] is not None]
    base = dict(node=node, cordon=list(cordon), places=[list(p) for p in places], tasks=len(places), walked=len(places),
                placed_idle=sum(p[2] == A for p in placed), placed_releasing=sum(p[2] == P for p in placed),
                unplaced=len(places) - len(placed), first_unplaced=next((p[0] for p in places if p[1] is None), None),
                nodes_used=len({p[1] for p in placed}), other_pods=0, jobs_short=0, panic_nodes=1, affinity_now=True,
                message=message + AFF)
    base.update(fields)
    return base


FIXTURE = {
    "name": "kat_drain", "actions": ["allocate"],
    "tiers": [[{"name": "priority"}, {"name": "gang"}], [{"name": "drf"}, {"name": "predicates"}, {"name": "proportion"}]],
    "nodes": [{"name": f"d{i:02d}", "allocatable": {"cpu": "4000m", "memory": "8192Mi", "pods": "110"},
               "labels": {"zone": "a" if i < 2 else "b"}} for i in range(4)],
    "queues": [{"name": "q", "weight": 1}],
    "podGroups": [{"namespace": "ns", "name": g, "minMember": m, "queue": "q", "creationTimestamp": t * 10 ** 9}
                  for t, (g, m) in enumerate((("A", 2), ("E", 1), ("P", 1), ("X", 1), ("Y", 1), ("Z", 1)), 1)],
    "pods": [pod("a0", "A", 1000, "d00"), pod("a1", "A", 1000, "d00"), pod("e0", "E", 0, "d00"),
             pod("p0", "P", 100, "d00", ports=PORT), pod("p1", "P", 100, "d00", ports=PORT),
             pod("x0", "X", 3500, "d01", labels={"app": "anchor"}),
             pod("y0", "Y", 1800, "d02", affinity={"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
                 {"labelSelector": {"matchLabels": {"app": "anchor"}}, "topologyKey": "zone"}]}}),
             pod("y1", "Y", 1500, "d02", deletionTimestamp="2026-01-01T00:00:00Z"), pod("z0", "Z", 3000, "d03"),
             pod("g0", "X", 1000, "ghost", phase="Succeeded")],
    "expected": {
        "status": "ok",
        "decisions": [],
        # kbg_node_drain at open: per (node, cordon) the places (task, node or null, kind or null) and the row
        "drain": [
            row("d00", (), [("a0", "d02", P), ("a1", "d03", A), ("e0", "d01", A), ("p0", "d01", A), ("p1", "d02", A)],
                "5 of 5 pods find room (1 on releasing resources, 3 nodes)", jobs_moved=3),
            row("d02", (), [("y0", None, None)],
                "0 of 1 pods find room (0 on releasing resources, 0 nodes); 1 do not, first task y0; breaks 1 gang",
                jobs_moved=1, other_pods=1, jobs_short=1),
            row("d03", (), [("z0", None, None)],
                "0 of 1 pods find room (0 on releasing resources, 0 nodes); 1 do not, first task z0; breaks 1 gang",
                jobs_moved=1, jobs_short=1),
            row("d00", ("d02",), [("a0", "d03", A), ("a1", None, None), ("e0", "d01", A), ("p0", "d01", A),
                                  ("p1", None, None)],
                "3 of 5 pods find room (0 on releasing resources, 2 nodes); 2 do not, first task a1; breaks 1 gang",
                jobs_moved=3, jobs_short=1),
            dict(row("", (), [], "", jobs_moved=0), message="no pods to move"),
        ],
    },
}


def main():
    with open(os.path.join(HERE, FIXTURE["name"] + ".json"), "w") as f:
        json.dump(FIXTURE, f, indent=1)
        f.write("\n")
    print(f"wrote {FIXTURE['name']}.json")


if __name__ == "__main__":
    main()
