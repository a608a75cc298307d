"""Hand-derived known-answer fixtures for kbg_task_headroom
(tests/golden/kat_headroom.json and kat_headroom_dev.json, checked by
tests/test_hostsim_headroom.py and tests/test_headroom_gpu.py). Every expected
number below was derived by reading the cited reference code, not by running
any implementation.

Run: python tests/golden/make_kat_headroom.py

Both sessions are described as they are at open, with limit 8, on the clusters
of tests/golden/make_kat_task_why.py (whose docstring derives each node's
predicate verdict). A copy goes onto a node by Resreq.LessEqual(node.Idle)
then Idle.Sub, else LessEqual(node.Releasing) then Releasing.Sub
(allocate.go:119-162, node_info.go:101-129), LessEqual being `r < a ||
|a - r| < min` per dimension (resource_info.go:142-146, min 10m / 10Mi / 10),
under the pod cap (predicates.go:125-127).

kat_headroom_dev (no host port, no pod affinity: the device kernel answers).
Past the predicates for every Pending pod: n04 Idle (5000, 16Gi, 0), no pod;
n05 Idle (1000, 16Gi, 0), one pod; n06 Idle (1000, 14Gi, 0), Releasing
(4000, 2Gi, 0), one pod (x2, being deleted, is still in NodeInfo.Tasks). The
pod cap is 110: rooms 110, 109, 109.
t-sel: 2000m, 1Gi
  n04 5000 -> 3000 -> 1000; 2000 is neither < 1000 nor within 10 of it: 2 from
  Idle. n05 none, Releasing 0: none. n06 none from Idle; Releasing (4000, 2Gi)
  -> (2000, 1Gi): 2000 < 2000 fails but |2000 - 2000| < 10 and |1Gi - 1Gi| <
  10Mi hold -> (0, 0); then nothing: 2 from Releasing.
t-gpu: 500m and one GPU: 1000 against Idle 0 and Releasing 0 everywhere: none.
t-be: no requests, Resreq.IsEmpty(): no resource test (backfill.go:47-60):
  min(limit 8, room) = 8 on each of the three nodes, each cut by the limit.

kat_headroom (host ports and pod affinity: host_headroom answers, and every
row carries affinity_now = 1). m0 Idle (4000, 16Gi, 0), m1 (5000, 16Gi, 0),
m2 (4000, 16Gi, 0), m3 (5000, 16Gi, 0); Releasing 0; rooms 109, 110, 109, 110.
h-port: 1000m, hostPort 8080/TCP
  m0 holds the port. m1, m2, m3 pass; Idle would hold 5, 4, 5 copies, but the
  first copy's port conflicts with the second's (predicates.go:143-155): one a
  node, and no node is cut by the limit.
h-aff: 1000m, podAffinity app=web over the zone: m0 and m1 pass (the verdict
  of now, for every copy): 4000 / 1000 = 4 and 5000 / 1000 = 5 copies, the
  next one against Idle 0.
h-anti: 1000m, podAntiAffinity app=db over the host: m0, m1, m3: 4 + 5 + 5.
h-big: 10 CPUs: m2 and m3 pass the stages and hold none."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_kat_task_why as k  # noqa: E402  (the two clusters)

LIMIT = 8


def row(task, needed, best_effort, nodes_pass, copies_idle, copies_releasing, nodes_idle, nodes_releasing_only,
        first_node, max_node_copies, limit_hit, affinity_now, message):
    return dict(task=task, needed=needed, best_effort=best_effort, queue_overused=False, limit=LIMIT,
                nodes_pass=nodes_pass, copies_idle=copies_idle, copies_releasing=copies_releasing,
                nodes_idle=nodes_idle, nodes_releasing_only=nodes_releasing_only, first_node=first_node,
                max_node_copies=max_node_copies, limit_hit=limit_hit, affinity_now=affinity_now, panic_nodes=0,
                message=message)


AFF_NOW = " (pod affinity as it is now)"
DEV_FIXTURE = dict(
    {key: v for key, v in k.FIXTURE.items() if key != "expected"}, name="kat_headroom_dev",
    expected={"limit": LIMIT, "task_room": [
        row("t-sel", 3, False, 3, 2, 2, 1, 1, "n04", 2, 0, False,
            "needs 3 more; room for 2 now, 2 more on releasing resources (2 nodes)"),
        row("t-gpu", 1, False, 3, 0, 0, 0, 0, None, 0, 0, False,
            "needs 1 more; room for 0 now, 0 more on releasing resources (0 nodes)"),
        row("t-be", 30, True, 3, 24, 0, 3, 0, "n04", 8, 3, False,
            "needs 30 more; room for 24 now, 0 more on releasing resources (3 nodes), lower bound"),
    ]})

HOST_FIXTURE = dict(
    {key: v for key, v in k.HOST_FIXTURE.items() if key != "expected"}, name="kat_headroom",
    expected={"limit": LIMIT, "task_room": [
        row("h-port", 4, False, 3, 3, 0, 3, 0, "m1", 1, 0, True,
            "needs 4 more; room for 3 now, 0 more on releasing resources (3 nodes)" + AFF_NOW),
        row("h-aff", 6, False, 2, 9, 0, 2, 0, "m0", 5, 0, True,
            "needs 6 more; room for 9 now, 0 more on releasing resources (2 nodes)" + AFF_NOW),
        row("h-anti", 6, False, 3, 14, 0, 3, 0, "m0", 5, 0, True,
            "needs 6 more; room for 14 now, 0 more on releasing resources (3 nodes)" + AFF_NOW),
        row("h-big", 1, False, 2, 0, 0, 0, 0, None, 0, 0, True,
            "needs 1 more; room for 0 now, 0 more on releasing resources (0 nodes)" + AFF_NOW),
    ]})


def main():
    for fx in (DEV_FIXTURE, HOST_FIXTURE):
        with open(os.path.join(HERE, fx["name"] + ".json"), "w") as f:
            json.dump(fx, f, indent=1)
            f.write("\n")
        print(f"wrote {fx['name']}.json")


if __name__ == "__main__":
    main()
