"""Hand-derived known-answer fixture for kbg_node_reasons
(tests/golden/kat_node_why.json, checked by tests/test_hostsim_node_why.py and
tests/test_node_why_gpu.py). Every expected number below was derived by
reading the cited reference code, not by running any implementation.

Run: python tests/golden/make_kat_node_why.py

The cluster is kat_task_why_host's (tests/golden/make_kat_task_why.py) with a
nil Node and a BestEffort pod: host ports, pod affinity and a nil Node are the
causes only the host path names (2, 5 and 9). The session is described as it
is at open. One tier [gang, drf, proportion, predicates]. Queue qb holds the
Running job X, queue qa the Pending job P: qa has allocated nothing and
deserves something, so it is not Overused (proportion.go:188-194) and every
pod of cause 6 or 7 is an open one.

Nodes m0..m3: 5 CPUs, 16Gi; m0 and m1 in zone a, m2 and m3 in zone b; label
host = the node's name.
  m0  w0 Running, 1000m, labels app=web, hostPort 8080/TCP   Idle (4000, 16Gi, 0)
  m1  empty                                                  Idle (5000, 16Gi, 0)
  m2  d0 Running, 1000m, labels app=db                       Idle (4000, 16Gi, 0)
  m3  empty                                                  Idle (5000, 16Gi, 0)
  ""  g0, Succeeded, names the node `ghost`, which no Node object describes:
      the cache makes a NodeInfo with a nil Node and the name "" for it and,
      the pod being over, puts no task on it (event_handlers.go:49-58). (A
      pod that still runs there would fail every node for every pod.)
All pods are in namespace ns, so every term selects within it (vendor
predicates.go:1155-1466); only pods with a node count, and g0 has no label.

The Pending pods of P, five of them on every node:
  h-port  1000m, hostPort 8080/TCP
  h-aff   1000m, required podAffinity app=web over the zone
  h-anti  1000m, required podAntiAffinity app=db over the host
  h-big   10 CPUs, required podAntiAffinity app=web over the zone
  h-be    no requests, Resreq.IsEmpty(): backfill's pod, predicates only (backfill.go:47-60)

m0: h-port meets the port w0 holds: HOST_PORTS (predicates.go:143-155). h-aff:
  w0 is in zone a, it passes, 1000 < 4000: FITS_IDLE. h-anti: no app=db pod on
  host m0: FITS_IDLE. h-big: w0 shares the zone: POD_AFFINITY (predicates.go:
  185-198), before any resource test. h-be: FITS_IDLE.
m1: nobody holds a port there: h-port FITS_IDLE. h-aff and h-anti as on m0.
  h-big: zone a again: POD_AFFINITY. h-be FITS_IDLE.
m2: h-port FITS_IDLE. h-aff: no app=web pod in zone b: POD_AFFINITY. h-anti:
  d0 is on this host: POD_AFFINITY. h-big: no web pod in zone b, it passes;
  10000 against Idle 4000 and Releasing 0: SHORT, FitDelta cpu 4000 - 10010 <
  0, memory and GPU not asked (resource_info.go:116-129): idle_short (1, 0, 0).
  h-be FITS_IDLE.
m3: h-port FITS_IDLE. h-aff POD_AFFINITY. h-anti: no db pod on host m3:
  FITS_IDLE. h-big SHORT of cpu (5000 - 10010 < 0). h-be FITS_IDLE.
"": a nil Node under the predicates plugin (predicates.go:122-123): PANIC for
  all five, the BestEffort pod too.

The fixture's own cycle (tests/test_oracle_golden.py runs every KAT's): allocate
places h-port, h-aff and h-anti, then h-big passes m0 and m1 (pod affinity),
m2 and m3 (short) and reaches the nil Node: the reference panics there
(predicates.go:122-123), status ref_panic."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_kat_task_why import HOST_FIXTURE, pod  # noqa: E402

AFF, PORTS = "affinity/anti-affinity failed", "didn't have available host ports"


def row(node, tasks, message, idle_short=(0, 0, 0)):
    idle = len(tasks.get("6", []))
    return dict(node=node, pending=5, tasks=tasks, idle_short=list(idle_short), open_idle=idle, open_releasing=0,
                idle_best_effort=1 if "h-be" in tasks.get("6", []) else 0, message=message)


FIXTURE = dict(
    HOST_FIXTURE, name="kat_node_why",
    pods=HOST_FIXTURE["pods"][:4] + [pod("h-be", "P", {}, labels={"app": "client"})] + HOST_FIXTURE["pods"][4:] +
    [pod("g0", "X", {"cpu": "1"}, "ghost", phase="Succeeded")],
    expected={
        "status": "ref_panic",
        # kbg_node_reasons at open; the Pending pods of each node by cause (KBG_WHY_* / KBG_TWHY_* codes)
        "node_why": [
            row("m0", {"2": ["h-port"], "5": ["h-big"], "6": ["h-aff", "h-anti", "h-be"]},
                f"takes 3 of 5 pending pods now (3 in queues that are not overused, 1 best-effort); turned away: "
                f"1 {AFF}, 1 {PORTS}"),
            row("m1", {"5": ["h-big"], "6": ["h-port", "h-aff", "h-anti", "h-be"]},
                f"takes 4 of 5 pending pods now (4 in queues that are not overused, 1 best-effort); turned away: "
                f"1 {AFF}"),
            row("m2", {"5": ["h-aff", "h-anti"], "6": ["h-port", "h-be"], "8": ["h-big"]},
                f"takes 2 of 5 pending pods now (2 in queues that are not overused, 1 best-effort); turned away: "
                f"2 {AFF}, 1 insufficient cpu", (1, 0, 0)),
            row("m3", {"5": ["h-aff"], "6": ["h-port", "h-anti", "h-be"], "8": ["h-big"]},
                f"takes 3 of 5 pending pods now (3 in queues that are not overused, 1 best-effort); turned away: "
                f"1 {AFF}, 1 insufficient cpu", (1, 0, 0)),
            row("", {"9": ["h-port", "h-aff", "h-anti", "h-big", "h-be"]},
                "takes 0 of 5 pending pods now; turned away: 5 no Node object"),
        ],
    })


def main():
    with open(os.path.join(HERE, FIXTURE["name"] + ".json"), "w") as f:
        json.dump(FIXTURE, f, indent=1)
        f.write("\n")
    print(f"wrote {FIXTURE['name']}.json")


if __name__ == "__main__":
    main()
