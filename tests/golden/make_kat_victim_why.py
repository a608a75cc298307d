"""Hand-derived known-answer fixture for kbg_victim_reasons
(tests/golden/kat_victim_why.json, checked by tests/test_victim_why_gpu.py).
Every expected number below was derived by reading the cited reference code,
not by running any implementation.

Run: python tests/golden/make_kat_victim_why.py

The session. One tier [gang, drf, proportion, predicates], so preempt consults
gang and drf, reclaim consults gang and proportion (gang.go:104-127,
drf.go:80-107, proportion.go:161-186; one tier: session_plugins.go:59-140).
The only action is backfill, which places nothing here (no Pending task is
BestEffort, backfill.go:45-48): the state the calls describe is the state at
open.

Nodes n00..n13: 5 CPUs and 16Gi each, n04 and n13 10 CPUs, so drf's and
proportion's total is (80000 m, 224Gi, 0 GPU). role=w everywhere but n01.
Queues qa (weight 7) and qb (weight 1).

proportion's deserved (proportion.go:102-144), first round: qb is offered
total / 8 = (10000, 28Gi, 0). Its request is its Running tasks' (13000, 0, 0),
no memory: 28Gi is not LessEqual 0, so deserved = Min = (10000, 0, 0) and qb is
met. qa is offered (70000, 196Gi, 0) against a request of (8750, 1Gi, 1000):
deserved = Min = (8750, 1Gi, 0), met; allocated is (5750, 0, 0), so qa is not
Overused (8750 is not LessEqual 5750). A reclaimee of qb is kept by proportion
when (10000, 0, 0) LessEqual (13000 - what the node's reclaimees before it and
itself ask): one or two 1-CPU tasks are (12000, 11000: kept), a 4-CPU task is
not (9000).

Jobs of qb, all Running, CPU only:
  B1 minMember 1, ready 5 (gang keeps: 1 <= 5 - 1): b1a n00, b1b n06, b1c and b1d n07 (1 CPU each), b1e n12 (4 CPUs)
  B3 minMember 2, ready 2 (gang drops: 2 <= 1 is false): b3a n10 (4 CPUs), b3b n11 (1 CPU)
Jobs of qa:
  P  Pending p0: 2 CPUs, 1Gi, 1 GPU, nodeSelector role=w    (the reclaimer below)
  R  Pending r0: 1 CPU, no selector                          (the preemptor below)
  A1 minMember 1, ready 2 (gang keeps): a1a n05, a1b n07, 1 CPU each; drf: allocated 2000
  A2 minMember 2, ready 2 (gang drops): a2a n08, a2b n09, 1 CPU each; drf: allocated 2000
  A3 minMember 1, ready 2 (gang keeps): a3a n10, a3b n11, 500 m each; drf: allocated 1000
  A4 minMember 3, ready 3 (gang drops): a4a n12, a4b and a4c n13, 250 m each; drf: allocated 750

RECLAIM for P (reclaim.go:112-150; reclaimees are the Running tasks of other
queues, i.e. qb's; PredicateFn first, predicates.go:121-201):
  n00  pods: 1, holds b1a                      MaxTaskNum <= len(pods)          POD_CAP
  n01  role=x, unschedulable                   the selector fails first         SELECTOR
  n02  unschedulable and tainted               unschedulable before taints      UNSCHEDULABLE
  n03  tainted (NoSchedule), p0 tolerates none                                   TAINTS
  n04  empty                                                                     NO_PREEMPTEES
  n05  a1a only (qa, the reclaimer's queue)                                      NO_PREEMPTEES
  n06  b1b: gang keeps, proportion keeps (12000); (1000, 0, 0) is Less than
       (2000, 1Gi, 1000) in all three dimensions (reclaim.go:137-143)            NOT_ENOUGH
  n07  b1c, b1d (a1b is qa's): both kept; (2000, 0, 0) is not Less in CPU        VICTIMS
  n08, n09  a2a / a2b only (qa)                                                  NO_PREEMPTEES
  n10  b3a: gang drops, proportion drops (9000)     NO_VICTIMS, gang and proportion empty
  n11  b3b: gang drops, proportion keeps (12000)    NO_VICTIMS, gang empty
  n12  b1e: gang keeps, proportion drops (9000)     NO_VICTIMS, proportion empty
  n13  a4b, a4c only (qa)                                                        NO_PREEMPTEES
  count      cap 1, selector 1, unschedulable 1, taints 1, no_preemptees 5, no_victims 3, not_enough 1, victims 1
  fn_empty   gang 2 (n10, n11), drf 0 (not a reclaimable fn), proportion 2 (n10, n12)

PREEMPT_JOBS for R (preempt.go:181-202; preemptees are the Running tasks of
the other jobs of qa). drf.go:80-105: ls = share of R's allocated (0) plus r0
= 1000 / 80000 = 1/80; a preemptee is kept when its job's share after the
subtraction is not below ls by more than 1e-6:
  n00  POD_CAP;  n01, n02 unschedulable (r0 has no selector)  UNSCHEDULABLE;  n03  TAINTS
  n04  empty; n06 holds b1b only (qb)                                            NO_PREEMPTEES
  n05  a1a: gang keeps; A1 2000 - 1000 = 1000, share 1/80 = ls: kept;
       (1000, 0, 0) is not Less than (1000, 0, 0)                                VICTIMS
  n07  a1b: the same                                                             VICTIMS
  n08, n09  a2a / a2b: gang drops; A2's share after is 1/80: drf keeps      NO_VICTIMS, gang empty
  n10, n11  a3a / a3b: gang keeps; A3 1000 - 500 = 500, share 1/160 < ls    NO_VICTIMS, drf empty
  n12  a4a: gang drops; A4 750 - 250 = 500: drf drops                       NO_VICTIMS, gang and drf empty
  n13  a4b, a4c: gang drops both; 500 and 250: drf drops both               NO_VICTIMS, gang and drf empty
  count      cap 1, unschedulable 2, taints 1, no_preemptees 2, no_victims 6, victims 2
  fn_empty   gang 4 (n08, n09, n12, n13), drf 4 (n10..n13), proportion 0
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
TAINT = [{"key": "dedicated", "value": "x", "effect": "NoSchedule"}]


def node(i, cpu="5", pods="110", role="w", **kw):
    n = {"name": f"n{i:02d}", "allocatable": {"cpu": cpu, "memory": "16Gi", "pods": pods}, "labels": {"role": role}}
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


def cpu(m):
    return {"cpu": f"{m}m"}


FIXTURE = {
    "name": "kat_victim_why",
    "actions": ["backfill"],
    "tiers": [[{"name": "gang"}, {"name": "drf"}, {"name": "proportion"}, {"name": "predicates"}]],
    "nodes": [node(0, pods="1"), node(1, role="x", unschedulable=True), node(2, unschedulable=True, taints=TAINT),
              node(3, taints=TAINT), node(4, cpu="10"), node(5), node(6), node(7), node(8), node(9), node(10),
              node(11), node(12), node(13, cpu="10")],
    "queues": [{"name": "qa", "weight": 7}, {"name": "qb", "weight": 1}],
    "podGroups": [pg("P", 1, "qa", 100), pg("R", 1, "qa", 101), pg("A1", 1, "qa", 1), pg("A2", 2, "qa", 2),
                  pg("A3", 1, "qa", 3), pg("A4", 3, "qa", 4), pg("B1", 1, "qb", 5), pg("B3", 2, "qb", 6)],
    "pods": [
        pod("p0", "P", {"cpu": "2", "memory": "1Gi", "nvidia.com/gpu": "1"}, nodeSelector={"role": "w"}),
        pod("r0", "R", cpu(1000)),
        pod("a1a", "A1", cpu(1000), "n05"), pod("a1b", "A1", cpu(1000), "n07"),
        pod("a2a", "A2", cpu(1000), "n08"), pod("a2b", "A2", cpu(1000), "n09"),
        pod("a3a", "A3", cpu(500), "n10"), pod("a3b", "A3", cpu(500), "n11"),
        pod("a4a", "A4", cpu(250), "n12"), pod("a4b", "A4", cpu(250), "n13"), pod("a4c", "A4", cpu(250), "n13"),
        pod("b1a", "B1", cpu(1000), "n00"), pod("b1b", "B1", cpu(1000), "n06"), pod("b1c", "B1", cpu(1000), "n07"),
        pod("b1d", "B1", cpu(1000), "n07"), pod("b1e", "B1", cpu(4000), "n12"),
        pod("b3a", "B3", cpu(4000), "n10"), pod("b3b", "B3", cpu(1000), "n11"),
    ],
    "expected": {
        "decisions": [], "evictions": [],
        # kbg_victim_reasons after the action: (mode, job uid) -> row; causes in KBG_WHY_* / KBG_VWHY_* order
        "victim_why": [
            {"mode": "reclaim", "job": "ns/P", "task": "p0", "queue_overused": 0,
             "count": [1, 1, 0, 1, 1, 0, 5, 3, 1, 1, 0],
             "first_node": ["n00", "n01", None, "n02", "n03", None, "n04", "n10", "n06", "n07", None],
             "fn_empty": [2, 0, 2]},
            {"mode": "preempt_jobs", "job": "ns/R", "task": "r0", "queue_overused": 0,
             "count": [1, 0, 0, 2, 1, 0, 2, 6, 0, 2, 0],
             "first_node": ["n00", None, None, "n01", "n03", None, "n04", "n08", None, "n05", None],
             "fn_empty": [4, 4, 0]},
        ],
    },
}


def main():
    with open(os.path.join(HERE, "kat_victim_why.json"), "w") as f:
        json.dump(FIXTURE, f, indent=1)
        f.write("\n")
    print("wrote kat_victim_why.json")


if __name__ == "__main__":
    main()
