"""Hand-written sessions for the per-predicate unschedulable reasons
(kbg_job_reasons, include/kbgpu.h) and what they must report, shared by the
host test (tests/test_reasons_host.py, the tool library) and the device test
(tests/test_reasons_gpu.py). Every session runs the predicates plugin alone
and its PodGroups ask for more members than they have, so no job gets ready
and every evaluated job is reported. Each case's docstring derives the counts
by hand, stage codes in the reference's order (predicates.go:125-198):
0 pod cap, 1 selector / node affinity, 2 host ports, 3 unschedulable,
4 taints, 5 pod (anti)affinity."""
import copy

from helpers import load_golden

NEVER_READY = 100


def node(name, cpu="8", pods="110", labels=None, taints=None, unschedulable=False):
    n = {"name": name, "allocatable": {"cpu": cpu, "memory": "64Gi", "pods": pods}, "labels": dict(labels or {})}
    if taints:
        n["taints"] = [{"key": k, "value": v, "effect": e} for k, v, e in taints]
    if unschedulable:
        n["unschedulable"] = True
    return n


def pod(uid, cpu="1", group="pg1", node_name="", ports=None, **spec):
    p = {"uid": uid, "namespace": "ns", "name": uid, "phase": "Running" if node_name else "Pending",
         "nodeName": node_name, "containers": [{"requests": {"cpu": cpu}}],
         "annotations": {"scheduling.k8s.io/group-name": group}}
    if ports:
        p["containers"][0]["ports"] = ports
    p.update(spec)
    return p


def session(nodes, pods, groups=("pg1",), min_member=NEVER_READY):
    return {"tiers": [[{"name": "predicates"}]], "nodes": nodes, "pods": pods,
            "podGroups": [{"namespace": "ns", "name": g, "minMember": min_member, "queue": "q",
                           "creationTimestamp": 100 * i} for i, g in enumerate(groups)],
            "queues": [{"name": "q", "weight": 1}]}


def why(task, before, visited, count=None, first=None, fit_nodes=0):
    c, f = [0] * 6, [-1] * 6
    for k, v in (count or {}).items():
        c[k] = v
    for k, v in (first or {}).items():
        f[k] = v
    return {"task": task, "before": before, "visited": visited, "count": c, "first_node": f, "fit_nodes": fit_nodes}


GPU_TAINT = [("dedicated", "gpu", "NoSchedule")]


def pod_cap_alone():
    """n1 and n2 allow one pod each and hold one: t1 meets the cap on both
    (stage 0), nothing else is wrong with them. count[0] = 2, first n1 (0)."""
    fx = session([node("n1", pods="1"), node("n2", pods="1")],
                 [pod("r1", group="old", node_name="n1"), pod("r2", group="old", node_name="n2"), pod("t1")],
                 groups=("old", "pg1"))
    return fx, {"ns/pg1": why("t1", 0, 2, {0: 2}, {0: 0})}


def selector_alone():
    """t1 selects zone=c; the nodes are in a, a, b: stage 1 on all three."""
    fx = session([node("n1", labels={"zone": "a"}), node("n2", labels={"zone": "a"}), node("n3", labels={"zone": "b"})],
                 [pod("t1", nodeSelector={"zone": "c"})])
    return fx, {"ns/pg1": why("t1", 0, 3, {1: 3}, {1: 0})}


def host_ports_alone():
    """Both nodes hold a pod on 0.0.0.0:80/TCP and t1 wants host port 80
    (TCP, every address): stage 2 on both."""
    web = [{"hostPort": 80}]
    fx = session([node("n1"), node("n2")],
                 [pod("r1", group="old", node_name="n1", ports=web), pod("r2", group="old", node_name="n2", ports=web),
                  pod("t1", ports=web)], groups=("old", "pg1"))
    return fx, {"ns/pg1": why("t1", 0, 2, {2: 2}, {2: 0})}


def unschedulable_alone():
    """n1 is schedulable but too small (1 cpu for 2): a FitError entry. n2 and
    n3 are cordoned: stage 3, first n2 (1). 2 + 1 entry = 3 visited."""
    fx = session([node("n1", cpu="1"), node("n2", unschedulable=True), node("n3", unschedulable=True)],
                 [pod("t1", cpu="2")])
    return fx, {"ns/pg1": why("t1", 0, 3, {3: 2}, {3: 1}, fit_nodes=1)}


def taints_alone():
    """Both nodes carry dedicated=gpu:NoSchedule, t1 tolerates nothing: stage
    4 on both. (A PreferNoSchedule taint would not count.)"""
    fx = session([node("n1", taints=GPU_TAINT), node("n2", taints=GPU_TAINT)], [pod("t1")])
    return fx, {"ns/pg1": why("t1", 0, 2, {4: 2}, {4: 0})}


def pod_affinity_alone():
    """t1 requires a pod app=nothing in its zone; no pod carries that label and
    t1 does not match its own term (app=other): stage 5 on both nodes."""
    aff = {"podAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": {"app": "nothing"}}, "topologyKey": "zone"}]}}
    fx = session([node("n1", labels={"zone": "a"}), node("n2", labels={"zone": "b"})],
                 [pod("t1", labels={"app": "other"}, affinity=aff)])
    return fx, {"ns/pg1": why("t1", 0, 2, {5: 2}, {5: 0})}


def earlier_stage_wins():
    """t1 (2 cpu) selects zone=a and tolerates nothing.
    n0 cordoned, zone b            -> selector (1) before unschedulable (3)
    n1 full (1 of 1 pods), tainted -> pod cap (0) before taints (4)
    n2 cordoned, tainted, zone a   -> unschedulable (3) before taints (4)
    n3 tainted, zone a             -> taints (4)
    n4 zone a, 1 cpu               -> passes every stage: a FitError entry
    n5 tainted, zone b             -> selector (1)
    count = [1, 2, 0, 1, 1, 0], first = [1, 0, -, 2, 3, -]; 5 + 1 entry = 6."""
    a, b = {"zone": "a"}, {"zone": "b"}
    fx = session([node("n0", labels=b, unschedulable=True), node("n1", pods="1", labels=a, taints=GPU_TAINT),
                  node("n2", labels=a, taints=GPU_TAINT, unschedulable=True), node("n3", labels=a, taints=GPU_TAINT),
                  node("n4", cpu="1", labels=a), node("n5", labels=b, taints=GPU_TAINT)],
                 [pod("r1", group="old", node_name="n1"), pod("t1", cpu="2", nodeSelector={"zone": "a"})],
                 groups=("old", "pg1"))
    return fx, {"ns/pg1": why("t1", 0, 6, {0: 1, 1: 2, 3: 1, 4: 1}, {0: 1, 1: 0, 3: 2, 4: 3}, fit_nodes=1)}


def cap_from_this_cycle():
    """n1 allows 2 pods, n2 one; both start empty. Job pgA (first): a1 goes to
    n1, then a2 (100 cpu) fits nowhere — at that point (one decision applied)
    n1 holds 1 of 2 and n2 0 of 1, so no stage fails and both nodes are
    FitError entries, although the final table has both nodes full. Job pgB:
    b1 -> n1 (now 2 of 2), b2 -> n2 (1 of 1), b3 meets the cap on both:
    count[0] = 2 after three decisions."""
    fx = session([node("n1", pods="2"), node("n2", pods="1")],
                 [pod("a1", group="pgA"), pod("a2", cpu="100", group="pgA"),
                  pod("b1", group="pgB"), pod("b2", group="pgB"), pod("b3", group="pgB")], groups=("pgA", "pgB"))
    return fx, {"ns/pgA": why("a2", 1, 2, fit_nodes=2), "ns/pgB": why("b3", 3, 2, {0: 2}, {0: 0})}


def allocated_at_k():
    """t1 is its job's only task and is allocated to n2 after n0 (cordoned,
    stage 3) and n1 (tainted, stage 4): visited = k + 1 = 3 = 2 + the node
    that took it; no FitError entry."""
    fx = session([node("n0", unschedulable=True), node("n1", taints=GPU_TAINT), node("n2"), node("n3")], [pod("t1")])
    return fx, {"ns/pg1": why("t1", 0, 3, {3: 1, 4: 1}, {3: 0, 4: 1})}


def pipelined_at_k():
    """n0 is cordoned (stage 3). n1 (2 cpu) holds a 2-cpu pod that is being
    deleted: Idle 0, Releasing 2, so t1 (1 cpu) does not fit Idle — a FitError
    entry — and is pipelined there: visited = k + 1 = 2 = 1 + that entry."""
    fx = session([node("n0", unschedulable=True), node("n1", cpu="2"), node("n2")],
                 [pod("r1", cpu="2", group="old", node_name="n1", deletionTimestamp="2026-01-01T00:00:00Z"), pod("t1")],
                 groups=("old", "pg1"))
    return fx, {"ns/pg1": why("t1", 0, 2, {3: 1}, {3: 0}, fit_nodes=1)}


def _kat(name, keep=None, drop=()):
    fx = copy.deepcopy(load_golden(name + ".json"))
    fx.pop("expected", None)
    for pg in fx["podGroups"]:
        pg["minMember"] = NEVER_READY
    fx["pods"] = [p for p in fx["pods"] if (keep is None or p["uid"] in keep) and p["uid"] not in drop]
    return fx


def kat_host_ports_upto_e():
    """kat_host_ports without its last two pods. a, c, d land on n1, b on n2;
    e wants 10.0.0.1:53/UDP: n1 holds c on the same triple and n2 holds dns on
    0.0.0.0:53/UDP, both conflicts (stage 2); n3 takes it: visited 3."""
    fx = _kat("kat_host_ports", drop=("f", "g"))
    return fx, {"ns/pg1": why("e", 4, 3, {2: 2}, {2: 0})}


def kat_pod_affinity_errors_upto_y1():
    """kat_pod_affinity_errors without z1: x1's anti-affinity term has an
    invalid operator and y1's affinity term an empty topology key; both make
    the predicate return an error on the only node. y1 is the job's last
    evaluated task: the error counts under stage 5. (pg0's pod is Running: it
    is never evaluated, valid = 0.)"""
    fx = _kat("kat_pod_affinity_errors", drop=("z1",))
    return fx, {"ns/pg1": why("y1", 0, 1, {5: 1}, {5: 0}), "ns/pg0": None}


def kat_pod_affinity_errors():
    """The whole fixture: z1 (no terms) is evaluated last and allocated to n1:
    visited 1, nothing failed."""
    fx = _kat("kat_pod_affinity_errors")
    return fx, {"ns/pg1": why("z1", 0, 1), "ns/pg0": None}


def kat_pod_affinity_first_pod():
    """a1 (first pod of its group, matches its own term) took n1's only cpu.
    a2 needs a pod app=cache in its zone: n1 (zone a, holds a1) passes and
    lacks cpu — a FitError entry; n2 (zone b) fails the affinity (stage 5,
    first 1); n3 (zone a) takes it: 1 + 1 + 1 = 3. c1 needs app=nothing and
    does not match its own term: stage 5 on all three nodes."""
    fx = _kat("kat_pod_affinity_first_pod")
    return fx, {"ns/pg1": why("a2", 1, 3, {5: 1}, {5: 1}, fit_nodes=1), "ns/pg2": why("c1", 2, 3, {5: 3}, {5: 0})}


def kat_pod_anti_affinity_spread():
    """s1, s2, s3 repel app=spread per hostname on two nodes: s1 -> n1,
    s2 -> n2, and s3 finds one of them on each node: stage 5 twice."""
    fx = _kat("kat_pod_anti_affinity_spread")
    return fx, {"ns/pg1": why("s3", 2, 2, {5: 2}, {5: 0})}


CASES = {f.__name__: f for f in (
    pod_cap_alone, selector_alone, host_ports_alone, unschedulable_alone, taints_alone, pod_affinity_alone,
    earlier_stage_wins, cap_from_this_cycle, allocated_at_k, pipelined_at_k, kat_host_ports_upto_e,
    kat_pod_affinity_errors_upto_y1, kat_pod_affinity_errors, kat_pod_affinity_first_pod, kat_pod_anti_affinity_spread)}
# Sessions with inter-pod (anti)affinity need a device session's cycle (the
# device-less cycle of the tool library declines them): the device test runs them.
AFFINITY_CASES = ("pod_affinity_alone", "kat_pod_affinity_errors_upto_y1", "kat_pod_affinity_errors",
                  "kat_pod_affinity_first_pod", "kat_pod_anti_affinity_spread")
HOST_CASES = [c for c in CASES if c not in AFFINITY_CASES]

# seeds of synth.random_fixture / contended_fixture whose S0 opens (verified by
# the host test: none may skip); the first 20 also run on the device
RANDOM_SEEDS = [21000, 21001, 21002, 21006, 21007, 21008, 21009, 21010, 21011, 21012, 21014, 21016, 21017, 21018,
                21019, 21021, 21022, 21023, 21024, 21025, 21026, 21028, 21029, 21030, 21033, 21034, 21035, 21036]
CONTENDED_SEEDS = list(range(500, 512))
SEEDS = [("random", s) for s in RANDOM_SEEDS] + [("contended", s) for s in CONTENDED_SEEDS]
# on the device: 20 of them, and contended sessions with pod (anti)affinity for the invariant
DEVICE_SEEDS = SEEDS[:14] + SEEDS[-6:]
AFFINITY_SEEDS = [("affinity", s) for s in (500, 502, 504, 506, 508, 510)]


def seeded_fixture(kind, seed):
    """Allocate only, and every job asks for more members than it has, so each
    evaluated job is reported."""
    from kbgpu import synth
    if kind == "random":
        fx = synth.random_fixture(seed)
    else:
        fx = synth.contended_fixture(seed, ports=0.3, aff=0.4 if kind == "affinity" else 0.0)
    fx = copy.deepcopy(fx)
    fx["actions"] = ["allocate"]
    for pg in fx["podGroups"]:
        pg["minMember"] = NEVER_READY
    return fx


def check_job(got, want, task_uid, fit_nodes):
    """got: kbg_job_reasons; want: a why() row or None (valid == 0)."""
    if want is None:
        assert got.valid == 0
        return
    assert got.valid == 1
    row = {"task": task_uid, "before": got.before, "visited": got.visited, "count": list(got.count),
           "first_node": list(got.first_node), "fit_nodes": fit_nodes}
    assert row == want
    assert list(got.reserved) == [0, 0]
