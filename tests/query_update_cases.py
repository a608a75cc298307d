"""The cases of the query-after-update tests (tests/query_update_session.py):
name -> (family, fixture S0, one change-list builder per update, flags). A
builder takes (session or view, the fixture after the rounds before) and reads
only what a session and a Python view of the cache both have (job, queue and
task uids), so tests/test_query_update_ref.py builds the same batches without
a library.

Families: `structural` (the session is rebuilt and renumbered), `in_place`
(JOB_UPDATE / QUEUE_SET and pod churn: nothing rebuilt, nothing renumbered),
`recompile` (NODE_SET: the static tables and the stage planes are rebuilt in
place) and `chain` (one session through all three and pod churn).

Every fixture has at most 70 nodes and 10 jobs of 6 tasks. The seeds were
picked on the CPU with the oracle and the hostsim library: S0 and S1 run every
action prefix "ok", the library takes the batch, a fixture can say S1, Pending
tasks are left before the first action and after the last, and some row of the
four older calls and of each of kbg_job_fit, kbg_node_reasons and
kbg_node_drain differs from the warm-up's (tests/test_query_update_ref.py)."""
import copy

import update_events as ue
from kbgpu import synth

GROUP = "scheduling.k8s.io/group-name"
ACTIONS = ["reclaim", "allocate", "backfill", "preempt"]


def seeded_fixture(kind, seed):
    if kind == "random":
        fx = synth.random_fixture(seed, max_nodes=16, max_jobs=8, max_tasks=6)
    elif kind == "contended":
        fx = synth.contended_fixture(seed)  # (8 nodes, 8 jobs of 6 tasks, 3 queues)
    elif kind == "ports":
        fx = synth.contended_fixture(seed, ports=0.3)
    else:
        fx = synth.contended_fixture(seed, aff=0.4, ports=0.2)
    return dict(fx, actions=list(ACTIONS) if kind != "random" else list(fx.get("actions") or ["allocate"]))


def _uids(s):
    return {t.uid for t in s.flat.task_objs if t is not None}


def structural_of(fx0, seed):
    return lambda s, fx: synth.structural(fx0, seed, {j.uid for j in s.jobs}, _uids(s), [q.uid for q in s.queues])


def fixed(changes):
    return lambda s, fx: copy.deepcopy(changes)


# ------------------------------------------------------------------ hand-made
def _pod(uid, group, cpu, node="", **spec):
    return dict({"uid": uid, "namespace": "ns", "name": uid, "phase": "Running" if node else "Pending",
                 "nodeName": node, "annotations": {GROUP: group}, "containers": [{"requests": {"cpu": cpu}}]}, **spec)


def _pg(name, queue, min_member=1, created=0):
    return {"namespace": "ns", "name": name, "minMember": min_member, "queue": queue,
            "creationTimestamp": created * 10 ** 9}


def _node(i, cpu="2", **kw):
    return dict({"name": f"n{i:03d}", "allocatable": {"cpu": cpu, "memory": "8Gi", "pods": "110"},
                 "labels": {"zone": "ab"[i % 2]}}, **kw)


# the spec of `run`'s pods: the session holds it (every task's spec is marshalled) and compiles no class for it
RUN_SPEC = {"tolerations": [{"key": "batch", "operator": "Exists", "effect": "NoSchedule"}]}


def hand_cluster(n_nodes):
    """`n_nodes` 2-CPU nodes in zones a and b, n003 tainted, n005 cordoned.
    Queue q1: `run` holds a 1-CPU Running pod on every fourth node, with a
    toleration no Pending pod carries (a spec without a predicate class), `big` asks
    3 CPUs twice (short everywhere), `sel` wants zone c (no node). Queue q2:
    `fill` has 4 Pending 1-CPU pods that are placed, `own` 2 Pending pods that
    want zone b and tolerate the taint. After any cycle `big` and `sel` stay
    Pending: the rows of the query calls speak of them. The oracle's preempt
    panics on this cluster (a Resource.Sub underflow of the reference), so the
    cycle is allocate and backfill."""
    nodes = [_node(i) for i in range(n_nodes)]
    nodes[3]["taints"] = [{"key": "dedicated", "value": "x", "effect": "NoSchedule"}]
    nodes[5]["unschedulable"] = True
    pods = [_pod(f"run-{i:03d}", "run", "1", nodes[i]["name"], tolerations=RUN_SPEC["tolerations"])
            for i in range(1, n_nodes, 4)][:6]
    pods += [_pod(f"big-{k}", "big", "3") for k in range(2)]
    pods += [_pod(f"sel-{k}", "sel", "1", nodeSelector={"zone": "c"}) for k in range(2)]
    pods += [_pod(f"fill-{k}", "fill", "1") for k in range(4)]
    pods += [_pod(f"own-{k}", "own", "500m", nodeSelector={"zone": "b"},
                  tolerations=[{"key": "dedicated", "operator": "Exists", "effect": "NoSchedule"}]) for k in range(2)]
    groups = [_pg("run", "q1"), _pg("big", "q1", 2, 1), _pg("sel", "q1", 1, 2), _pg("fill", "q2", 1, 3),
              _pg("own", "q2", 1, 4)]
    return {"name": f"hand-{n_nodes}", "tiers": None, "nodes": nodes, "pods": pods, "podGroups": groups,
            "queues": [{"name": "q1", "weight": 1}, {"name": "q2", "weight": 1}], "actions": ["allocate", "backfill"]}


def w_grows():
    """63 -> 65 nodes: the node words W go 1 -> 2. The new nodes have 4 CPUs: `big` fits them (n063 first)."""
    fx = hand_cluster(63)
    return fx, [fixed([("node_add", _node(63, "4")), ("node_add", _node(64, "4"))])], {}


def w_shrinks():
    """65 -> 64 nodes by deleting n000 (it holds no pod): W goes 2 -> 1 and
    every later node's index moves. n000 was the first node of `big`'s
    insufficient-resources cause and of `sel`'s selector cause."""
    fx = hand_cluster(65)
    return fx, [fixed([("node_delete", copy.deepcopy(fx["nodes"][0]))])], {}


def queue_delete_first_holder():
    """Queue q1 goes with `run`, `big` and `sel`: the tasks whose rows held the
    lowest first nodes of the warm-up leave, the tasks and jobs of q2 are
    renumbered, and a new job of zone-c pods joins q2 in the same batch."""
    fx = hand_cluster(12)
    new = [("pod_group_add", _pg("late", "q2", 1, 9))] + \
          [("pod_add", _pod(f"late-{k}", "late", "1", nodeSelector={"zone": "c"})) for k in range(2)]
    return fx, [fixed([("queue_delete", {"name": "q1"})] + new)], {}


def pod_group_add_new_class():
    """A PodGroup whose Pending pods carry `run`'s spec, which only Running
    pods had: the static predicate had no class for it, so the update
    recompiles with one more class and the stage planes get larger."""
    fx = hand_cluster(12)
    new = [("pod_group_add", _pg("wide", "q2", 1, 9))] + \
          [("pod_add", _pod(f"wide-{k}", "wide", "2500m", **RUN_SPEC)) for k in range(3)]
    return fx, [fixed(new)], {}


def queue_add_starves():
    """A new queue of weight 8 with a job that asks 16 of the 24 CPUs: queue
    q1's deserved share falls under what `run` holds, so queue_overused turns
    true for the Pending tasks of `big` and `sel`."""
    fx = hand_cluster(12)
    new = [("queue_add", {"name": "q3", "weight": 8}), ("pod_group_add", _pg("hog", "q3", 1, 9))] + \
          [("pod_add", _pod(f"hog-{k}", "hog", "2")) for k in range(8)]
    return fx, [fixed(new)], {}


def regrow_keys():
    """pod_add alone (in place): three new Pending pods of `big`, `sel` and
    `own` with requests no task had, so the Pending tasks hold more distinct
    (class, request) keys than at the warm-up and the query buffers regrow on
    the live session."""
    fx = hand_cluster(12)
    own = next(p for p in fx["pods"] if p["uid"] == "own-0")
    new = [dict(copy.deepcopy(own), uid=f"own-x{k}", name=f"own-x{k}", containers=[{"requests": {"cpu": cpu}}])
           for k, cpu in enumerate(("2500m", "2750m", "3250m"))]
    new.append(_pod("big-x", "big", "5"))
    new.append(_pod("sel-x", "sel", "1500m", nodeSelector={"zone": "c"}))
    return fx, [fixed([("pod_add", p) for p in new])], {}


def staged_after_preempt(seed=1):
    """A batch sent right after a cycle that ended in preempt and was not
    asked, without a reset: the deltas its evictions staged are still to push
    when the update arrives."""
    fx = seeded_fixture("contended", seed)
    return fx, [lambda s, fx_now: ue.fuzz_changes(fx_now, 2 * seed + 1, s)], {"staged": True}


def relabel_hand():
    """n004 is cordoned, n007 moves to zone c and n003 loses its taint: `sel`
    now passes n007 (short no longer: it fits), `big`'s nodes move between the
    unschedulable, taint and resource causes."""
    fx = hand_cluster(12)
    n4, n7, n3 = (copy.deepcopy(fx["nodes"][i]) for i in (4, 7, 3))
    n4["unschedulable"] = True
    n7["labels"]["zone"] = "c"
    n3["taints"] = []
    return fx, [fixed([("node_update", n4), ("node_update", n7), ("node_update", n3)])], {}


def relabel_twice():
    """Two recompiles in a row on one session: the second undoes half of the first."""
    fx, (first,), _ = relabel_hand()
    n7, n9 = copy.deepcopy(fx["nodes"][7]), copy.deepcopy(fx["nodes"][9])
    n7["labels"]["zone"] = "b"
    n9["taints"] = [{"key": "maint", "value": "", "effect": "NoSchedule"}]
    return fx, [first, fixed([("node_update", n7), ("node_update", n9)])], {}


def earlier_stage_wins():
    """tests/reasons_cases.py's session: n4 is cordoned and n5 moves to zone a (tests/test_reasons_gpu.py)."""
    import reasons_cases as rc
    fx, _ = rc.earlier_stage_wins()
    fx2 = copy.deepcopy(fx)
    fx2["nodes"][4]["unschedulable"] = True
    fx2["nodes"][5]["labels"]["zone"] = "a"
    return fx, [fixed([("node_update", fx2["nodes"][4]), ("node_update", fx2["nodes"][5])])], {}


def relabel_seeded(seed):
    """test_update_node_relabel's batch on a small random fixture."""
    import random
    fx0 = seeded_fixture("random", 6000 + seed)

    def changes(s, fx):
        rng = random.Random(seed)
        out = []
        nodes = copy.deepcopy(fx["nodes"])
        for n in rng.sample(nodes, min(3, len(nodes))):
            labels = dict(n.get("labels") or {})
            if labels and rng.random() < 0.5:
                labels.pop(rng.choice(sorted(labels)))
            labels[rng.choice(["zone", "disk", "tier"])] = rng.choice(["a", "b", "ssd", "x"])
            n["labels"] = labels
            if rng.random() < 0.5:
                n["taints"] = list(n.get("taints") or []) + [{"key": "maint", "value": "", "effect": "NoSchedule"}]
            elif n.get("taints"):
                n["taints"] = []
            out.append(("node_update", n))
        return out
    return fx0, [changes], {}


def in_place_case(name):
    """A case of update_events.IN_PLACE with the four actions."""
    fx0, rounds = ue.CASES[name]()
    # two pods no node can hold, of a job of their own: Pending tasks are left whatever the cycle does
    fx0 = dict(fx0, tiers=None, actions=list(ACTIONS),
               podGroups=fx0["podGroups"] + [ue._pg("qb", "pgz", "qb", created=9)],
               pods=fx0["pods"] + [ue._pod(f"z{k}", "qb", "pgz", cpu="64") for k in (1, 2)])
    if name in ("min_member_up", "min_member_down", "pod_group_add_again"):
        # the gang runs, with a third pod on a third node: whether its pods may be evicted for the pods of
        # queue qb is the gang plugin's answer (MinAvailable against the 3 ready tasks), which the event changes
        a1, a2 = fx0["pods"][:2]
        fx0["nodes"] = fx0["nodes"] + ue._nodes(3, 1)[2:]
        fx0["pods"] = [dict(a1, phase="Running", nodeName="n1"), dict(a2, phase="Running", nodeName="n2"),
                       ue._pod("a3", "qa", "pga", phase="Running", node="n3")] + fx0["pods"][2:]
    if name == "pdb_add":  # two pods of the job run: the PDB's MinAvailable 5 keeps them from queue qb's reclaim
        fx0["pods"] = [dict(p, phase="Running", nodeName="n1") for p in fx0["pods"][:2]] + fx0["pods"][2:]
    if name in ("min_member_up", "min_member_down", "pod_group_add_again", "pdb_add"):
        # (the oracle's reclaim panics once the gang gives its pods up, a Resource.Sub underflow of the reference)
        fx0["actions"] = ["allocate", "backfill"]
    return fx0, [fixed(ch) for ch in rounds], {}


def fuzz_in_place(seed):
    """update_events.fuzz_changes, odd seeds: JOB_UPDATE / QUEUE_SET beside pod churn and node updates."""
    assert seed % 2
    fx0 = dict(ue.fuzz_fixture(seed))
    return fx0, [lambda s, fx: ue.fuzz_changes(fx, seed, s)], {}


def seeded_structural(kind, seed):
    fx0 = seeded_fixture(kind, seed)
    return fx0, [structural_of(fx0, seed)], {}


def chain(seed):
    """structural -> in place -> relabel -> churn on one session."""
    fx0 = dict(synth.contended_fixture(seed, nodes=6, jobs=5, tasks=4), actions=list(ACTIONS))
    # an empty node ahead of the others, deleted by the structural round: every node's index moves
    spare = dict(copy.deepcopy(fx0["nodes"][0]), name="m-spare")
    fx0["nodes"] = [spare] + fx0["nodes"]

    def structural(s, fx):
        ch = [c for c in structural_of(fx0, seed)(s, fx) if c[1].get("name") != "m-spare"]
        return ch + [("node_delete", copy.deepcopy(spare))]

    def in_place(s, fx):
        groups = {f"{g.get('namespace', '')}/{g['name']}": g for g in fx["podGroups"]}
        jobs = sorted(j.uid for j in s.jobs if j.uid in groups)
        queues = [q.uid for q in s.queues]
        out = [("pod_group_update", dict(groups[jobs[0]], minMember=groups[jobs[0]]["minMember"] + 2)),
               ("queue_add", {"name": queues[-1], "weight": 3})]
        if len(queues) > 1:
            g = groups[jobs[-1]]
            out.append(("pod_group_update", dict(g, queue=next(q for q in queues if q != g["queue"]))))
        return out

    def relabel(s, fx):
        # a node a Pending pod's selector turned away takes the selector's labels and a taint (the pod goes
        # from the selector stage to the taint stage there), a second node is cordoned, a third changes zone
        nodes = copy.deepcopy(fx["nodes"])
        free = [n for n in nodes if not n.get("taints") and not n.get("unschedulable")]
        sel = next((p["nodeSelector"] for p in fx["pods"] if p["phase"] == "Pending" and p.get("nodeSelector")), {})
        first = next((n for n in free if any((n.get("labels") or {}).get(k) != v for k, v in sel.items())), free[0])
        first["labels"] = dict(first.get("labels") or {}, **sel)
        first["taints"] = [{"key": "maint", "value": "", "effect": "NoSchedule"}]
        rest = [n for n in free if n is not first][:2]
        rest[0]["unschedulable"] = True
        rest[1]["labels"] = dict(rest[1].get("labels") or {}, zone="zz")
        return [("node_update", n) for n in [first] + rest]

    def churn(s, fx):
        return synth.churn(fx, seed, _uids(s), done=0.2, delete=0.05, add=0.05, node_frac=0.1)[0]
    return fx0, [structural, in_place, relabel, churn], {}


STRUCTURAL_SEEDS = {"random": (15, 17, 24, 34), "contended": (1, 6, 35, 72), "ports": (1, 13, 28, 35),
                    "affinity": (1, 13, 35, 56)}
FUZZ_SEEDS = (1, 15, 23, 27, 45, 59)
RELABEL_SEEDS = (4, 5, 8, 18)
CHAIN_SEEDS = (13, 108, 167, 235)  # (235: the node its structural round adds takes a kbg_job_fit or kbg_node_drain place)

HAND = {"structural": (w_grows, w_shrinks, queue_delete_first_holder, pod_group_add_new_class,
                       queue_add_starves),
        "in_place": (regrow_keys, staged_after_preempt),
        "recompile": (relabel_hand, relabel_twice, earlier_stage_wins)}


def all_cases():
    """{case id: (family, builder)}; a builder returns (fx0, rounds_of, flags)."""
    out = {}
    for fam, fns in HAND.items():
        for fn in fns:
            out[f"{fam}/{fn.__name__}"] = (fam, fn)
    for kind, seeds in STRUCTURAL_SEEDS.items():
        for s in seeds:
            out[f"structural/{kind}{s}"] = ("structural", lambda kind=kind, s=s: seeded_structural(kind, s))
    for name in ue.IN_PLACE:
        out[f"in_place/{name}"] = ("in_place", lambda name=name: in_place_case(name))
    for s in FUZZ_SEEDS:
        out[f"in_place/fuzz{s}"] = ("in_place", lambda s=s: fuzz_in_place(s))
    for s in RELABEL_SEEDS:
        out[f"recompile/relabel{s}"] = ("recompile", lambda s=s: relabel_seeded(s))
    for s in CHAIN_SEEDS:
        out[f"chain/contended{s}"] = ("chain", lambda s=s: chain(s))
    return out
