"""Update events of resident sessions (include/kbgpu.h KBG_EV_JOB_UPDATE,
KBG_EV_QUEUE_SET, KBG_EV_QUEUE_UPDATE; PodGroup, PDB, Queue and namespace
handlers of event_handlers.go:344-494,635-755): the hand-written cases, the
fuzz generator and the replay helpers shared by tests/test_update_events_host.py
(CPU, through the tool library) and tests/test_update_events_gpu.py.

The generator lives here and not in kbgpu/synth.py: the bench's fixtures stay
byte-identical."""
import copy
import random

GROUP = "scheduling.k8s.io/group-name"

_HANDLER = {"node_add": "add_node", "node_update": "update_node", "node_delete": "delete_node",
            "pod_group_add": "add_pod_group", "pod_group_update": "update_pod_group",
            "pod_group_delete": "delete_pod_group", "pdb_add": "add_pdb", "pdb_update": "update_pdb",
            "pdb_delete": "delete_pdb", "queue_add": "add_queue", "queue_update": "update_queue",
            "queue_delete": "delete_queue", "namespace_add": "add_namespace",
            "namespace_update": "update_namespace", "namespace_delete": "delete_namespace"}


def _ns_name(obj):
    return obj if isinstance(obj, str) else obj["name"]


def replay(fx0, rounds):
    """The cache of fx0 after every change of `rounds` (a list of change
    lists), handler by handler (kbgpu/cache.py)."""
    from kbgpu.cache import FakeBinder, cache_from_fixture
    cache = cache_from_fixture(fx0, FakeBinder())
    pods = {p["uid"]: p for p in fx0["pods"]}
    for changes in rounds:
        for kind, obj in changes:
            if kind == "pod_add":
                cache.add_pod(obj)
                pods[obj["uid"]] = obj
            elif kind == "pod_update":
                cache.update_pod(pods[obj["uid"]], obj)
                pods[obj["uid"]] = obj
            elif kind == "pod_delete":
                cache.delete_pod(obj)
                pods.pop(obj["uid"], None)
            elif kind.startswith("namespace_"):
                getattr(cache, _HANDLER[kind])(_ns_name(obj))
            else:
                getattr(cache, _HANDLER[kind])(obj)
    return cache


def fixture_after(fx0, rounds):
    """fx0 after the changes as a fixture, or None when a fixture cannot say
    it: a deleted node that pods still name (a fresh cache would make a
    NodeInfo(nil)), or a job whose fields were last written by a PodGroup or
    PDB other than the one a fresh cache sets last (a fixture's PDBs are set
    after its PodGroups; UnsetPDB / UnsetPodGroup restore nothing)."""
    pods = {p["uid"]: p for p in fx0["pods"]}
    nodes = {n["name"]: n for n in fx0["nodes"]}
    groups = {f"{g.get('namespace', '')}/{g['name']}": g for g in fx0.get("podGroups", [])}
    pdbs = {d.get("controller", ""): d for d in fx0.get("pdbs", [])}
    queues = {}  # name -> its Queue, or None for a namespace (weight 1)
    for q in fx0.get("queues", []):
        queues[q["name"]] = q
    for n in fx0.get("namespaces", []):
        queues[_ns_name(n)] = None
    last = {jid: "pdb" for jid in pdbs}  # which of the two wrote the job's fields last
    gone = set()
    for changes in rounds:
        for kind, o in changes:
            if kind in ("pod_add", "pod_update"):
                pods.pop(o["uid"], None)
                pods[o["uid"]] = o
            elif kind == "pod_delete":
                pods.pop(o["uid"], None)
            elif kind in ("node_add", "node_update"):
                nodes[o["name"]] = o
                gone.discard(o["name"])
            elif kind == "node_delete":
                nodes.pop(o["name"], None)
                gone.add(o["name"])
            elif kind in ("pod_group_add", "pod_group_update"):
                jid = f"{o.get('namespace', '')}/{o['name']}"
                groups[jid] = o
                last[jid] = "pg"
            elif kind == "pod_group_delete":
                groups.pop(f"{o.get('namespace', '')}/{o['name']}", None)
            elif kind in ("pdb_add", "pdb_update"):
                pdbs[o.get("controller", "")] = o
                last[o.get("controller", "")] = "pdb"
            elif kind == "pdb_delete":
                pdbs.pop(o.get("controller", ""), None)
            elif kind == "queue_add":
                queues[o["name"]] = o
            elif kind == "queue_update":
                queues.pop(o["name"], None)
                queues[o["name"]] = o
            elif kind == "queue_delete":
                queues.pop(o["name"], None)
            elif kind == "namespace_add":
                queues[_ns_name(o)] = None
            elif kind == "namespace_update":
                queues.pop(_ns_name(o), None)
                queues[_ns_name(o)] = None
            elif kind == "namespace_delete":
                queues.pop(_ns_name(o), None)
            else:
                raise ValueError(kind)
    if any(p.get("nodeName") in gone for p in pods.values()):
        return None
    for jid in set(groups) | set(pdbs):  # a fresh cache sets the PodGroups, then the PDBs
        want = "pdb" if jid in pdbs else "pg"
        if last.get(jid, want) != want:
            return None
    fx1 = dict(fx0, pods=list(pods.values()), nodes=list(nodes.values()), podGroups=list(groups.values()),
               pdbs=list(pdbs.values()), queues=[q for q in queues.values() if q is not None])
    fx1.pop("namespaces", None)
    if any(q is None for q in queues.values()):
        fx1["namespaces"] = [n for n, q in queues.items() if q is None]
    return fx1


# ------------------------------------------------------------ hand-written
def _pod(uid, ns, group, phase="Pending", node="", cpu="1", controller=None):
    p = {"uid": uid, "namespace": ns, "name": uid, "phase": phase, "nodeName": node,
         "containers": [{"requests": {"cpu": cpu}}]}
    if group:
        p["annotations"] = {GROUP: group}
    if controller:
        p["controller"] = controller
    return p


def _pg(ns, name, queue, min_member=1, created=0):
    return {"namespace": ns, "name": name, "minMember": min_member, "queue": queue, "creationTimestamp": created}


def _nodes(n, cpu):
    return [{"name": f"n{i + 1}", "allocatable": {"cpu": str(cpu), "memory": "8Gi", "pods": "110"}} for i in range(n)]


def _gang(min_member):
    """2 nodes x 1 CPU, one job of 2 Pending 1-CPU pods, a second queue with a small job."""
    return {"nodes": _nodes(2, 1),
            "pods": [_pod("a1", "qa", "pga"), _pod("a2", "qa", "pga")],
            "podGroups": [_pg("qa", "pga", "qa", min_member)],
            "queues": [{"name": "qa", "weight": 1}, {"name": "qb", "weight": 1}]}


def _two_queues():
    """1 node x 4 CPU, two queues 1:1, each with one job of 4 Pending 1-CPU pods."""
    return {"nodes": _nodes(1, 4),
            "pods": [_pod(f"a{i}", "qa", "pga") for i in range(1, 5)] + [_pod(f"b{i}", "qb", "pgb") for i in range(1, 5)],
            "podGroups": [_pg("qa", "pga", "qa"), _pg("qb", "pgb", "qb", created=1)],
            "queues": [{"name": "qa", "weight": 1}, {"name": "qb", "weight": 1}]}


def _three_jobs():
    """As _two_queues, the jobs split 1 + 2 over the queues: moving one of
    queue qb's jobs to qa changes what each queue requests and deserves."""
    return {"nodes": _nodes(2, 2),
            "pods": [_pod("a1", "qa", "pga")] + [_pod(f"b{i}", "qb", "pgb") for i in range(1, 4)] +
                    [_pod(f"c{i}", "qb", "pgc") for i in range(1, 4)],
            "podGroups": [_pg("qa", "pga", "qa"), _pg("qb", "pgb", "qb", created=1), _pg("qb", "pgc", "qb", created=2)],
            "queues": [{"name": "qa", "weight": 1}, {"name": "qb", "weight": 1}]}


def _with_pdb(pod_group=True):
    """Two jobs on 2 nodes x 2 CPU; the first holds a PDB (its controller is
    the job's ID), with or without a PodGroup beside it. A PDB's job takes its
    namespace as its queue (job_info.go:188-200)."""
    fx = _two_queues()
    fx["nodes"] = _nodes(2, 2)
    fx["pods"][0] = dict(fx["pods"][0], phase="Running", nodeName="n1")
    if pod_group:
        fx["pdbs"] = [{"namespace": "qa", "name": "pdba", "controller": "qa/pga", "minAvailable": 2}]
    else:
        fx["pods"] = [_pod(f"a{i}", "qa", None, controller="ctl-a") for i in range(1, 5)] + fx["pods"][4:]
        fx["pods"][0] = dict(fx["pods"][0], phase="Running", nodeName="n1")
        fx["podGroups"] = fx["podGroups"][1:]
        fx["pdbs"] = [{"namespace": "qa", "name": "pdba", "controller": "ctl-a", "minAvailable": 1}]
    return fx


def _namespaces():
    fx = _two_queues()
    fx["queues"] = []
    fx["namespaces"] = ["qa", "qb"]
    for g in fx["podGroups"]:
        g["queue"] = ""  # the job's queue is its namespace
    return fx


def _case_job_in_updated_queue():
    new = [_pod(f"d{i}", "qa", "pgd") for i in range(1, 3)]
    return (_two_queues(),
            [[("queue_update", {"name": "qa", "weight": 2}), ("queue_add", {"name": "qc", "weight": 1}),
              ("pod_group_add", _pg("qa", "pgd", "qa", created=5))] + [("pod_add", p) for p in new]])


# name -> (fx0, rounds): `rounds` is a list of change lists, one session update each
CASES = {
    # MinMember raised: 2 pods can never make 3, nothing dispatches; lowered: both do
    "min_member_up": lambda: (_gang(1), [[("pod_group_update", _pg("qa", "pga", "qa", 3))]]),
    "min_member_down": lambda: (_gang(3), [[("pod_group_update", _pg("qa", "pga", "qa", 2))]]),
    # an AddPodGroup of a JobID the cache holds is the same setPodGroup
    "pod_group_add_again": lambda: (_gang(1), [[("pod_group_add", _pg("qa", "pga", "qa", 3))]]),
    "queue_move": lambda: (_three_jobs(), [[("pod_group_update", _pg("qb", "pgc", "qa", created=2))]]),
    "queue_set_weight": lambda: (_two_queues(), [[("queue_add", {"name": "qb", "weight": 3})]]),
    "queue_update": lambda: (_two_queues(), [[("queue_update", {"name": "qa", "weight": 3})]]),
    "queue_update_then_adds": _case_job_in_updated_queue,
    # a second update of the session the queue_update renumbered
    "queue_update_chain": lambda: (_two_queues(), [[("queue_update", {"name": "qa", "weight": 3})],
                                                   [("queue_add", {"name": "qa", "weight": 1}),
                                                    ("pod_group_update", _pg("qb", "pgb", "qb", 4, created=1))]]),
    "pdb_add": lambda: (_two_queues(), [[("pdb_add", {"namespace": "qa", "name": "pdba", "controller": "qa/pga",
                                                       "minAvailable": 5})]]),
    "pdb_add_new_job": lambda: (_two_queues(), [[("pdb_add", {"namespace": "qb", "name": "pdbx", "controller": "ctl-x",
                                                               "minAvailable": 1}),
                                                  ("pod_add", _pod("x1", "qb", None, controller="ctl-x"))]]),
    "pdb_delete_with_pod_group": lambda: (_with_pdb(), [[("pdb_delete", {"namespace": "qa", "name": "pdba",
                                                                         "controller": "qa/pga"})]]),
    "pdb_delete_alone": lambda: (_with_pdb(False), [[("pdb_delete", {"namespace": "qa", "name": "pdba",
                                                                     "controller": "ctl-a"})]]),
    "pod_group_delete_pdb_left": lambda: (_with_pdb(), [[("pod_group_delete", _pg("qa", "pga", "qa"))]]),
    "namespaces": lambda: (_namespaces(), [[("namespace_add", "qc"), ("namespace_add", "qa"),
                                            ("namespace_update", "qa")]]),
    "namespace_delete": lambda: (_namespaces(), [[("namespace_update", {"name": "qb"}), ("namespace_delete", "qa")]]),
}

# cases whose batch holds only in-place events (JOB_UPDATE / QUEUE_SET)
IN_PLACE = ("min_member_up", "min_member_down", "pod_group_add_again", "queue_move", "queue_set_weight", "pdb_add")
# cases after which the next cycle must differ from the one before the update
CHANGES_OUTCOME = ("min_member_up", "min_member_down", "queue_move", "queue_set_weight", "pdb_add",
                   "pdb_delete_alone", "namespace_delete")


# ------------------------------------------------------------------- fuzz
def fuzz_fixture(seed):
    from kbgpu import synth
    if seed % 3:
        return synth.random_fixture(21000 + seed)
    return synth.contended_fixture(21000 + seed, nodes=12, jobs=8, tasks=6)


def fuzz_changes(fx, seed, view):
    """One batch mixing the update events with the structural kinds
    (synth.structural; even seeds) or with pod churn and node updates alone
    (synth.churn; odd seeds: KBG_EV_JOB_UPDATE / QUEUE_SET beside pod events,
    applied without a rebuild). Only accepted changes: PodGroups and PDBs of
    session jobs that stay, to queues that stay; weights of queues that stay.
    `view`: the session (its jobs, queues and tasks as the wrapper lists them)."""
    from kbgpu import synth
    rng = random.Random(seed * 7919 + 13)
    jobs = {j.uid: j for j in view.jobs}
    queues = [q.uid for q in view.queues]
    uids = {t.uid for t in view.flat.task_objs}
    in_place = seed % 2 == 1  # odd seeds: no structural kind, so the batch is applied without a rebuild
    if in_place:  # pod churn (completions, deletions, new pods of session jobs) and node updates
        base = synth.churn(fx, seed, uids, done=0.15, delete=0.05, add=0.05, node_frac=0.1)[0]
    else:
        base = synth.structural(fx, seed, set(jobs), uids, queues)
    gone_q = {o["name"] for k, o in base if k == "queue_delete"}
    gone_j = {f"{o.get('namespace', '')}/{o['name']}" for k, o in base if k == "pod_group_delete"}
    gone_j |= {uid for uid, j in jobs.items() if j.queue in gone_q}
    groups = {f"{g.get('namespace', '')}/{g['name']}": g for g in fx.get("podGroups", [])}
    stay_j = sorted(uid for uid in jobs if uid not in gone_j and uid in groups and jobs[uid].pdb is None)
    stay_q = [q for q in queues if q not in gone_q]
    weight = {q.uid: q.weight for q in view.queues}
    pre, post = [], []

    def some(n):
        return rng.sample(stay_j, min(len(stay_j), n))

    for uid in some(rng.randint(0, 2)):  # MinMember raised or lowered
        (pre if rng.random() < 0.5 else post).append(
            ("pod_group_update", dict(groups[uid], queue=jobs[uid].queue, minMember=rng.randint(0, 4))))
    if len(stay_q) > 1:
        for uid in some(rng.randint(0, 2)):  # a job moves to another live queue
            to = rng.choice([q for q in stay_q if q != jobs[uid].queue] or stay_q)
            (pre if rng.random() < 0.5 else post).append(("pod_group_update", dict(groups[uid], queue=to)))
    for q in rng.sample(stay_q, min(len(stay_q), rng.randint(0, 2))):  # addQueue of a UID the cache holds
        (pre if rng.random() < 0.5 else post).append(("queue_add", {"name": q, "weight": rng.randint(1, 4)}))
    if stay_q and not in_place and rng.random() < 0.5:  # updateQueue: the queue takes the last place, its jobs stay
        q = rng.choice(stay_q)
        (pre if rng.random() < 0.6 else post).append(("queue_update", {"name": q, "weight": rng.randint(1, 4)}))
    if stay_j and stay_q and rng.random() < 0.5:  # a PDB beside a session job's PodGroup (its namespace: its queue)
        uid = rng.choice(stay_j)
        pdb = {"namespace": rng.choice(stay_q), "name": f"pdb{seed}", "controller": uid,
               "minAvailable": rng.randint(0, 3), "creationTimestamp": 10 ** 12 + 2 * seed}
        if not (fx.get("options") or {}).get("defaultQueue"):
            pre.append(("pdb_add", pdb))
            r = rng.random()
            if r < 0.3:
                post.append(("pdb_delete", pdb))  # the PodGroup keeps the job
            elif r < 0.5:
                post.append(("pod_group_delete", groups[uid]))  # the PDB keeps the job
            elif r < 0.7:
                post.append(("pdb_update", dict(pdb, minAvailable=rng.randint(0, 3))))
    live = [t.pod for t in view.flat.task_objs if t is not None and t.job in stay_j]
    if live and stay_q and not in_place and rng.random() < 0.4 and not (fx.get("options") or {}).get("defaultQueue"):
        # a PDB of a controller new to the cache: a new job, with a pod
        base_pod = rng.choice(live)
        ctl = f"ctl{seed}"
        post.append(("pdb_add", {"namespace": rng.choice(stay_q), "name": f"pdbn{seed}", "controller": ctl,
                                 "minAvailable": rng.randint(0, 2), "creationTimestamp": 10 ** 12 + 2 * seed + 1}))
        p = dict(copy.deepcopy(base_pod), uid=f"pc{seed}", name=f"pc{seed}", phase="Pending", nodeName="",
                 controller=ctl)
        p["annotations"] = {k: v for k, v in (p.get("annotations") or {}).items() if k != GROUP}
        p.pop("deletionTimestamp", None)
        post.append(("pod_add", p))
    return pre + base + post


# Seeds chosen on the CPU: S0 and S1 both open under the oracle ("ok", no
# RefPanic), the wrapper accepts the batch and the library applies it.
# Every one of them carries at least one of the new kinds; half are even
# (structural batches), half odd (in-place batches beside pod churn); 24 of
# the 40 can say S1 as a fixture (fixture_after), so the oracle runs their S1.
SEEDS = [0, 2, 6, 7, 9, 10, 11, 12, 15, 16, 17, 18, 21, 23, 24, 26, 27, 28, 30, 35,
         37, 39, 40, 42, 43, 45, 46, 50, 51, 52, 53, 54, 57, 59, 60, 61, 65, 69, 72, 74]
GPU_SEEDS = [0, 6, 7, 9, 12, 15, 16, 23, 24, 27, 28, 35, 39, 40, 42, 45, 46, 51, 52, 57]  # 20 of them
