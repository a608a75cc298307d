"""What the resident-session tests share and a CPU-only module may import
(tests/test_update_gpu.py is a gpu module): a session opened on a fixture, the
cycle's actions through the C ABI, the Python cache replayed through a change
list, and the fixture that says the cache after it."""
import ctypes

from kbgpu import _abi
from kbgpu.api import pod_key
from kbgpu.cache import FakeBinder, cache_from_fixture
from kbgpu.fixture import _OrderedCache, fixture_tiers
from kbgpu.framework import open_session

ENTRY = {"allocate": "kbg_allocate", "backfill": "kbg_backfill", "reclaim": "kbg_reclaim", "preempt": "kbg_preempt"}


def _open(fx, opts=None):
    return open_session(_OrderedCache(cache_from_fixture(fx, FakeBinder()), fx), fixture_tiers(fx), opts or {})


def abi_cycle(ssn, actions):
    """The cycle's actions through the C ABI; results in run_fixture's schema
    (decisions, binds, job / queue / node state), without the host replay."""
    L = _abi.lib()
    cap = max(1, len(ssn.flat.task_objs))
    buf = (_abi.kbg_decision * cap)()
    n = ctypes.c_int32(0)
    status = "ok"
    for a in actions:
        code = getattr(L, ENTRY[a])(ssn.handle, buf, cap, ctypes.byref(n))
        if code == _abi.KBG_E_REF_PANIC:
            return {"status": "ref_panic"}
        if code == _abi.KBG_E_UNSUPPORTED:
            return {"status": "unsupported"}
        _abi.check(code)
    acts = (ctypes.c_int32 * cap)()
    m = ctypes.c_int32(0)
    _abi.check(L.kbg_decision_actions_get(ssn.handle, acts, cap, ctypes.byref(m)))
    tasks, names = ssn.flat.task_objs, ssn.flat.node_names
    out = {"status": status, "decisions": [], "binds": {}, "jobs": [], "queues": [], "nodes": []}
    for i in range(n.value):
        d = buf[i]
        row = {"task": tasks[d.task].uid, "job": tasks[d.task].job, "node": names[d.node],
               "kind": "allocate" if d.kind == _abi.KIND_ALLOCATE else "pipeline", "dispatched_at": d.dispatched_at}
        if acts[i] != 0:
            row["action"] = _abi.ACTION_NAMES[acts[i]]
        out["decisions"].append(row)
        if d.dispatched_at >= 0:
            out["binds"][pod_key(tasks[d.task].pod)] = names[d.node]
    for j, job in enumerate(ssn.jobs):
        st = ssn.job_state(j)
        row = {"uid": job.uid, "ready_num": st.ready_num, "ready": bool(st.ready), "drf_share": st.drf_share}
        if st.fit_valid:
            from kbgpu.fixture import fit_error
            row["fit_error"] = fit_error(st.fit_nodes, st.fit_cpu, st.fit_memory, st.fit_gpu)
        out["jobs"].append(row)
    for q, queue in enumerate(ssn.queues):
        st = ssn.queue_state(q)
        if st.has_attr:
            out["queues"].append({"uid": queue.uid, "share": st.share,
                                  "deserved": [st.deserved.milli_cpu, st.deserved.memory, st.deserved.milli_gpu]})
    for i, nd in enumerate(ssn.nodes):
        st = ssn.node_state(i)
        out["nodes"].append({"name": nd.name, "idle": [st.idle.milli_cpu, st.idle.memory, st.idle.milli_gpu],
                             "releasing": [st.releasing.milli_cpu, st.releasing.memory, st.releasing.milli_gpu],
                             "ntasks": st.num_tasks})
    return out


def _replay(fx0, changes):
    """The cache of fx0 after `changes` (event_handlers.go): what a fresh open
    of the updated cache sees, including what a fixture cannot say (pods
    whose node was deleted, PodGroup-less jobs that still hold pods)."""
    cache = cache_from_fixture(fx0, FakeBinder())
    pods = {p["uid"]: p for p in fx0["pods"]}
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
        else:
            getattr(cache, {"node_add": "add_node", "node_update": "update_node", "node_delete": "delete_node",
                            "pod_group_add": "add_pod_group", "pod_group_delete": "delete_pod_group",
                            "queue_add": "add_queue", "queue_delete": "delete_queue"}[kind])(obj)
    return cache


def _fixture_after(fx0, changes):
    """fx0 after `changes` as a fixture, or None when a fixture cannot say it:
    a deleted node that pods still name (a fresh cache would make a
    NodeInfo(nil) for them; the live one has none)."""
    pods = {p["uid"]: p for p in fx0["pods"]}
    nodes = {n["name"]: n for n in fx0["nodes"]}
    groups = {(g.get("namespace", ""), g["name"]): g for g in fx0.get("podGroups", [])}
    queues = {q["name"]: q for q in fx0.get("queues", [])}
    gone = set()
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
        elif kind == "pod_group_add":
            groups[(o.get("namespace", ""), o["name"])] = o
        elif kind == "pod_group_delete":
            groups.pop((o.get("namespace", ""), o["name"]), None)
        elif kind == "queue_add":
            queues[o["name"]] = o
        elif kind == "queue_delete":
            queues.pop(o["name"], None)
    if any(p.get("nodeName") in gone for p in pods.values()):
        return None
    return dict(fx0, pods=list(pods.values()), nodes=list(nodes.values()), podGroups=list(groups.values()),
                queues=list(queues.values()))
