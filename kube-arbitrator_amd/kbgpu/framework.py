"""framework: Session, plugin/action registries (pkg/scheduler/framework).

`open_session` / `close_session` mirror framework.OpenSession / CloseSession
(framework.go:26-54). The plugins named in the tiers (drf, proportion, gang,
priority, predicates) run their OnSessionOpen inside the device library
(kbg_session_open), which also uploads the node table to HBM. Every tier
entry goes to the library with KBG_PLUGIN_REGISTERED set when this process's
registry has a builder for its name (kbg_options.plugin_registry = 1): names
without one are skipped, exactly like GetPluginBuilder misses
(framework.go:30-35), and a registered plugin the library does not implement
refuses the session (KBG_E_UNSUPPORTED: run the reference path). `Session.allocate` / `Session.pipeline` /
`Session.dispatch` replay device decisions into the host objects with the
reference's bookkeeping (session.go:205-316).
"""
import ctypes
import os

import numpy as np

from . import _abi
from .api import ALLOCATED, BINDING, PENDING, PIPELINED, RELEASING, pod_key
from .snapshot import FlatSnapshot

KNOWN_PLUGINS = ("priority", "gang", "drf", "predicates", "proportion")

_plugin_builders = {n: n for n in KNOWN_PLUGINS}
_actions = {}


def register_plugin_builder(name, builder=None):  # plugins.go:28-33
    _plugin_builders[name] = builder or name


def cleanup_plugin_builders():  # plugins.go:35-40
    _plugin_builders.clear()


def get_plugin_builder(name):  # plugins.go:42-49
    return _plugin_builders.get(name)


def register_action(action):  # plugins.go:53-58
    _actions[action.name()] = action


def get_action(name):  # plugins.go:60-66
    return _actions.get(name)


def _copy_job_fields(src, dst):
    """What SetPodGroup / SetPDB / UnsetPodGroup / UnsetPDB write (job_info.go:166-226)."""
    for k in ("name", "namespace", "queue", "priority", "min_available", "creation_timestamp", "pod_group", "pdb"):
        setattr(dst, k, getattr(src, k))
    return dst


class Session:
    """framework.Session (session.go:35-61) plus the device handle."""

    def __init__(self, cache, tiers, options=None, reasons=False):
        snap = cache.snapshot()
        self.cache = cache
        self.jobs = snap.jobs  # JobValid is a no-op at openSession time
        self.job_index = {j.uid: j for j in self.jobs}
        self.nodes = snap.nodes
        self.node_index = {n.name: n for n in self.nodes}
        self.queues = snap.queues
        self.queue_index = {q.uid: q for q in self.queues}
        self.others = snap.others
        self.tiers = tiers
        self.plugins = [p.name for t in tiers for p in t.plugins if get_plugin_builder(p.name) is not None]
        self.flat = FlatSnapshot(self.nodes, self.jobs, self.queues, self.others, self.tiers,
                                 registered=lambda name: get_plugin_builder(name) is not None)
        self.handle = ctypes.c_void_p()
        opts = _abi.kbg_options()
        opts.device = -1
        opts.plugin_registry = 1
        options = dict(options or {})
        comm = options.pop("comm", None)  # dist.ShardComm: node-axis shard of an RCCL clique
        for k, v in options.items():
            setattr(opts, k, v)
        if reasons:
            opts.reasons = 1
        # allocate also computes the unschedulable reasons (job_reasons; not over a communicator)
        self.reasons = bool(opts.reasons) and comm is None
        L = _abi.lib()
        if comm is not None:
            _abi.check(L.kbg_session_open_sharded(ctypes.byref(self.flat.snap), ctypes.byref(opts), comm.handle,
                                                  ctypes.byref(self.handle)))
        else:
            _abi.check(L.kbg_session_open(ctypes.byref(self.flat.snap), ctypes.byref(opts),
                                          ctypes.byref(self.handle)))
        self.decisions = []
        self.action_of = []  # action name of each decision of the cycle
        self.evictions = []  # (task, by, action) committed evictions (cache.Evict)

    # ---- session.go:205-241
    def pipeline(self, task, hostname):
        job = self.job_index.get(task.job)
        if job is not None:
            job.update_task_status(task, PIPELINED)
        task.node_name = hostname
        node = self.node_index.get(hostname)
        if node is not None:
            node.add_task(task)

    # ---- session.go:243-293 (the JobReady/dispatch decision comes from the device log)
    def allocate(self, task, hostname):
        job = self.job_index.get(task.job)
        if job is not None:
            job.update_task_status(task, ALLOCATED)
        task.node_name = hostname
        node = self.node_index.get(hostname)
        if node is not None:
            node.add_task(task)

    # ---- session.go:295-316
    def dispatch(self, task):
        self.cache.bind(task, task.node_name)
        job = self.job_index.get(task.job)
        if job is not None:
            job.update_task_status(task, BINDING)

    # ---- session.go:318-352 / statement.go: the resource side of evictions and of
    # the pipelines that follow them lives in the device session (node Idle /
    # Releasing, including what discarded statements leave behind); the host
    # objects record the statuses, the node membership and the cache's Evict.
    def evict(self, task, reason):
        job = self.job_index.get(task.job)
        if job is not None:
            job.update_task_status(task, RELEASING)
        node = self.node_index.get(task.node_name)
        if node is not None:
            held = node.tasks.get(pod_key(task.pod))
            if held is not None:
                held.status = RELEASING
        self.cache.evict(task, reason)

    def pipeline_replay(self, task, hostname):
        job = self.job_index.get(task.job)
        if job is not None:
            job.update_task_status(task, PIPELINED)
        task.node_name = hostname
        node = self.node_index.get(hostname)
        if node is not None and pod_key(task.pod) not in node.tasks:
            node.tasks[pod_key(task.pod)] = task.clone()

    def sync_node_resources(self):
        """Idle / Releasing of every host NodeInfo from the device session,
        after an action whose statements changed them (reclaim, preempt), so
        later actions' replays account from the same values."""
        for i, name in enumerate(self.flat.node_names):
            node = self.node_index.get(name)
            if node is None or node.node is None:
                continue
            st = self.node_state(i)
            for mine, dev in ((node.idle, st.idle), (node.releasing, st.releasing)):
                mine.milli_cpu, mine.memory, mine.milli_gpu = dev.milli_cpu, dev.memory, dev.milli_gpu

    def update(self, changes):
        """kbg_session_update: cache events since the session's snapshot,
        applied to the resident session (include/kbgpu.h). `changes` is a list
        of ("pod_update", pod) | ("pod_delete", pod) | ("pod_add", pod) |
        ("node_add", node) | ("node_update", node) | ("node_delete", node) |
        ("pod_group_add", pg) | ("pod_group_update", pg) | ("pod_group_delete", pg) |
        ("pdb_add", pdb) | ("pdb_update", pdb) | ("pdb_delete", pdb) |
        ("queue_add", q) | ("queue_update", q) | ("queue_delete", q) |
        ("namespace_add", ns) | ("namespace_update", ns) | ("namespace_delete", ns)
        in event order, objects as the informer delivers
        them (event_handlers.go). New pods must use a pod spec the session
        already has. Structural changes (a node, PodGroup or queue joins or
        leaves, a queue is updated: delete + add; a pod naming a node the cache
        does not know, which makes a NodeInfo(nil), event_handlers.go:49-53)
        renumber the session: the wrapper's task, node, job and queue lists
        follow the library's renumbering (kbg_session_renumbering). A PodGroup
        or PDB set on a session job (KBG_EV_JOB_UPDATE) and a queue added again
        under a UID the session holds (KBG_EV_QUEUE_SET) change it in place.
        A queue, PodGroup or PDB that returns for jobs or pods the cache holds
        outside ssn.Jobs (a deleted queue added again, a PodGroup deleted and
        set again on a job with pods, a queue that was missing at open) would
        bring them back in the reference's cache; the session adopts none of
        them, so marshal raises a ValueError naming the queue or JobID: re-open.
        The wrapper's JobInfo / QueueInfo objects follow the events (pod_group,
        pdb, min_available, queue, weight) once the library took the batch;
        the host-side task and node objects are not replayed: read results
        through the C ABI (decisions, job / queue / node state)."""
        plan = self.marshal(changes)
        _abi.check(_abi.lib().kbg_session_update(self.handle, plan.evs, plan.n_ev))
        self._accept(plan)

    def marshal(self, changes):
        """The kbg_event batch of `changes` against this session's current
        numbering (update's first half; host-only, also used by the CPU tests
        of the structural path through the tool library)."""
        from types import SimpleNamespace
        from .api import JobInfo, NodeInfo, QueueInfo, TaskInfo, pod_key
        flat = self.flat
        tidx = {t.uid: i for i, t in enumerate(flat.task_objs) if t is not None}
        nidx = {n: i for i, n in enumerate(flat.node_names) if n}
        pod_only = dict(flat.pod_only_names)  # NodeName -> index of a node the cache knows only from pods
        jidx = dict(flat.job_index)
        qidx = dict(flat.queue_index)
        n_nodes, n_jobs, n_queues = len(flat.node_names), len(self.jobs), len(self.queues)
        new_nodes, new_jobs, new_queues = {}, {}, {}  # new index -> NodeInfo / JobInfo / QueueInfo
        # at most two events per change: a pod naming a node new to the cache makes it first
        evs = (_abi.kbg_event * max(1, 2 * len(changes)))()
        n_ev = 0
        keep = []
        objs = {}  # task index -> its TaskInfo after the events (applied once the library accepts them)
        n_objs = len(flat.task_objs)
        renamed = {}  # pod-only node index -> the name its Node gave it
        # wrapper state the events change, applied in _accept once the library took the batch:
        job_edits = {}  # session job index -> a JobInfo holding its fields after the events
        queue_weights = {}  # session queue index -> its weight after the events
        queue_moved = {}  # queue index a queue_update killed -> the index the queue took
        outside = set()  # JobIDs whose pods stay in the cache outside the session jobs
        # the cache's jobs outside ssn.Jobs as the events leave them (applied in _accept): a job that
        # left keeps its JobInfo and its tasks in sc.Jobs (deletePodGroup, event_handlers.go:366-380;
        # deleteQueue removes only sc.Queues[uid], :649-654), so a queue or PodGroup that returns
        # brings back what the session dropped
        away = dict(self._away_jobs())
        dead_uids = set()  # pods the batch deleted
        live_delta = {}  # JobID -> pods the batch added minus those it deleted
        base_live = []  # (lazily) JobID -> its live pods in the wrapper's task list
        default_queue = getattr(self.cache, "default_queue", "")

        def ev():
            nonlocal n_ev
            n_ev += 1
            return evs[n_ev - 1]

        def job_of(j):
            if j in job_edits:
                return job_edits[j]
            return self.jobs[j] if j < len(self.jobs) else new_jobs[j]

        def job_edit(j):
            """Job j's fields to write: a job this batch added is the plan's own
            object; a session job gets a copy that _accept writes back."""
            if j >= len(self.jobs):
                return new_jobs[j]
            if j not in job_edits:
                job_edits[j] = _copy_job_fields(self.jobs[j], JobInfo(self.jobs[j].uid))
            return job_edits[j]

        def job_update(j, job):
            """KBG_EV_JOB_UPDATE: session job j takes SetPodGroup's / SetPDB's fields."""
            if job.queue not in qidx:
                raise ValueError(f"job {job.uid!r}: queue {job.queue!r} is not a session queue (re-open when it "
                                 "exists)")
            e = ev()
            e.kind, e.job = _abi.EV_JOB_UPDATE, j
            e.queue = qidx[job.queue]
            e.min_available = job.min_available
            e.priority = job.priority
            e.creation_ns = job.creation_timestamp

        def job_add(job):
            """KBG_EV_JOB_ADD of a JobID new to the cache (NewJobInfo + SetPodGroup / SetPDB)."""
            nonlocal n_jobs
            if job.queue not in qidx:
                raise ValueError(f"job {job.uid!r}: queue {job.queue!r} is not a session queue (re-open when it "
                                 "exists)")
            e = ev()
            e.kind = _abi.EV_JOB_ADD
            keep.append(job.uid.encode())
            e.name = keep[-1]
            e.queue = qidx[job.queue]
            e.min_available = job.min_available
            e.priority = job.priority
            e.creation_ns = job.creation_timestamp
            jidx[job.uid] = n_jobs
            new_jobs[n_jobs] = job
            n_jobs += 1

        def has_pods(jid):
            """Whether the cache's JobInfo of session job jid holds tasks now."""
            if not base_live:
                gone, count = self._dead_uids(), {}
                for t in flat.task_objs:
                    if t is not None and t.uid not in gone:
                        count[t.job] = count.get(t.job, 0) + 1
                base_live.append(count)
            return base_live[0].get(jid, 0) + live_delta.get(jid, 0) > 0

        def job_delete(jid):
            """KBG_EV_JOB_DELETE: neither a PodGroup nor a PDB is left (cache.go:570-582)."""
            e = ev()
            e.kind, e.job = _abi.EV_JOB_DELETE, jidx[jid]
            away[jid] = SimpleNamespace(queue=job_of(jidx[jid]).queue, pod_group=False, pdb=False, pods=has_pods(jid))
            jidx.pop(jid)
            if away[jid].pods:
                outside.add(jid)  # its pods stay in the cache, outside the session jobs

        def outside_job(jid):
            return jid in outside or jid in self._outside_jobs()

        def returning_job(jid, what):
            """A PodGroup or PDB set on a JobID the cache holds outside ssn.Jobs takes up
            the JobInfo it finds there (setPodGroup, event_handlers.go:344-358): its pods,
            or the PodGroup / PDB it kept, which the session does not hold."""
            a = away.get(jid)
            if a is None:
                return
            if a.pods or a.pod_group or a.pdb:
                raise ValueError(f"{what} {jid!r}: the cache holds that job outside the session jobs (it left the "
                                 "session, or its queue was missing, and keeps its pods, PodGroup or PDB): re-open")
            del away[jid]  # a JobInfo without pods, PodGroup or PDB: as good as new

        def returning_queue(name):
            """A queue that joins brings every cache job naming it into the snapshot
            (cache.go:584-588): jobs that left with it, or that never had their queue."""
            for jid, a in away.items():
                if a.queue == name and (a.pod_group or a.pdb):
                    raise ValueError(f"queue {name!r}: the cache holds job {jid!r} of that queue outside the session "
                                     "jobs (it left with the queue, or its queue was missing at open): re-open")

        def node_spec(e, obj):
            ni = NodeInfo(obj)
            e.resource = _abi.kbg_resource(*ni.allocatable.as_tuple())
            e.max_task_num = ni.allocatable.max_task_num
            e.unschedulable = 1 if obj.get("unschedulable") else 0
            labels = [x.encode() for kv in (obj.get("labels") or {}).items() for x in kv]
            taints = [str(t.get(f, "")).encode() for t in (obj.get("taints") or []) for f in ("key", "value", "effect")]
            la = (ctypes.c_char_p * max(1, len(labels)))(*labels)
            ta = (ctypes.c_char_p * max(1, len(taints)))(*taints)
            spec = _abi.kbg_node_spec(obj["name"].encode(), la, len(labels) // 2, len(taints) // 3, ta)
            keep.extend([la, ta, spec])
            e.node_spec = ctypes.pointer(spec)

        def node_of(name):
            """kbg_event.node of a pod's NodeName: the session node of that name,
            else the node the cache knows only from pods carrying it
            (sc.Nodes[NodeName]); a name the cache does not know makes that
            node (NewNodeInfo(nil), event_handlers.go:49-53): KBG_EV_NODE_ADD."""
            nonlocal n_nodes
            if not name:
                return -1
            i = nidx.get(name)
            if i is None:
                i = pod_only.get(name)
            if i is None:
                e = ev()
                e.kind = _abi.EV_NODE_ADD
                keep.append(name.encode())
                e.node_name = keep[-1]
                i = pod_only[name] = n_nodes
                new_nodes[i] = NodeInfo(None)
                n_nodes += 1
            return i

        def pod_node(e, name):
            e.node = node_of(name)
            if e.node >= 0 and name not in nidx:
                keep.append(name.encode())  # a node known only from pods: its NodeName
                e.node_name = keep[-1]

        for kind, obj in changes:
            if kind.startswith("namespace_"):  # a namespace used as a queue: its name, weight 1 (:726-755)
                kind = "queue_" + kind[len("namespace_"):]
                obj = {"name": obj if isinstance(obj, str) else obj["name"], "weight": 1}
            if kind in ("node_update", "node_add"):
                # cache.AddNode / UpdateNode -> SetNode with the whole Node (the library
                # compares labels and taints and rebuilds only when they change)
                name = obj["name"]
                idx = nidx.get(name)
                if idx is None:
                    idx = pod_only.get(name)
                    if idx is None:
                        if kind == "node_update":  # updateNode: "node does not exist" (event_handlers.go:249-259)
                            continue
                        e = ev()  # a new node: NewNodeInfo(node), last in the session's node order
                        e.kind = _abi.EV_NODE_ADD
                        node_spec(e, obj)
                        nidx[name] = n_nodes
                        new_nodes[n_nodes] = NodeInfo(obj)
                        n_nodes += 1
                        continue
                    pod_only.pop(name, None)
                    if idx in new_nodes:  # made by a pod earlier in the batch
                        new_nodes[idx] = NodeInfo(obj)
                    else:
                        renamed[idx] = name
                    nidx[name] = idx  # later events of the batch name the node by its Node's name
                e = ev()
                e.kind = _abi.EV_NODE_SET
                e.node = idx
                if os.environ.get("KBG_PY_NODE_UPDATE") == "1" and idx not in renamed:  # (A/B: Allocatable only)
                    ni = NodeInfo(obj)
                    e.kind = _abi.EV_NODE_UPDATE
                    e.resource = _abi.kbg_resource(*ni.allocatable.as_tuple())
                    e.max_task_num = ni.allocatable.max_task_num
                    e.unschedulable = 1 if obj.get("unschedulable") else 0
                    continue
                node_spec(e, obj)
                continue
            if kind == "node_delete":  # deleteNode (event_handlers.go:262-268); an unknown name is an error there
                name = obj["name"]
                idx = nidx.pop(name, None)
                if idx is None:
                    idx = pod_only.pop(name, None)
                if idx is None:
                    continue
                e = ev()
                e.kind, e.node = _abi.EV_NODE_DELETE, idx
                continue
            if kind in ("pod_group_add", "pod_group_update", "pod_group_delete"):
                jid = f"{obj.get('namespace', '')}/{obj['name']}"
                if kind == "pod_group_delete":  # UnsetPodGroup: the job leaves ssn.Jobs unless a PDB keeps it
                    j = jidx.get(jid)
                    if j is not None:
                        if job_of(j).pdb is not None:
                            job_edit(j).pod_group = None  # it stays in ssn.Jobs, its fields as they are (cache.go:570)
                        else:
                            job_delete(jid)
                    elif jid in away:
                        away[jid] = SimpleNamespace(**dict(vars(away[jid]), pod_group=False))
                    continue
                if jid in jidx:  # setPodGroup on a job the session holds (:344-363): in place
                    job = job_edit(jidx[jid])
                    job.set_pod_group(obj, default_queue)
                    job_update(jidx[jid], job)
                    continue
                if outside_job(jid):
                    raise ValueError(f"PodGroup {jid!r}: the cache holds pods of it outside the session jobs "
                                     "(they predate the PodGroup): re-open")
                returning_job(jid, "PodGroup")
                job = JobInfo(jid)
                job.set_pod_group(obj, default_queue)
                job_add(job)
                continue
            if kind in ("pdb_add", "pdb_update", "pdb_delete"):
                jid = obj.get("controller", "")  # the JobID is the PDB's controller (:458-494)
                if not jid:  # "the controller of PodDisruptionBudget is empty": the handler returns an error
                    continue
                if kind == "pdb_delete":  # UnsetPDB: the job stays in ssn.Jobs while it has a PodGroup
                    j = jidx.get(jid)
                    if j is not None:
                        if job_of(j).pod_group is not None:
                            job_edit(j).pdb = None
                        else:
                            job_delete(jid)
                    elif jid in away:
                        away[jid] = SimpleNamespace(**dict(vars(away[jid]), pdb=False))
                    continue
                if jid in jidx:  # setPDB on a job the session holds: in place
                    job = job_edit(jidx[jid])
                    job.set_pdb(obj, default_queue)
                    job_update(jidx[jid], job)
                    continue
                if outside_job(jid):
                    raise ValueError(f"PodDisruptionBudget of {jid!r}: the cache holds pods of it outside the session "
                                     "jobs (they predate the PDB): re-open")
                returning_job(jid, "PodDisruptionBudget of")
                job = JobInfo(jid)
                job.set_pdb(obj, default_queue)
                job_add(job)
                continue
            if kind in ("queue_add", "queue_update", "queue_delete"):
                qi = QueueInfo(obj["name"], obj.get("weight", 0))
                if kind == "queue_delete":
                    q = qidx.pop(qi.uid, None)
                    if q is not None:
                        e = ev()
                        e.kind, e.queue = _abi.EV_QUEUE_DELETE, q
                        for jid in [k for k, j in jidx.items() if job_of(j).queue == qi.uid]:
                            job = job_of(jidx[jid])  # it leaves ssn.Jobs (cache.go:584-588); sc.Jobs keeps it
                            away[jid] = SimpleNamespace(queue=qi.uid, pod_group=job.pod_group is not None,
                                                        pdb=job.pdb is not None, pods=has_pods(jid))
                            jidx.pop(jid)
                            if away[jid].pods:
                                outside.add(jid)
                    continue
                q = qidx.get(qi.uid)
                if q is not None and kind == "queue_add":  # sc.Queues[uid] = qi of a UID the cache holds: in place
                    e = ev()
                    e.kind, e.queue, e.weight = _abi.EV_QUEUE_SET, q, qi.weight
                    if q < len(self.queues):
                        queue_weights[q] = qi.weight
                    else:
                        new_queues[q].weight = qi.weight
                    continue
                e = ev()
                if q is not None:  # updateQueue: deleteQueue + addQueue, the queue takes the last place; its jobs stay
                    e.kind, e.queue = _abi.EV_QUEUE_UPDATE, q
                    queue_moved[q] = n_queues
                else:  # (an update of a queue the cache does not hold deletes nothing and adds it)
                    returning_queue(qi.uid)
                    e.kind = _abi.EV_QUEUE_ADD
                    keep.append(qi.uid.encode())
                    e.name = keep[-1]
                e.weight = qi.weight
                qidx[qi.uid] = n_queues
                new_queues[n_queues] = qi
                n_queues += 1
                continue
            ti = TaskInfo(obj)
            if kind in ("pod_update", "pod_delete"):
                if kind == "pod_update":
                    node_of(ti.node_name)  # a NodeInfo(nil) first, when the name is new to the cache
                e = ev()
                e.kind = _abi.EV_POD_UPDATE if kind == "pod_update" else _abi.EV_POD_DELETE
                e.task = tidx[obj["uid"]]
                e.status = ti.status
                if kind == "pod_update":
                    pod_node(e, ti.node_name)
                else:
                    dead_uids.add(ti.uid)
                    live_delta[ti.job] = live_delta.get(ti.job, 0) - 1
                objs[e.task] = ti
            elif kind == "pod_add":
                if ti.job not in jidx:
                    raise ValueError(f"pod {ti.uid!r}: job {ti.job!r} is not a session job (re-open)")
                node_of(ti.node_name)
                e = ev()
                e.kind = _abi.EV_POD_ADD
                e.job = jidx[ti.job]
                e.spec = flat.spec_index(obj)
                e.status = ti.status
                e.priority = ti.priority
                pod_node(e, ti.node_name)
                e.resource = _abi.kbg_resource(*ti.resreq.as_tuple())
                keep += [ti.uid.encode(), pod_key(obj).encode()]
                e.uid, e.pod_key = keep[-2], keep[-1]
                tidx[ti.uid] = n_objs
                objs[n_objs] = ti
                n_objs += 1
                dead_uids.discard(ti.uid)
                live_delta[ti.job] = live_delta.get(ti.job, 0) + 1
            else:
                raise ValueError(f"unknown change {kind}")
        return SimpleNamespace(evs=evs, n_ev=n_ev, keep=keep, objs=objs, n_objs=n_objs, renamed=renamed, tidx=tidx,
                               new_nodes=new_nodes, new_jobs=new_jobs, new_queues=new_queues, pod_only=pod_only,
                               job_edits=job_edits, queue_weights=queue_weights, queue_moved=queue_moved,
                               outside=outside, away=away, dead_uids=dead_uids, jidx=jidx, qidx=qidx)

    def _accept(self, plan, maps=None):
        """update's second half, once the library applied the batch: the
        wrapper's jobs and queues take the events' fields and its lists follow
        the library's (renumbered after a structural batch; `maps`: the four
        renumbering maps when the caller has them, as the CPU tests do)."""
        flat = self.flat
        evs, n_ev, objs, n_objs, tidx = plan.evs, plan.n_ev, plan.objs, plan.n_objs, plan.tidx
        new_nodes, new_jobs, new_queues, pod_only = plan.new_nodes, plan.new_jobs, plan.new_queues, plan.pod_only
        for i, name in plan.renamed.items():  # the NodeInfo the cache made from a pod has its Node's name now
            flat.node_names[i] = name
            flat.pod_only_names.pop(name, None)
            self.nodes[i].name = name
            self.node_index[name] = self.nodes[i]
        task_objs = flat.task_objs + [None] * (n_objs - len(flat.task_objs))
        for i, ti in objs.items():
            task_objs[i] = ti
        # the wrapper's jobs and queues follow the events (only here: a refused batch changes nothing)
        for j, job in plan.job_edits.items():
            _copy_job_fields(job, self.jobs[j])
        for q, weight in plan.queue_weights.items():
            self.queues[q].weight = weight
        self._outside_jobs().update(plan.outside)
        self._away = plan.away
        self._dead_uids().update(plan.dead_uids)
        structural = any(evs[k].kind in _abi.STRUCTURAL_EVENTS for k in range(n_ev))
        if structural or maps is not None:
            self._renumber(task_objs, new_nodes, new_jobs, new_queues, pod_only, maps=maps,
                           queue_moved=plan.queue_moved)
        else:
            flat.task_objs = task_objs
        from .api import PENDING
        live = set(tidx)  # (deleted pods keep their index; counts only size output buffers)
        flat.pending_all = max(flat.pending_all, sum(1 for t in flat.task_objs
                                                     if t is not None and t.uid in live and t.status == PENDING))
        flat.pending_count = max(flat.pending_count, flat.pending_all)

    def _outside_jobs(self):
        """JobIDs with pods the snapshot holds outside the session jobs
        (Others, pods on nodes): a PodGroup for one of them needs a re-open."""
        if getattr(self, "_outside", None) is None:
            mine = {t.uid for t in self.flat.task_objs if t is not None}
            out = {t.job for t in self.others}
            out |= {t.job for n in self.nodes for t in n.tasks.values() if t.uid not in mine}
            self._outside = out
        return self._outside

    def _away_jobs(self):
        """The cache's jobs outside ssn.Jobs: JobID -> its queue, whether it
        holds a PodGroup, a PDB, pods. From the cache the session was opened on
        (jobs whose queue was missing, jobs with neither PodGroup nor PDB), then
        kept by the accepted batches (marshal / _accept)."""
        if getattr(self, "_away", None) is None:
            from types import SimpleNamespace
            self._away = {jid: SimpleNamespace(queue=j.queue, pod_group=j.pod_group is not None,
                                               pdb=j.pdb is not None, pods=bool(j.tasks))
                          for jid, j in getattr(self.cache, "jobs", {}).items() if jid not in self.job_index}
        return self._away

    def _dead_uids(self):
        """Pods deleted in place: they keep their index in the task list until the next renumbering."""
        if getattr(self, "_dead", None) is None:
            self._dead = set()
        return self._dead

    def _renumber(self, task_objs, new_nodes, new_jobs, new_queues, pod_only, maps=None, queue_moved=None):
        """The wrapper's lists after a structural update, by the library's
        old -> new index maps (kbg_session_renumbering; `maps`: given).
        `queue_moved`: the queues a queue_update moved (dead index -> the index
        the queue took; KBG_RENUM_QUEUES maps both to its final place)."""
        L = _abi.lib()
        flat = self.flat

        def renum(kind):
            if maps is not None:
                return np.asarray(maps[kind], dtype=np.int64)
            n = ctypes.c_int32(0)
            _abi.check(L.kbg_session_renumbering(self.handle, kind, None, 0, ctypes.byref(n)))
            buf = (ctypes.c_int32 * max(1, n.value))()
            _abi.check(L.kbg_session_renumbering(self.handle, kind, buf, n.value, ctypes.byref(n)))
            return np.frombuffer(buf, dtype=np.int32, count=n.value).astype(np.int64)

        def remap(old, r):
            # out[r[i]] = old[i] for every kept i (r[i] >= 0); positions no old
            # entry maps to stay None. In numpy: a C4 session has 500k tasks.
            if r.size == 0 or r.max() < 0:
                return []
            out = np.full(int(r.max()) + 1, None, dtype=object)
            n = min(len(old), r.size)
            if n:
                src = np.fromiter(old if n == len(old) else old[:n], dtype=object, count=n)
                rr = r[:n]
                keep = rr >= 0
                out[rr[keep]] = src[keep]
            return out.tolist()

        rt, rn, rj, rq = (renum(k) for k in (_abi.RENUM_TASKS, _abi.RENUM_NODES, _abi.RENUM_JOBS, _abi.RENUM_QUEUES))
        flat.task_objs = remap(task_objs, rt)
        self._dead_uids().clear()  # the library's renumbering dropped every deleted pod
        nodes = list(self.nodes) + [new_nodes[i] for i in sorted(new_nodes)]
        names = list(flat.node_names) + [new_nodes[i].name for i in sorted(new_nodes)]
        self.nodes = remap(nodes, rn)
        flat.node_names = remap(names, rn)
        self.node_index = {n.name: n for n in self.nodes if n.name}
        flat.pod_only_names = {nm: int(rn[i]) for nm, i in pod_only.items() if i < len(rn) and rn[i] >= 0}
        jobs = list(self.jobs) + [new_jobs[i] for i in sorted(new_jobs)]
        self.jobs = remap(jobs, rj)
        self.job_index = {j.uid: j for j in self.jobs}
        flat.job_index = {j.uid: i for i, j in enumerate(self.jobs)}
        queues = list(self.queues) + [new_queues[i] for i in sorted(new_queues)]
        for old in sorted(queue_moved or {}, reverse=True):  # the dead index holds the queue as it is now
            queues[old] = queues[queue_moved[old]]
        self.queues = remap(queues, rq)
        self.queue_index = {q.uid: q for q in self.queues}
        flat.queue_index = {q.uid: i for i, q in enumerate(self.queues)}

    def job_state(self, j):
        st = _abi.kbg_job_state()
        _abi.check(_abi.lib().kbg_job_state_get(self.handle, j, ctypes.byref(st)))
        return st

    def job_reasons(self, j):
        """kbg_job_reasons of job j after allocate: the nodes that turned its
        last evaluated task away, per predicate stage (sessions opened with
        reasons=True)."""
        st = _abi.kbg_job_reasons()
        _abi.check(_abi.lib().kbg_job_reasons_get(self.handle, j, ctypes.byref(st)))
        return st

    def victim_reasons(self, mode, jobs=None):
        """kbg_victim_why per job (every job, or the indices `jobs`): why the
        next reclaim / preempt try of its first Pending task would find no
        victims, against the session as it is now. Legal after the cycle's
        first action on sessions opened with reasons=True; changes nothing."""
        if jobs is None:
            n, arr = len(self.jobs), None
        else:
            n = len(jobs)
            arr = (ctypes.c_int32 * max(n, 1))(*jobs)
        out = (_abi.kbg_victim_why * max(n, 1))()
        _abi.check(_abi.lib().kbg_victim_reasons(self.handle, int(mode), arr, n, out))
        return list(out[:n])

    def task_reasons(self, tasks=None):
        """One dict per task (the indices `tasks`, or every task Pending now in
        the mirror): why it would not be placed now, every live node under one
        cause against the session as it is (kbg_task_why). Legal any time
        after open on sessions opened with reasons=True; changes nothing."""
        if tasks is None:
            tasks = [t for t, obj in enumerate(self.flat.task_objs) if obj is not None and obj.status == PENDING]
        n = len(tasks)
        arr = (ctypes.c_int32 * max(n, 1))(*tasks)
        out = (_abi.kbg_task_why * max(n, 1))()
        _abi.check(_abi.lib().kbg_task_reasons(self.handle, arr, n, out))
        return [{"valid": bool(r.valid), "task": r.task, "visited": r.visited, "best_effort": bool(r.best_effort),
                 "queue_overused": bool(r.queue_overused), "count": list(r.count), "first_node": list(r.first_node),
                 "idle_short": list(r.idle_short)} for r in out[:n]]

    def task_headroom(self, tasks=None, limit=_abi.ROOM_MAX_LIMIT):
        """One dict per task (the indices `tasks`, or every task Pending now in
        the mirror): how many copies of it fit now, each live node taking up
        to `limit` (1..1024) copies one after the other from Idle, then from
        Releasing, under its pod cap (kbg_task_room). Legal any time after
        open on sessions opened with reasons=True; changes nothing."""
        if tasks is None:
            tasks = [t for t, obj in enumerate(self.flat.task_objs) if obj is not None and obj.status == PENDING]
        n = len(tasks)
        arr = (ctypes.c_int32 * max(n, 1))(*tasks)
        out = (_abi.kbg_task_room * max(n, 1))()
        _abi.check(_abi.lib().kbg_task_headroom(self.handle, arr, n, int(limit), out))
        return [{"valid": bool(r.valid), "task": r.task, "best_effort": bool(r.best_effort),
                 "queue_overused": bool(r.queue_overused), "limit": r.limit, "nodes_pass": r.nodes_pass,
                 "copies_idle": r.copies_idle, "copies_releasing": r.copies_releasing, "nodes_idle": r.nodes_idle,
                 "nodes_releasing_only": r.nodes_releasing_only, "first_node": r.first_node,
                 "max_node_copies": r.max_node_copies, "limit_hit": r.limit_hit, "affinity_now": bool(r.affinity_now),
                 "panic_nodes": r.panic_nodes} for r in out[:n]]

    def job_fit(self, jobs=None, limit=_abi.FIT_MAX_LIMIT):
        """One dict per job (the indices `jobs`, or every job): where its
        Pending tasks with a request, the first `limit` (1..512) in
        TaskOrderFn order, would land now, each on its first fitting node of a
        view in which the tasks before it have taken their share
        (kbg_job_fit). `places` holds (task, node, kind) per walked task, node
        -1 for a task no node takes. Legal any time after open on sessions
        opened with reasons=True; changes nothing."""
        if jobs is None:
            n, arr = len(self.jobs), None
        else:
            n, arr = len(jobs), (ctypes.c_int32 * max(len(jobs), 1))(*jobs)
        out = (_abi.kbg_job_fit * max(n, 1))()
        need = ctypes.c_int32(0)
        _abi.check(_abi.lib().kbg_job_fit(self.handle, arr, n, int(limit), out, None, 0, ctypes.byref(need)))
        places = (_abi.kbg_fit_place * max(need.value, 1))()
        _abi.check(_abi.lib().kbg_job_fit(self.handle, arr, n, int(limit), out, places, need.value, ctypes.byref(need)))
        keys = ("job", "pending", "walked", "placed_idle", "placed_releasing", "first_unplaced", "nodes_used",
                "ready_num", "min_available", "ready_after", "panic_nodes")
        rows = []
        for r in out[:n]:
            row = {"valid": bool(r.valid), **{k: getattr(r, k) for k in keys},
                   "queue_overused": bool(r.queue_overused), "affinity_now": bool(r.affinity_now), "places": []}
            if r.valid:
                row["places"] = [(p.task, p.node, p.kind) for p in places[r.place_off:r.place_off + r.walked]]
            rows.append(row)
        return rows

    def node_reasons(self, nodes=None):
        """One dict per node (the indices `nodes`, duplicates allowed, or every
        node): the tasks that are Pending now by the cause kbg_task_reasons
        gives this node in their rows, with the lowest task index per cause
        (kbg_node_why). Legal any time after open on sessions opened with
        reasons=True; changes nothing."""
        if nodes is None:
            n, arr = len(self.flat.node_names), None
        else:
            n, arr = len(nodes), (ctypes.c_int32 * max(len(nodes), 1))(*nodes)
        out = (_abi.kbg_node_why * max(n, 1))()
        _abi.check(_abi.lib().kbg_node_reasons(self.handle, arr, n, out))
        return [{"valid": bool(r.valid), "node": r.node, "pending": r.pending, "count": list(r.count),
                 "first_task": list(r.first_task), "idle_short": list(r.idle_short), "open_idle": r.open_idle,
                 "open_releasing": r.open_releasing, "idle_best_effort": r.idle_best_effort} for r in out[:n]]

    def node_drain(self, nodes=None, cordon=(), limit=_abi.FIT_MAX_LIMIT):
        """One dict per node (the indices `nodes`, duplicates allowed, or every
        node): where the pods it holds now, the first `limit` (1..512) in
        NodeInfo.Tasks order, would land if the node and every node of
        `cordon` took nothing, each on its first fitting node of a view in
        which the pods before it have taken their share (kbg_node_drain).
        `places` holds (task, node, kind) per walked task, node -1 for a task
        no node takes. Legal any time after open on sessions opened with
        reasons=True; changes nothing."""
        if nodes is None:
            n, arr = len(self.flat.node_names), None
        else:
            n, arr = len(nodes), (ctypes.c_int32 * max(len(nodes), 1))(*nodes)
        cordon = list(cordon)
        carr = (ctypes.c_int32 * len(cordon))(*cordon) if cordon else None
        out = (_abi.kbg_node_drain * max(n, 1))()
        need = ctypes.c_int32(0)
        L = _abi.lib()
        # one call: a buffer for `limit` places per row, or every task per row where that is less
        cap = max(1, n * min(int(limit) if 1 <= int(limit) <= _abi.FIT_MAX_LIMIT else 1, len(self.flat.task_objs)))
        places = (_abi.kbg_fit_place * cap)()
        _abi.check(L.kbg_node_drain(self.handle, arr, n, carr, len(cordon), int(limit), out, places, cap,
                                    ctypes.byref(need)))
        keys = ("node", "tasks", "walked", "placed_idle", "placed_releasing", "unplaced", "first_unplaced",
                "nodes_used", "other_pods", "jobs_moved", "jobs_short", "panic_nodes")
        rows = []
        for r in out[:n]:
            row = {"valid": bool(r.valid), **{k: getattr(r, k) for k in keys}, "affinity_now": bool(r.affinity_now),
                   "places": []}
            if r.valid:
                row["places"] = [(p.task, p.node, p.kind) for p in places[r.place_off:r.place_off + r.walked]]
            rows.append(row)
        return rows

    def queue_state(self, q):
        st = _abi.kbg_queue_state()
        _abi.check(_abi.lib().kbg_queue_state_get(self.handle, q, ctypes.byref(st)))
        return st

    def node_state(self, n):
        st = _abi.kbg_node_state()
        _abi.check(_abi.lib().kbg_node_state_get(self.handle, n, ctypes.byref(st)))
        return st

    def stats(self):
        st = _abi.kbg_stats()
        _abi.check(_abi.lib().kbg_stats_get(self.handle, ctypes.byref(st)))
        return st

    def close(self):
        if self.handle:
            _abi.lib().kbg_session_close(self.handle)
            self.handle = ctypes.c_void_p()


def open_session(cache, tiers, options=None, reasons=False):
    return Session(cache, tiers, options, reasons=reasons)


def close_session(ssn):
    ssn.close()
