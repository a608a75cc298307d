"""Queue and job names that return to a resident session: the hand-made
cases, a seeded generator and the truth of every round, computed from the
Python cache mirror alone (update_events.replay; kbgpu/cache.py).

The reference's deleteQueue only removes sc.Queues[uid] (event_handlers.go:
649-654) and Snapshot() filters the jobs by queue (cache.go:584-588);
deletePodGroup keeps the JobInfo and its tasks (event_handlers.go:366-380,
cache.go:476-506) and setPodGroup finds it again (:344-358). So a name that
returns brings back what a resident session dropped when it left. The session
does not adopt such jobs: it must refuse the batch (KBG_E_UNSUPPORTED; the
wrapper's re-open ValueError), and must accept every other one and equal a
fresh session on the replayed cache.

Shared by tests/test_revival_ref.py (the truth itself), test_revival_host.py
(tool library), test_revival_hostsim.py (sessions on the simulated stream) and
test_revival_gpu.py. The generator lives here and not in kbgpu/synth.py:
synth.structural's draws stay as they are."""
import random
from types import SimpleNamespace

from update_events import _gang, _namespaces, _pg, _pod, _two_queues, _with_pdb, fixture_after, replay

SET_KINDS = ("pod_group_add", "pod_group_update", "pdb_add", "pdb_update")
QUEUE_KINDS = ("queue_add", "queue_update", "namespace_add", "namespace_update")
WATCHED = SET_KINDS + QUEUE_KINDS + ("pod_group_delete", "pdb_delete", "queue_delete", "namespace_delete")


# ------------------------------------------------------------------- truth
def session_jobs(cache):
    """The JobIDs of cache.Snapshot()'s jobs (cache.go:570-588), without the
    clones (a clone may panic; the job list does not depend on it)."""
    return [jid for jid, j in cache.jobs.items()
            if (j.pod_group is not None or j.pdb is not None) and j.queue in cache.queues]


def _job_of(kind, obj):
    if kind.startswith("pod_group_"):
        return f"{obj.get('namespace', '')}/{obj['name']}"
    return obj.get("controller", "")


def _queue_of(obj):
    return obj if isinstance(obj, str) else obj["name"]


def verdicts(fx0, rounds):
    """One entry per round, up to and including the first that must be
    refused: None (must be accepted) or the refusal. A round must be refused
    iff, at one of its events,
      (a) the replayed cache's snapshot gains a job with a PodGroup or PDB
          that the cache already held before, and the session did not hold it;
      (b) a PodGroup or PDB is set on a JobID for which the cache held tasks
          before while the session did not hold that job.
    The session's jobs are followed event by event (a name may leave and
    return within one batch): a job leaves them when the snapshot loses it and
    joins them when the snapshot gains it for the first time (a JobID new to
    the cache, or a JobInfo left with neither PodGroup, PDB nor tasks).
    The refusal: rule, round, event, kind, the job, the queue (queue events),
    `seen` (the job was a session job earlier, so the library saw it leave;
    otherwise only a caller that has the cache can know), and `differs`: what
    a session that naively applied the event (a queue joins empty, a job joins
    without tasks) would hold against the replayed cache's snapshot."""
    cache0 = replay(fx0, [])
    held = set(session_jobs(cache0))
    ever = set(held)
    out = []
    for r, changes in enumerate(rounds):
        refusal = None
        for k, (kind, obj) in enumerate(changes):
            if kind not in WATCHED:
                continue
            before = replay(fx0, rounds[:r] + [changes[:k]])
            after = replay(fx0, rounds[:r] + [changes[:k + 1]])
            now = session_jobs(after)
            held &= set(now)
            target = _job_of(kind, obj) if kind in SET_KINDS else None
            hit = None
            if target and target not in held and target in before.jobs and before.jobs[target].tasks:
                hit = ("b", target)
            for jid in now:
                if jid in held or hit:
                    continue
                prior = before.jobs.get(jid)
                if prior is None or (prior.pod_group is None and prior.pdb is None and not prior.tasks):
                    held.add(jid)  # new to the cache, or a JobInfo nothing hangs on
                    ever.add(jid)
                elif prior.pod_group is not None or prior.pdb is not None:
                    hit = ("a", jid)
                else:
                    hit = ("b", jid)
            if hit:
                rule, jid = hit
                naive = [j for j in now if j in held or j == target]
                counts = {j: (0 if j == target and j not in held else len(after.jobs[j].tasks)) for j in naive}
                differs = naive != now or any(counts[j] != len(after.jobs[j].tasks) for j in naive)
                refusal = SimpleNamespace(rule=rule, round=r, event=k, kind=kind, job=jid,
                                          queue=_queue_of(obj) if kind in QUEUE_KINDS else None, seen=jid in ever,
                                          differs=differs, naive_jobs=naive, jobs=now,
                                          naive_tasks=counts.get(jid), tasks=len(after.jobs[jid].tasks))
                break
        out.append(refusal)
        if refusal:
            break
    return out


# ------------------------------------------------------------ hand-written
def _three_queues():
    fx = _two_queues()
    fx["pods"] += [_pod(f"c{i}", "qc", "pgc") for i in range(1, 3)]
    fx["podGroups"].append(_pg("qc", "pgc", "qc", created=2))
    fx["queues"].append({"name": "qc", "weight": 1})
    return fx


def _waiting_job():
    """_two_queues plus a PodGroup with pods whose queue the cache does not
    hold: the job is in sc.Jobs and in no session."""
    fx = _two_queues()
    fx["pods"] += [_pod(f"c{i}", "qc", "pgc") for i in range(1, 3)]
    fx["podGroups"].append(_pg("qc", "pgc", "qc", created=2))
    return fx


def _empty_group():
    """_two_queues plus a PodGroup without pods."""
    fx = _two_queues()
    fx["podGroups"].append(_pg("qa", "pgz", "qa", created=3))
    return fx


QA, QB = {"name": "qa", "weight": 1}, {"name": "qb", "weight": 1}
PGA = _pg("qa", "pga", "qa")
PGZ = _pg("qa", "pgz", "qa", created=3)
PDBA = {"namespace": "qa", "name": "pdba", "controller": "ctl-a", "minAvailable": 1}
_CHURN = [("pod_group_update", _pg("qb", "pgb", "qb", 2, created=1)), ("pod_add", _pod("b5", "qb", "pgb"))]
_UNRELATED = [("queue_add", {"name": "qz", "weight": 2}),
              ("node_add", {"name": "n9", "allocatable": {"cpu": "2", "memory": "8Gi", "pods": "110"}})]

# name -> (fx0, rounds)
CASES = {
    # ---- queues
    "queue_same_batch": lambda: (_two_queues(), [[("queue_delete", QA), ("queue_add", QA)]]),
    "queue_next_batch": lambda: (_two_queues(), [[("queue_delete", QA)], [("queue_add", QA)]]),
    "queue_churn_between": lambda: (_two_queues(), [[("queue_delete", QA)], list(_CHURN), [("queue_add", QA)]]),
    "queue_other_weight": lambda: (_two_queues(), [[("queue_delete", QA)], [("queue_add", {"name": "qa", "weight": 3})]]),
    "queue_delete_then_update": lambda: (_two_queues(), [[("queue_delete", QA)],
                                                         [("queue_update", {"name": "qa", "weight": 2})]]),
    "namespace_delete_then_add": lambda: (_namespaces(), [[("namespace_delete", "qa")], [("namespace_add", "qa")]]),
    "two_queues_deleted_one_back": lambda: (_three_queues(), [[("queue_delete", QA), ("queue_delete", QB)],
                                                              [("queue_add", QB)]]),
    "queue_structural_between": lambda: (_two_queues(), [[("queue_delete", QA)], list(_UNRELATED), [("queue_add", QA)]]),
    "jobless_queue_back": lambda: (_gang(1), [[("queue_delete", QB)], [("queue_add", {"name": "qb", "weight": 2})]]),
    "jobless_queue_back_same_batch": lambda: (_gang(1), [[("queue_delete", QB), ("queue_add", {"name": "qb", "weight": 2})]]),
    "jobless_queue_updated_back": lambda: (_gang(1), [[("queue_delete", QB)], [("queue_update", {"name": "qb", "weight": 3})]]),
    "queue_first_time_for_waiting_job": lambda: (_waiting_job(), [[("queue_add", {"name": "qc", "weight": 1})]]),
    # ---- jobs
    "pod_group_same_batch": lambda: (_two_queues(), [[("pod_group_delete", PGA), ("pod_group_add", PGA)]]),
    "pod_group_next_batch": lambda: (_two_queues(), [[("pod_group_delete", PGA)], [("pod_group_add", PGA)]]),
    "pod_group_structural_between": lambda: (_two_queues(), [[("pod_group_delete", PGA)], list(_UNRELATED),
                                                             [("pod_group_add", PGA)]]),
    "pdb_alone_back": lambda: (_with_pdb(False), [[("pdb_delete", PDBA)], [("pdb_add", PDBA)]]),
    "pod_group_into_live_queue": lambda: (_two_queues(), [[("queue_delete", QA)],
                                                          [("pod_group_update", _pg("qa", "pga", "qb"))]]),
    "empty_pod_group_back": lambda: (_empty_group(), [[("pod_group_delete", PGZ)], [("pod_group_add", PGZ)]]),
    "empty_pod_group_back_same_batch": lambda: (_empty_group(), [[("pod_group_delete", PGZ), ("pod_group_add", PGZ)]]),
}

# The verdicts, written out: the round that must be refused and the name its
# refusal must carry, or None when every round must be accepted.
EXPECT = {
    "queue_same_batch": (0, "qa"),
    "queue_next_batch": (1, "qa"),
    "queue_churn_between": (2, "qa"),
    "queue_other_weight": (1, "qa"),
    "queue_delete_then_update": (1, "qa"),
    "namespace_delete_then_add": (1, "qa"),
    "two_queues_deleted_one_back": (1, "qb"),
    "queue_structural_between": (2, "qa"),
    "jobless_queue_back": None,
    "jobless_queue_back_same_batch": None,
    "jobless_queue_updated_back": None,
    "queue_first_time_for_waiting_job": (0, "qc"),
    "pod_group_same_batch": (0, "qa/pga"),
    "pod_group_next_batch": (1, "qa/pga"),
    "pod_group_structural_between": (2, "qa/pga"),
    "pdb_alone_back": (1, "ctl-a"),
    "pod_group_into_live_queue": (1, "qa/pga"),
    "empty_pod_group_back": None,
    "empty_pod_group_back_same_batch": None,
}
# the one refusal only a caller holding the cache can make: the job was never a session job
CALLER_ONLY = ("queue_first_time_for_waiting_job",)


def refused_name(v):
    """The name a refusal must carry: the queue of a queue event, else the JobID."""
    return v.queue or v.job


# --------------------------------------------------------------- generator
def fuzz_fixture(seed):
    from kbgpu import synth
    if seed % 3:
        return synth.random_fixture(31000 + seed)
    return synth.contended_fixture(31000 + seed, nodes=12, jobs=8, tasks=6)


def fuzz_rounds(fx0, seed):
    """1-3 rounds: synth.structural batches mixed with re-adds of names
    deleted earlier, in the same batch or in an earlier round. A third of the
    seeds (seed % 3 == 2) re-add nothing; the others return a queue or a
    PodGroup that left. The rounds end with the first that must be refused
    (the session after a refused batch is the session before it, and the
    cache has moved on: the caller re-opens)."""
    from kbgpu import synth
    rng = random.Random(seed * 6271 + 5)
    groups = {f"{g.get('namespace', '')}/{g['name']}": g for g in fx0.get("podGroups", [])}
    weights = {q["name"]: q.get("weight", 1) for q in fx0.get("queues", [])}
    n_rounds = rng.randint(1, 3)
    revive = seed % 3 != 2
    gone_q, gone_j = [], []  # queue names / PodGroups deleted so far
    rounds = []
    for r in range(n_rounds):
        cache = replay(fx0, rounds)
        jobs = session_jobs(cache)
        uids = {u for j in jobs for u in cache.jobs[j].tasks}
        queues = list(cache.queues)
        fx = fx0 if r == 0 else fixture_after(fx0, rounds)
        batch = synth.structural(fx, 100 * seed + r, set(jobs), uids, queues) if fx is not None else []
        if r == 0 and revive and not any(k in ("queue_delete", "pod_group_delete") for k, _ in batch):
            # something must leave: a queue, or a session job that only its PodGroup keeps
            only_pg = [j for j in jobs if j in groups and cache.jobs[j].pdb is None]
            if only_pg and (rng.random() < 0.5 or not queues):
                batch.insert(0, ("pod_group_delete", groups[rng.choice(only_pg)]))
            elif queues:
                batch.insert(0, ("queue_delete", {"name": rng.choice(sorted(queues))}))
        here_q = [o["name"] for k, o in batch if k == "queue_delete"]
        here_j = [o for k, o in batch if k == "pod_group_delete"]
        last = r == n_rounds - 1
        back = []
        if revive and (last or rng.random() < 0.4):
            pool_q = gone_q + (here_q if rng.random() < 0.5 or not gone_q else [])
            pool_j = gone_j + (here_j if rng.random() < 0.5 or not gone_j else [])
            pool_q = pool_q or here_q
            pool_j = pool_j or here_j
            if pool_q and (rng.random() < 0.5 or not pool_j):
                q = rng.choice(pool_q)
                kind = "queue_update" if rng.random() < 0.25 else "queue_add"
                back.append((kind, {"name": q, "weight": weights.get(q, 1) if rng.random() < 0.5 else rng.randint(1, 4)}))
            elif pool_j:
                back.append(("pod_group_add", rng.choice(pool_j)))
        if not batch and not back:
            continue
        rounds.append(batch + back)
        gone_q += here_q
        gone_j += here_j
        if verdicts(fx0, rounds)[-1] is not None:
            break
    return rounds


# Seeds chosen on the CPU: S0 opens, no reference panic along the rounds, and
# the wrapper and the library take every round that must be accepted.
# 25 of the 40 end in a round that must be refused (the name returns in the
# batch that deleted it, or one or two updates later), 15 have every round
# accepted.
SEEDS = [0, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 21, 22, 24, 26, 27,
         28, 29, 31, 32, 33, 35, 36, 38, 39, 40, 42, 44, 47, 48, 49, 50, 52, 53, 54, 55]
GPU_SEEDS = [0, 6, 11, 12, 21, 22]  # refused in round 0, 1, 2 (a job, two queues); two with every round accepted
