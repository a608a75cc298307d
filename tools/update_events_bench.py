"""What an edit of a live PodGroup or Queue costs a resident session (GPU box):
python tools/update_events_bench.py [config] [reps]

On a BASELINE config (default C3) it opens one session and reports, as one
JSON line, the median kbg_stats.update_ms over `reps` (default 21, at least 20)
one-event batches of each kind:
  job_update    KBG_EV_JOB_UPDATE    a PodGroup's MinMember changes (in place)
  queue_set     KBG_EV_QUEUE_SET     a queue's weight changes (in place)
  queue_update  KBG_EV_QUEUE_UPDATE  updateQueue: delete + add (the session is rebuilt)
  job_add       KBG_EV_JOB_ADD       a new PodGroup (structural: the yardstick for queue_update)
beside the same session's open_ms: before these events existed a close and an
open was the only way to apply such an edit. KBG_PROFILE_OPEN=1 prints the
library's phase split of every update to stderr."""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kube-arbitrator_amd"))

from kbgpu import _abi, synth  # noqa: E402
from kbgpu.cache import FakeBinder, cache_from_fixture  # noqa: E402
from kbgpu.fixture import _OrderedCache, fixture_tiers  # noqa: E402
from kbgpu.framework import open_session  # noqa: E402


def main():
    cid = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    reps = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 21
    fx = synth.config_fixture(cid)
    groups = {f"{g.get('namespace', '')}/{g['name']}": g for g in fx["podGroups"]}
    opens = []
    for _ in range(3):  # the first open of a process also pays for the runtime's start
        ssn = open_session(_OrderedCache(cache_from_fixture(fx, FakeBinder()), fx), fixture_tiers(fx), {"device": 0})
        opens.append(ssn.stats().open_ms)
        if len(opens) < 3:
            ssn.close()
    out = {"tool": "update_events_bench", "config": f"C{cid}", "reps": reps, "nodes": len(ssn.nodes),
           "jobs": len(ssn.jobs), "tasks": len(ssn.flat.task_objs), "queues": len(ssn.queues),
           "open_ms": min(opens[1:]), "open_ms_all": opens}  # the better warm open: the yardstick at its best
    rebuilds0 = ssn.stats().update_rebuilds

    def timed(name, change_of):
        ms = []
        for r in range(reps):
            ssn.update([change_of(r)])
            ms.append(ssn.stats().update_ms)
        out[name + "_ms"] = statistics.median(ms)
        out[name + "_ms_min"] = min(ms)
        out[name + "_ms_max"] = max(ms)

    job = next(j for j in ssn.jobs if j.uid in groups)
    pg = dict(groups[job.uid], queue=job.queue)
    qname, weight, min_member = ssn.queues[0].uid, ssn.queues[0].weight, job.min_available
    # MinMember alternates between two values. The weights are sent as they are: on the over-requested
    # configs (C3) any other weight makes the reference's own water-fill panic (remaining.Sub(deserved),
    # proportion.go:140), which the library reports as KBG_E_REF_PANIC; the library does the
    # same work for a QUEUE_SET / QUEUE_UPDATE whatever the weight (the derive recomputes every queue)
    timed("job_update", lambda r: ("pod_group_update", dict(pg, minMember=min_member + 1 - r % 2)))
    timed("queue_set", lambda r: ("queue_add", {"name": qname, "weight": weight}))
    out["in_place_rebuilds"] = ssn.stats().update_rebuilds - rebuilds0  # 0: neither kind rebuilt the session
    timed("queue_update", lambda r: ("queue_update", {"name": qname, "weight": weight}))
    timed("job_add", lambda r: ("pod_group_add", {"namespace": "bench", "name": f"pg-added-{r}", "minMember": 1,
                                                  "queue": qname, "creationTimestamp": 10 ** 12 + r}))
    out["rebuilds"] = ssn.stats().update_rebuilds - rebuilds0
    # the cycle after them still runs (the session is usable): its status
    buf = (_abi.kbg_decision * max(1, len(ssn.flat.task_objs)))()
    n = ctypes.c_int32(0)
    out["allocate_status"] = _abi.STATUS_NAMES.get(_abi.lib().kbg_allocate(ssn.handle, buf, len(buf), ctypes.byref(n)))
    out["decisions"] = n.value
    ssn.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
