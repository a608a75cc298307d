"""Hand-derived known-answer fixture for kbg_job_fit
(tests/golden/kat_job_fit.json, checked by tests/test_hostsim_job_fit.py and
tests/test_job_fit_gpu.py). Every expected value below was derived by reading
the cited reference code, not by running any implementation.

Run: python tests/golden/make_kat_job_fit.py

The cluster is kat_headroom.json's (tests/golden/make_kat_headroom.py): m0 and
m1 in zone a, m2 and m3 in zone b, 5000m each; w0 (app=web, host port
8080/TCP, 1000m) runs on m0 and d0 (app=db, 1000m) on m2, so Idle is 4000m,
5000m, 4000m, 5000m, Releasing 0, and no pod cap is near. The session has host
ports and pod affinity: host_job_fit answers, and the row carries
affinity_now = 1. Job A (MinMember 3) at open, its pods in UID order, each to
the first node in index order that passes the predicates against the job's
view and has Resreq.LessEqual(Idle) (allocate.go:119-162):
  a0-port  1000m, hostPort 8080: m0 holds the port (predicates.go:143-155);
           m1 -> Allocate, m1 at 4000m and the port now used there in the view.
  a1-port  1000m, hostPort 8080: m0 holds it, m1 holds it in the view;
           m2 -> Allocate, m2 at 3000m.
  a2-aff   3000m, podAffinity app=web over the zone: zone a passes (w0), the
           verdict of now; m0 4000m -> Allocate, m0 at 1000m.
  a3-aff   the same: m0 1000m short; m1 4000m -> Allocate, m1 at 1000m.
  a4-aff   the same: m0 and m1 hold 1000m, zone b fails the term: nowhere.
  a5-anti  4000m, podAntiAffinity app=db over the host: m0, m1 short, m2 holds
           d0; m3 5000m -> Allocate.
Five of six on Idle, four nodes; the third placement is step 3: ready after 3.
At limit 2 the walk is a0-port and a1-port alone: two placed, MinMember 3 not
reached, nothing unplaced, four pods not walked."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def pod(uid, cpu, ports=None, affinity=None):
    c = {"requests": {"cpu": cpu}}
    if ports:
        c["ports"] = ports
    p = {"uid": uid, "namespace": "ns", "name": uid, "phase": "Pending", "nodeName": "",
         "annotations": {"scheduling.k8s.io/group-name": "A"}, "containers": [c], "labels": {"app": "client"}}
    if affinity:
        p["affinity"] = affinity
    return p


def term(app, key):
    return {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": key}]}


def main():
    with open(os.path.join(HERE, "kat_headroom.json")) as f:
        base = json.load(f)
    port = [{"hostPort": 8080, "protocol": "TCP"}]
    aff = {"podAffinity": term("web", "zone")}
    pods = [pod("a0-port", "1", ports=port), pod("a1-port", "1", ports=port), pod("a2-aff", "3", affinity=aff),
            pod("a3-aff", "3", affinity=aff), pod("a4-aff", "3", affinity=aff),
            pod("a5-anti", "4", affinity={"podAntiAffinity": term("db", "host")})]
    pods += [p for p in base["pods"] if p["phase"] == "Running"]
    groups = [dict(g, name="A", minMember=3) if g["name"] == "P" else g for g in base["podGroups"]]
    common = dict(job="ns/A", pending=6, ready_num=0, min_available=3, queue_overused=False, affinity_now=True,
                  panic_nodes=0, placed_releasing=0)
    full = dict(common, limit=512, walked=6, placed_idle=5, first_unplaced="a4-aff", nodes_used=4, ready_after=3,
                places=[["a0-port", "m1", "allocate"], ["a1-port", "m2", "allocate"], ["a2-aff", "m0", "allocate"],
                        ["a3-aff", "m1", "allocate"], ["a4-aff", None, None], ["a5-anti", "m3", "allocate"]],
                message="needs 3 more; 5 of its next 6 pending pods fit now (5 on idle, 0 on releasing resources, "
                        "4 nodes): enough after pod 3 (pod affinity as it is now)")
    cut = dict(common, limit=2, walked=2, placed_idle=2, first_unplaced=None, nodes_used=2, ready_after=-1,
               places=[["a0-port", "m1", "allocate"], ["a1-port", "m2", "allocate"]],
               message="needs 3 more; 2 of its next 2 pending pods fit now (2 on idle, 0 on releasing resources, "
                       "2 nodes): not enough, 4 not walked (pod affinity as it is now)")
    fx = dict(name="kat_job_fit", actions=["allocate"], tiers=base["tiers"], nodes=base["nodes"], queues=base["queues"],
              podGroups=groups, pods=pods, expected={"job_fit": [full, cut]})
    with open(os.path.join(HERE, "kat_job_fit.json"), "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
