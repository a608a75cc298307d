"""A plain restatement of the predicates plugin's stages (predicates.go:121-201
and the vendored predicates behind it) for the per-predicate unschedulable
reasons (kbg_job_reasons, include/kbgpu.h): the fixture's nodes with the
decisions before a task's evaluation applied, walked in session order, each
visited node counted under the first stage that turns the task away.

Inputs are the fixture dict (node labels, taints, unschedulable flag; pod
selectors, node affinity, tolerations, host ports), the session's snapshot of
the Python cache mirror (which pods each node holds at open, MaxTaskNum) and
a decision log. Inter-pod (anti)affinity is not restated: a node that passes
stages 0-4 is reported as passing, and tests of fixtures that carry it use
hand-derived counts."""
import re

WHY_POD_CAP, WHY_SELECTOR, WHY_HOST_PORTS, WHY_UNSCHEDULABLE, WHY_TAINTS, WHY_POD_AFFINITY = range(6)

_NAME = re.compile(r"^([A-Za-z0-9][-A-Za-z0-9_.]*)?[A-Za-z0-9]$")
_DNS = re.compile(r"^[a-z0-9]([-a-z0-9]*[a-z0-9])?(\.[a-z0-9]([-a-z0-9]*[a-z0-9])?)*$")


def _key_ok(k):  # validation.IsQualifiedName
    parts = k.split("/")
    if len(parts) == 2:
        if not parts[0] or len(parts[0]) > 253 or not _DNS.match(parts[0]):
            return False
        name = parts[1]
    elif len(parts) == 1:
        name = parts[0]
    else:
        return False
    return 0 < len(name) <= 63 and bool(_NAME.match(name))


def _value_ok(v):  # validation.IsValidLabelValue
    return len(v) <= 63 and (v == "" or bool(_NAME.match(v)))


def _int(s):  # strconv.ParseInt(s, 10, 64)
    if not re.match(r"^[+-]?[0-9]+$", s or ""):
        return None
    v = int(s)
    return v if -(1 << 63) <= v < (1 << 63) else None


def _requirement(e):
    """labels.NewRequirement of one NodeSelectorRequirement: a matcher over a
    label dict, or None when it is invalid (the whole term is then skipped)."""
    key, op, vals = e.get("key", ""), e.get("operator", ""), list(e.get("values") or [])
    if op not in ("In", "NotIn", "Exists", "DoesNotExist", "Gt", "Lt"):
        return None
    if op in ("In", "NotIn") and not vals:
        return None
    if op in ("Exists", "DoesNotExist") and vals:
        return None
    if op in ("Gt", "Lt") and (len(vals) != 1 or _int(vals[0]) is None):
        return None
    if not _key_ok(key) or not all(_value_ok(v) for v in vals):
        return None
    if op == "In":
        return lambda ls: key in ls and ls[key] in vals
    if op == "NotIn":
        return lambda ls: key not in ls or ls[key] not in vals
    if op == "Exists":
        return lambda ls: key in ls
    if op == "DoesNotExist":
        return lambda ls: key not in ls
    bound = _int(vals[0])

    def cmp(ls):
        v = _int(ls[key]) if key in ls else None
        return v is not None and (v > bound if op == "Gt" else v < bound)
    return cmp


def _field(e):  # NodeSelectorRequirementsAsFieldSelector, one requirement
    op, vals = e.get("operator", ""), list(e.get("values") or [])
    if op not in ("In", "NotIn") or len(vals) != 1:
        return None
    key = e.get("key", "")
    if op == "In":
        return lambda fs: fs.get(key, "") == vals[0]
    return lambda fs: fs.get(key, "") != vals[0]


def selector_ok(pod, node):
    """PodMatchNodeSelector: the nodeSelector map, then the required node
    affinity terms (ORed; a term with nothing in it or an invalid requirement
    never matches)."""
    labels = node.get("labels") or {}
    sel = pod.get("nodeSelector") or {}
    if sel and all(_key_ok(k) and _value_ok(v) for k, v in sel.items()):  # an invalid entry: the selector matches everything
        if any(labels.get(k) != v or k not in labels for k, v in sel.items()):
            return False
    aff = pod.get("affinity") or {}
    na = aff.get("nodeAffinity") if isinstance(aff, dict) else None
    req = (na or {}).get("requiredDuringSchedulingIgnoredDuringExecution")
    if req is None:
        return True
    for term in req.get("nodeSelectorTerms") or []:
        exprs, fields = term.get("matchExpressions") or [], term.get("matchFields") or []
        if not exprs and not fields:
            continue
        rs = [_requirement(e) for e in exprs]
        fs = [_field(e) for e in fields]
        if any(r is None for r in rs) or any(f is None for f in fs):
            continue
        if all(r(labels) for r in rs) and all(f({"metadata.name": node["name"]}) for f in fs):
            return True
    return False


def taints_ok(pod, node):
    """PodToleratesNodeTaints: every NoSchedule / NoExecute taint tolerated."""
    def tolerates(tol, t):
        if tol.get("effect") and tol["effect"] != t.get("effect"):
            return False
        if tol.get("key") and tol["key"] != t.get("key"):
            return False
        op = tol.get("operator") or "Equal"
        if op == "Equal":
            return (tol.get("value") or "") == (t.get("value") or "")
        return op == "Exists"
    for t in node.get("taints") or []:
        if t.get("effect") not in ("NoSchedule", "NoExecute"):
            continue
        if not any(tolerates(tol, t) for tol in pod.get("tolerations") or []):
            return False
    return True


def _ports(pod):  # (ip, protocol, port) with the defaults HostPortInfo.sanitize applies
    out = []
    for c in pod.get("containers", []):
        for p in c.get("ports") or []:
            port = int(p.get("hostPort") or 0)
            if port > 0:
                out.append((p.get("hostIP") or "0.0.0.0", p.get("protocol") or "TCP", port))
    return out


def ports_ok(pod, pods_on_node):
    """PodFitsHostPorts against the ports of the pods the node holds."""
    used = [x for q in pods_on_node for x in _ports(q)]
    for ip, proto, port in _ports(pod):
        for uip, uproto, uport in used:
            if (uproto, uport) == (proto, port) and (ip == "0.0.0.0" or uip == "0.0.0.0" or uip == ip):
                return False
    return True


def pod_key(pod):
    return f"{pod.get('namespace', '')}/{pod['name']}"


def node_pods_at(snapshot_nodes, pods_by_uid, decisions, before):
    """Per node (session order) the pods it holds once decisions[:before] are
    applied: {pod key: pod}. A decision whose key the node already holds
    leaves the node as it is (node_info.go:101-106)."""
    held = [{k: t.pod for k, t in n.tasks.items()} for n in snapshot_nodes]
    index = {n.name: i for i, n in enumerate(snapshot_nodes)}
    for d in decisions[:before]:
        pod = pods_by_uid[d["task"]]
        held[index[d["node"]]].setdefault(pod_key(pod), pod)
    return held


def first_failing_stage(pod, node_obj, max_task_num, held):
    if max_task_num <= len(held):
        return WHY_POD_CAP
    if not selector_ok(pod, node_obj):
        return WHY_SELECTOR
    if not ports_ok(pod, held.values()):
        return WHY_HOST_PORTS
    if node_obj.get("unschedulable"):
        return WHY_UNSCHEDULABLE
    if not taints_ok(pod, node_obj):
        return WHY_TAINTS
    return -1


def job_reasons(fx, snapshot_nodes, decisions, task_uid, before, predicates_on=True):
    """(visited, count[6], first_node[6]) of the task evaluated after
    decisions[:before]: it was placed at decisions[before]'s node when that
    decision is its own (the walk stopped there), else it fitted nowhere."""
    pods = {p["uid"]: p for p in fx["pods"]}
    placed = before < len(decisions) and decisions[before]["task"] == task_uid
    names = [n.name for n in snapshot_nodes]
    stop = names.index(decisions[before]["node"]) if placed else len(names) - 1
    allocated_at = stop if placed and decisions[before]["kind"] == "allocate" else -1
    held = node_pods_at(snapshot_nodes, pods, decisions, before)
    count, first = [0] * 6, [-1] * 6
    for i in range(stop + 1):
        if not predicates_on or i == allocated_at:
            continue
        n = snapshot_nodes[i]
        c = first_failing_stage(pods[task_uid], n.node, n.allocatable.max_task_num, held[i])
        if c >= 0:
            if count[c] == 0:
                first[c] = i
            count[c] += 1
    return stop + 1, count, first
