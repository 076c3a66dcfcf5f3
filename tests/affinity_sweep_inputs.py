"""Inputs and CPU oracles of the scenario sweep over inter-pod affinity queues (ksim_sweep_affinity),
shared by tests/test_sweep_affinity_host.py (their properties) and tests/test_gpu_sweep_affinity.py
(the GPU cases), on the pattern of tests/spread_sweep_inputs.py.

Every oracle works on objects: the nodes without the absent ones, the running pods without those
bound to them, ingested anew — ksim_ref.simulate for the small inputs (`oracle_ref`), cpu_ref.run on
the reduced cluster's own plan for the large ones and for histograms (`oracle_cpu`) — and node names
mapped back to the ranks of the loaded table.  A queue is a list of pods in scheduling order; the
simulator pops its list from the end, so it is fed the reverse."""
import copy
import functools
import random

import numpy as np

import cpu_ref
import ksim_ref as R
import spread_sweep_inputs as X
from ksim import abi, ingest, scheduler, spread, synth
from workloads import rnd_affinity_workload, rnd_spread_workload

ZONE = "zone"  # the topology label of workloads.rnd_affinity_nodes
DEFAULT = scheduler.provider("DefaultProvider")
RND_SIZES = [(18, 60, 18), (70, 90, 70), (130, 120, 130)]  # (nodes, queued pods, running pods)
INTERPOD_REASONS = (abi.R_EXISTING_ANTI, abi.R_AFFINITY_RULES, abi.R_ANTI_AFFINITY_RULES)


class Input:
    """nodes, running pods, queue (scheduling order), lister objects or None; cluster() ingests them."""

    def __init__(self, nodes, running, queue, objs=None, policy=DEFAULT):
        self.nodes, self.running, self.queue, self.objs = list(nodes), list(running), list(queue), objs
        self.policy = policy
        self._cl = {}

    def listers(self):
        return spread.SpreadListers(**self.objs) if self.objs else None

    def cluster(self, extra=()):
        """The loaded cluster; extra: pods appended to the queue (the drain copies)."""
        key = len(extra)
        if key not in self._cl:
            self._cl[key] = ingest.Cluster.from_objects(self.nodes, self.running, self.queue + list(extra),
                                                        spread=self.listers())
        return self._cl[key]


def sets_of(cl, zone=ZONE):
    """(label, absent node ranks): none, the first and last node, each value of the zone label."""
    n = cl.n_nodes
    out = [("none", []), ("first", [0]), ("last", [n - 1])]
    return out + [("zone-" + v, list(idx)) for v, idx in scheduler.outage_sets(cl, zone)]


def oracle_ref(inp, absent, queue=None, bound=(), counter=0, policy=None):
    """ksim_ref.simulate of `queue` (default: the input's) on the reduced snapshot: dict(out — ranks
    of the loaded table, -1 failed —, counter, listed, names, msgs [(pod name, FitError text)])."""
    cl = inp.cluster()
    queue = inp.queue if queue is None else queue
    preds, prios = policy or inp.policy
    left, stay = X._reduced(inp, cl, absent, bound)
    names = [x["metadata"]["name"] for x in queue]
    lst = R.SpreadListers(**inp.objs) if inp.objs else None
    want, lni = R.simulate(left, stay, list(reversed(queue)), set(preds), list(prios), spread=lst, last_node_index=counter)
    assert [nm for nm, _, _ in want] == names
    out = np.array([cl.index[h] if h is not None else -1 for _, h, _ in want], np.int32)
    return dict(out=out, counter=lni, listed=len(left), names=names, msgs=[(nm, m) for nm, h, m in want if h is None])


def oracle_cpu(inp, absent, queue=None):
    """cpu_ref.run on the plan of the reduced objects: dict(out, counter, listed, count, pod, hist)."""
    cl = inp.cluster()
    queue = inp.queue if queue is None else queue
    preds, prios = inp.policy
    left, stay = X._reduced(inp, cl, absent)
    m = len(queue)
    sub = ingest.Cluster.from_objects(left, stay, queue, spread=inp.listers())
    pl = scheduler.plan(sub, preds, prios)
    ref, reasons, _, ctr, _ = cpu_ref.run(sub, None, 0, m, threads=8, plan=pl)
    back = np.array([cl.index[nm] for nm in sub.names], np.int32)
    failed = np.nonzero(ref < 0)[0].astype(np.int32)
    return dict(out=np.where(ref >= 0, back[np.maximum(ref, 0)], -1).astype(np.int32), counter=ctr, listed=len(left),
                count=len(failed), pod=failed, hist=np.ascontiguousarray(reasons[failed]))


def lost_affinity_pods(inp, absent):
    """Running pods with inter-pod affinity terms on the absent nodes."""
    cl = inp.cluster()
    gone = {cl.names[i] for i in absent}
    return sum(1 for x in inp.running if x["spec"].get("affinity") and x["spec"]["nodeName"] in gone)


# ---- 1. the four three-node cases: zone-keyed required terms under a zone or node outage
def _node(name, zone, cpu):
    return {"metadata": {"name": name, "labels": {ZONE: zone, "kubernetes.io/hostname": name}}, "spec": {},
            "status": {"allocatable": {"cpu": cpu, "memory": "16Gi", "pods": "110"},
                       "conditions": [{"type": "Ready", "status": "True"}]}}


def _pod(name, app, cpu="1", node=None, affinity=None):
    pod = {"metadata": {"name": name, "namespace": "default", "labels": {"app": app}},
           "spec": {"containers": [{"resources": {"requests": {"cpu": cpu, "memory": "256Mi"}}}]}}
    if node:
        pod["spec"]["nodeName"] = node
    if affinity:
        pod["spec"]["affinity"] = affinity
    return pod


def _term(kind, app):
    return {kind: {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": ZONE}]}}


# case: (running pod, queue pod, outage node, the reference's node for q or None, the answer of a sweep
# whose counts still hold the lost pod)
HAND = {
    "own-anti-affinity": (_pod("r", "db", node="a1"), _pod("q", "web", affinity=_term("podAntiAffinity", "db")),
                          "a1", "a2", None),
    "existing-anti-affinity": (_pod("r", "db", node="a1", affinity=_term("podAntiAffinity", "web")), _pod("q", "web"),
                               "a1", "a2", None),
    "own-affinity": (_pod("r", "db", node="a1"), _pod("q", "web", affinity=_term("podAffinity", "db")),
                     "a1", None, "a2"),
    "self-match-waiver": (_pod("r", "db", cpu="100m", node="b1"), _pod("q", "db", affinity=_term("podAffinity", "db")),
                          "b1", "a2", None),
}


@functools.lru_cache(maxsize=None)
def hand_input(case):
    """Nodes a1, a2 in zone A with 4 cpu each, b1 in zone B with 500m: too small for the 1-cpu queue pod."""
    r, q, _, _, _ = HAND[case]
    nodes = [_node("a1", "A", "4"), _node("a2", "A", "4"), _node("b1", "B", "500m")]
    return Input(nodes, [copy.deepcopy(r)], [copy.deepcopy(q)])


def hand_sets(case):
    """An outage of nothing, then the case's outage."""
    cl = hand_input(case).cluster()
    return [("none", []), ("outage", [cl.index[HAND[case][2]]])]


# ---- 2. the random workloads
@functools.lru_cache(maxsize=None)
def rnd_input(n_nodes, seed=1):
    _, n_pods, n_running = next(t for t in RND_SIZES if t[0] == n_nodes)
    nodes, running, pods = rnd_affinity_workload(seed, n_nodes, n_pods, n_running)
    return Input(nodes, running, pods)


@functools.lru_cache(maxsize=None)
def rnd_refs(n_nodes):
    """(input, sets, cpu_ref answers with histograms) of one random workload, once."""
    inp = rnd_input(n_nodes)
    sets_ = sets_of(inp.cluster())
    return inp, sets_, [oracle_cpu(inp, a) for _, a in sets_]


def without_priority(inp, name="InterPodAffinityPriority"):
    preds, prios = inp.policy
    return Input(inp.nodes, inp.running, inp.queue, inp.objs, (preds, [(n, w) for n, w in prios if n != name]))


# ---- 3. two rows per thread
@functools.lru_cache(maxsize=None)
def wide_refs():
    nodes, running, pods = rnd_affinity_workload(1, 1100, 60, 300)
    inp = Input(nodes, running, pods)
    sets_ = sets_of(inp.cluster())
    sets_ = [s for s in sets_ if s[0] in ("none", "first")] + [s for s in sets_ if s[0].startswith("zone-")][:2]
    return inp, sets_, [oracle_cpu(inp, a) for _, a in sets_]


# ---- 4. the node cap
@functools.lru_cache(maxsize=None)
def caps_input(n=abi.SWEEP_GENERAL_MAX_NODES, zones=64, p=40):
    """n equal nodes in `zones` zones; one service whose replicas repel each other per hostname and
    prefer other zones, twelve of them running."""
    anti = {"podAntiAffinity": {
        "requiredDuringSchedulingIgnoredDuringExecution": [
            {"labelSelector": {"matchLabels": {"app": "a"}}, "topologyKey": "kubernetes.io/hostname"}],
        "preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 50, "podAffinityTerm": {"labelSelector": {"matchLabels": {"app": "a"}}, "topologyKey": ZONE}}]}}
    nodes = [_node("k-%05d" % i, "z%03d" % (i % zones), "8") for i in range(n)]
    running = [_pod("run-%d" % k, "a", node="k-%05d" % ((k * 911) % n), affinity=anti) for k in range(12)]
    queue = [_pod("q-%d" % k, "a", affinity=anti) for k in range(p)]
    return Input(nodes, running, queue)


# ---- 4b. more zones than a swept SelectorSpread queue may have, and no spread pair
HOST_ANTI = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
    {"labelSelector": {"matchLabels": {"app": "a"}}, "topologyKey": "kubernetes.io/hostname"}]}}


@functools.lru_cache(maxsize=None)
def many_zones_input(zones=abi.SWEEP_SPREAD_MAX_ZONES + 8, p=60):
    """Two 2-cpu nodes per zone of the well-known zone label, no listers (no class has a spread pair); the
    replicas of app a repel each other per zone (required) and those of app b prefer zones without b;
    forty pods are running, so the queue's 1-cpu pods meet occupied zones and full nodes."""
    n = 2 * zones
    nodes = [_node("m-%04d" % i, "unused", "2") for i in range(n)]
    for i, x in enumerate(nodes):
        x["metadata"]["labels"] = {X.ZONE: "z%04d" % (i // 2), "kubernetes.io/hostname": x["metadata"]["name"]}

    def aff(app):
        t = {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": X.ZONE}
        return {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [t]} if app == "a" else
                {"preferredDuringSchedulingIgnoredDuringExecution": [{"weight": 40, "podAffinityTerm": t}]}}
    running = [_pod("run-%d" % k, "ab"[k % 2], node="m-%04d" % ((k * 53) % n), affinity=aff("ab"[k % 2])) for k in range(40)]
    queue = [_pod("q-%d" % k, "ab"[k % 2], affinity=aff("ab"[k % 2])) for k in range(p)]
    return Input(nodes, running, queue)


# ---- 5. affinity and SelectorSpread together
@functools.lru_cache(maxsize=None)
def spread_input(n_nodes=70, n_pods=90):
    """workloads.rnd_spread_workload with its listers; every third queued pod and every fourth running
    pod also repels, per zone or hostname, the pods that carry its own labels."""
    nodes, running, pods, objs = rnd_spread_workload(1, n_nodes=n_nodes, n_pods=n_pods, n_running=n_nodes, zones=True)
    running, pods = copy.deepcopy(running), copy.deepcopy(pods)
    rng = random.Random(5)
    for k, x in enumerate(running + pods):
        lab = (x["metadata"].get("labels") or {})
        if not lab or k % (4 if k < len(running) else 3):
            continue
        key = rng.choice([X.ZONE, "kubernetes.io/hostname"])
        kind = "requiredDuringSchedulingIgnoredDuringExecution" if rng.random() < 0.4 else \
            "preferredDuringSchedulingIgnoredDuringExecution"
        t = {"labelSelector": {"matchLabels": dict(lab)}, "topologyKey": key}
        x["spec"]["affinity"] = {"podAntiAffinity": {kind: [t] if kind.startswith("required") else
                                                     [{"weight": rng.randint(1, 100), "podAffinityTerm": t}]}}
    return Input(nodes, running, pods, objs)


# ---- 6. several reduce classes together with affinity
@functools.lru_cache(maxsize=None)
def classes_input(n=1500, p=200):
    """synth.c2_objects (taints and tolerations: several TaintToleration classes), nodes in four zones,
    pods labelled app=a|b|c; every other pod repels its own app per hostname and prefers its zone."""
    nodes, pods = synth.c2_objects(n, p, seed=7)
    nodes, pods = copy.deepcopy(nodes), copy.deepcopy(pods)
    rng = random.Random(77)
    for x in nodes:
        x["metadata"]["labels"]["kubernetes.io/hostname"] = x["metadata"]["name"]
        if rng.random() < 0.8:
            x["metadata"]["labels"][ZONE] = "z%d" % rng.randint(1, 4)
    for k, x in enumerate(pods):
        app = rng.choice("abc")
        x["metadata"]["labels"] = {"app": app}
        if k % 2 == 0:
            sel = {"matchLabels": {"app": app}}
            x["spec"]["affinity"] = {
                "podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
                    {"labelSelector": sel, "topologyKey": "kubernetes.io/hostname"}]},
                "podAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                    {"weight": 30, "podAffinityTerm": {"labelSelector": sel, "topologyKey": ZONE}}]}}
    return Input(nodes, [], pods)


# ---- 7. prefix queues: per outage the evictable running pods of its nodes, re-queued
def drain_plan(inp, sets_):
    """(copies appended to the queue, per set the loaded-queue indices of its copies, per set the
    scenario's own queue as objects): running pods in their order, those on a node of some set."""
    cl = inp.cluster()
    lost = set().union(*[set(a) for _, a in sets_]) if sets_ else set()
    evicted = [(cl.index[x["spec"]["nodeName"]], x) for x in inp.running
               if cl.index[x["spec"]["nodeName"]] in lost and scheduler.default_evictable(x)]
    copies = [scheduler.requeue_copy(x) for _, x in evicted]
    nq = len(inp.queue)
    requeue = [[nq + k for k, (w, _) in enumerate(evicted) if w in set(a)] for _, a in sets_]
    return copies, requeue, [[copies[q - nq] for q in rq] for rq in requeue]
