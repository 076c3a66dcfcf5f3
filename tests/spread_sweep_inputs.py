"""Inputs and CPU oracles of the scenario sweep over SelectorSpread queues, shared by
tests/test_sweep_spread_host.py (their properties) and tests/test_gpu_sweep_spread.py (the GPU cases).

Every oracle works on objects: the nodes without the absent ones, the running pods without those
bound to them, the same listers, ingested anew — ksim_ref.simulate for the small inputs (`ref`),
cpu_ref.run on the reduced cluster's own plan for the large ones and for histograms (`cpu`) — and
node names mapped back to the ranks of the loaded table.  A queue is a list of pods in scheduling
order; the simulator pops its list from the end, so it is fed the reverse."""
import copy
import functools
import random

import numpy as np

import cpu_ref
import ksim_ref as R
from ksim import abi, ingest, scheduler, spread, synth
from workloads import rnd_spread_workload

ZONE = "failure-domain.beta.kubernetes.io/zone"

POLICIES = {  # those of tests/test_gpu_spread.py
    "default": scheduler.provider("DefaultProvider"),
    "service_spreading": (["GeneralPredicates"], [("ServiceSpreadingPriority", 2), ("LeastRequestedPriority", 1)]),
    "spread_heavy": (["GeneralPredicates", "PodToleratesNodeTaints"],
                     [("SelectorSpreadPriority", 5), ("BalancedResourceAllocation", 1)]),
}
RND_SIZES = [(18, 60), (70, 90), (130, 120)]  # (nodes, queued pods): one, two and three waves with rows


class Input:
    """nodes, running pods, queue (scheduling order), lister objects; cluster() ingests them."""

    def __init__(self, nodes, running, queue, objs, services_only=False):
        self.nodes, self.running, self.queue, self.objs = list(nodes), list(running), list(queue), objs
        self.services_only = services_only
        self._cl = {}

    def listers(self, with_listers=True):
        return spread.SpreadListers(**self.objs) if with_listers else None

    def cluster(self, with_listers=True, extra=()):
        """The loaded cluster; extra: pods appended to the queue (the drain copies)."""
        key = (with_listers, len(extra))
        if key not in self._cl:
            self._cl[key] = ingest.Cluster.from_objects(self.nodes, self.running, self.queue + list(extra),
                                                        spread=self.listers(with_listers),
                                                        spread_services_only=self.services_only)
        return self._cl[key]


def for_policy(inp, policy):
    """ServiceSpreadingPriority alone reads the services only (ClusterCapacity derives the same flag)."""
    names = {n for n, _ in POLICIES[policy][1]}
    only = "ServiceSpreadingPriority" in names and "SelectorSpreadPriority" not in names
    if only == inp.services_only:
        return inp
    return Input(inp.nodes, inp.running, inp.queue, inp.objs, services_only=only)


def sets_of(cl):
    """(label, absent node ranks): none, the first and last node, each zone as a whole, every zoned
    node (haveZones turns false in that scenario only), every node."""
    n = cl.n_nodes
    out = [("none", []), ("first", [0]), ("last", [n - 1])]
    zones = scheduler.outage_sets(cl, ZONE)
    out += [("zone-" + v, list(idx)) for v, idx in zones]
    if zones:
        out.append(("all-zoned", sorted(i for _, idx in zones for i in idx)))
    out.append(("every-node", list(range(n))))
    return out


def _reduced(inp, cl, absent, bound=()):
    """(nodes left, running pods left) of an absent set; bound: (pod, node rank) commits made since
    the snapshot (a schedule() of a prefix), kept as running pods unless their node is absent."""
    gone = {cl.names[i] for i in absent}
    left = [x for x in inp.nodes if x["metadata"]["name"] not in gone]
    stay = [x for x in inp.running if (x.get("spec") or {}).get("nodeName") not in gone]
    for pod, w in bound:
        if cl.names[w] not in gone:
            pod = copy.deepcopy(pod)
            pod["spec"]["nodeName"] = cl.names[w]
            stay.append(pod)
    return left, stay


def oracle_ref(inp, policy, absent, queue=None, with_listers=True, bound=(), counter=0):
    """ksim_ref.simulate of `queue` (default: the input's) on the reduced snapshot: dict(out — ranks
    of the loaded table, -1 failed —, counter, listed, names, msgs [(pod name, FitError text)])."""
    cl = inp.cluster()
    queue = inp.queue if queue is None else queue
    preds, prios = POLICIES[policy]
    left, stay = _reduced(inp, cl, absent, bound)
    names = [x["metadata"]["name"] for x in queue]
    if not left:
        from ksim.report import ERR_NO_NODES
        return dict(out=np.full(len(queue), -1, np.int32), counter=counter, listed=0, names=names,
                    msgs=[(nm, ERR_NO_NODES) for nm in names])
    lst = R.SpreadListers(**inp.objs) if with_listers else None
    want, lni = R.simulate(left, stay, list(reversed(queue)), set(preds), list(prios), spread=lst, last_node_index=counter)
    assert [nm for nm, _, _ in want] == names
    out = np.array([cl.index[h] if h is not None else -1 for _, h, _ in want], np.int32)
    return dict(out=out, counter=lni, listed=len(left), names=names, msgs=[(nm, m) for nm, h, m in want if h is None])


def oracle_cpu(inp, policy, absent, queue=None, with_listers=True):
    """cpu_ref.run on the plan of the reduced objects: dict(out, counter, listed, count, pod, hist)."""
    cl = inp.cluster()
    queue = inp.queue if queue is None else queue
    preds, prios = POLICIES[policy]
    left, stay = _reduced(inp, cl, absent)
    m = len(queue)
    if not left:
        return dict(out=np.full(m, -1, np.int32), counter=0, listed=0, count=m, pod=np.arange(m, dtype=np.int32),
                    hist=np.zeros((m, abi.NREASONS), np.int32))
    sub = ingest.Cluster.from_objects(left, stay, queue, spread=inp.listers(with_listers),
                                      spread_services_only=inp.services_only)
    pl = scheduler.plan(sub, preds, prios)
    ref, reasons, _, ctr, _ = cpu_ref.run(sub, None, 0, m, threads=8, plan=pl)
    back = np.array([cl.index[nm] for nm in sub.names], np.int32)
    failed = np.nonzero(ref < 0)[0].astype(np.int32)
    return dict(out=np.where(ref >= 0, back[np.maximum(ref, 0)], -1).astype(np.int32), counter=ctr, listed=len(left),
                count=len(failed), pod=failed, hist=np.ascontiguousarray(reasons[failed]))


# ---- 1. the random workloads
@functools.lru_cache(maxsize=None)
def rnd_input(n_nodes, zones, seed=1):
    n_pods = dict(RND_SIZES)[n_nodes]
    nodes, running, pods, objs = rnd_spread_workload(seed, n_nodes=n_nodes, n_pods=n_pods, n_running=n_nodes, zones=zones)
    return Input(nodes, running, pods, objs)


@functools.lru_cache(maxsize=None)
def rnd_refs(n_nodes, zones, policy, with_listers=True):
    """(input, sets, ksim_ref answers) of one random workload under one policy, once."""
    inp = for_policy(rnd_input(n_nodes, zones), policy)
    sets_ = sets_of(inp.cluster())
    return inp, sets_, [oracle_ref(inp, policy, a, with_listers=with_listers) for _, a in sets_]


# ---- 2. segment geometry: wide ties on a uniform cluster
def _node(name, zone=None, cpu="8", mem="32Gi", pods="110"):
    lab = {ZONE: zone} if zone else {}
    return {"metadata": {"name": name, "labels": lab}, "spec": {},
            "status": {"allocatable": {"cpu": cpu, "memory": mem, "pods": pods},
                       "conditions": [{"type": "Ready", "status": "True"}]}}


def _pod(name, labels, cpu="500m", mem="1Gi", ns="default"):
    return {"metadata": {"name": name, "namespace": ns, "labels": dict(labels)},
            "spec": {"containers": [{"resources": {"requests": {"cpu": cpu, "memory": mem}}}]}}


@functools.lru_cache(maxsize=None)
def uniform_input(n, p=300):
    """n equal nodes, every tenth without a zone and the others in z1..z3 by turns; one service that
    selects every pod: the scores tie over whole zones, so lastNodeIndex % C walks the segments."""
    nodes = [_node("u-%05d" % i, None if i % 10 == 9 else "z%d" % (1 + i % 3)) for i in range(n)]
    running = [dict(_pod("run-%d" % k, {"app": "a"}), spec=dict(_pod("x", {})["spec"], nodeName="u-%05d" % ((k * 37) % n)))
               for k in range(20)]
    queue = [_pod("q-%d" % k, {"app": "a"}) for k in range(p)]
    objs = dict(services=[{"metadata": {"namespace": "default", "name": "svc"}, "spec": {"selector": {"app": "a"}}}],
                rcs=[], rss=[], sss=[])
    return Input(nodes, running, queue, objs)


@functools.lru_cache(maxsize=None)
def uniform_refs(n, with_listers=True):
    inp = uniform_input(n)
    sets_ = sets_of(inp.cluster())
    return inp, sets_, [oracle_cpu(inp, "default", a, with_listers=with_listers) for _, a in sets_]


# ---- 3. several reduce classes together with spread
@functools.lru_cache(maxsize=None)
def classes_input(n=1500, p=600):
    """synth.c2_objects (taints and tolerations: several TaintToleration classes) with the pods
    labelled app=a|b|c, nodes in four zones (a fifth of them in none) and two services."""
    nodes, pods = synth.c2_objects(n, p, seed=7)
    nodes, pods = copy.deepcopy(nodes), copy.deepcopy(pods)
    rng = random.Random(77)
    for x in nodes:
        if rng.random() < 0.8:
            x["metadata"]["labels"][ZONE] = "z%d" % rng.randint(1, 4)
    for x in pods:
        x["metadata"]["labels"] = {"app": rng.choice("abc")}
    objs = dict(services=[{"metadata": {"namespace": "default", "name": "sa"}, "spec": {"selector": {"app": "a"}}},
                          {"metadata": {"namespace": "default", "name": "sb"}, "spec": {"selector": {"app": "b"}}}],
                rcs=[], rss=[], sss=[])
    return Input(nodes, [], pods, objs)


def max_reduce_classes(cl, policy="default"):
    """The largest K = TaintToleration classes x NodeAffinity classes over the queued pods' classes."""
    preds, prios = POLICIES[policy]
    pl = scheduler.plan(cl, preds, prios)
    w = scheduler.make_config(preds, prios).weights
    use_na = bool(w[abi.W_NODE_AFF]) or pl.na_add is not None
    k = 1
    for c in np.unique(np.asarray(pl.pods)["cls"]):
        k1 = int(pl.tables["n_tt"][c]) if w[abi.W_TAINT_TOL] else 1
        k2 = int(pl.tables["n_na"][c]) if use_na else 1
        k = max(k, k1 * k2)
    return k


@functools.lru_cache(maxsize=None)
def classes_refs(with_listers=True):
    inp = classes_input()
    cl = inp.cluster()
    sets_ = [s for s in sets_of(cl) if s[0] in ("none", "first", "zone-z2", "all-zoned")]
    return inp, sets_, [oracle_cpu(inp, "default", a, with_listers=with_listers) for _, a in sets_]


# ---- 4. fit nodes only: a queue that overflows the cluster
@functools.lru_cache(maxsize=None)
def overflow_input():
    """24 nodes in three zones (four in none), three of 2000m cpu and the others of 2500m; 30 running
    100m pods of the one service, ten on each of the three; the queue, all of the service: 50 1-cpu
    pods, which overflow the cluster, then 600m pods, which fit nowhere any more, between 100m pods,
    which still bind.  The three nodes are full after one 1-cpu pod, with the highest counts by far."""
    nodes = [_node("o-%02d" % i, None if i % 6 == 5 else "z%d" % (1 + i % 3), cpu="2000m" if i in (0, 4, 8) else "2500m", mem="8Gi")
             for i in range(24)]
    running = [dict(_pod("run-%d" % k, {"app": "a"}, cpu="100m", mem="64Mi"),
                    spec=dict(_pod("x", {}, cpu="100m", mem="64Mi")["spec"], nodeName="o-%02d" % (4 * (k % 3)))) for k in range(30)]
    queue = [_pod("big-%d" % k, {"app": "a"}, cpu="1", mem="64Mi") for k in range(50)]
    queue += [_pod("mid-%d" % k, {"app": "a"}, cpu="600m", mem="64Mi") if k % 3 == 0 else _pod("small-%d" % k, {"app": "a"}, cpu="100m", mem="64Mi")
              for k in range(40)]
    objs = dict(services=[{"metadata": {"namespace": "default", "name": "svc"}, "spec": {"selector": {"app": "a"}}}],
                rcs=[], rss=[], sss=[])
    return Input(nodes, running, queue, objs)


def _mcpu(pod):
    req = pod["spec"]["containers"][0]["resources"]["requests"]["cpu"]
    return int(req[:-1]) if req.endswith("m") else 1000 * int(req)


def overflow_conditions(inp, ref, absent=()):
    """(pods of the service bound after the first failure, bound pods behind a failure for which some
    node that no longer fits them holds more pods of the service than every node that does), in the
    reference's answer `ref` for the absent set."""
    cl = inp.cluster()
    cpu = {cl.index[x["metadata"]["name"]]: int(x["status"]["allocatable"]["cpu"][:-1]) for x in inp.nodes}
    for i in absent:
        del cpu[i]
    cnt = dict.fromkeys(cpu, 0)
    for x in inp.running:
        w = cl.index[x["spec"]["nodeName"]]
        if w in cpu:
            cpu[w] -= _mcpu(x)
            cnt[w] += 1
    first_fail = int(np.nonzero(ref["out"] < 0)[0][0])
    after = full_higher = 0
    for k, (pod, w) in enumerate(zip(inp.queue, ref["out"])):
        need = _mcpu(pod)
        if w >= 0 and k > first_fail:
            after += 1
            fit = [i for i in cpu if cpu[i] >= need]
            full = [i for i in cpu if cpu[i] < need]
            if full and max(cnt[i] for i in full) > max(cnt[i] for i in fit):
                full_higher += 1
        if w >= 0:
            cpu[int(w)] -= need
            cnt[int(w)] += 1
    return after, full_higher


# ---- 5. first pod of a service, and a pod no selector matches
@functools.lru_cache(maxsize=None)
def first_pod_input():
    """No running pod: the first pod of the service sees count 0 everywhere (max_node == 0, every
    spread score 10); every third pod carries labels no selector matches (no spread pair)."""
    inp = rnd_input(18, True)
    queue = []
    for k in range(30):
        queue.append(_pod("svc-%d" % k, {"app": "a"}, ns="ns1") if k % 3 else _pod("lone-%d" % k, {"role": "none"}, ns="ns3"))
    return Input(inp.nodes, [], queue, inp.objs)


# ---- 6. the caps
@functools.lru_cache(maxsize=None)
def caps_input(n=abi.SWEEP_GENERAL_MAX_NODES, zones=None, p=40):
    """n equal nodes spread over `zones` zones (default: the cap), one service, p pods."""
    zones = abi.SWEEP_SPREAD_MAX_ZONES if zones is None else zones
    nodes = [_node("k-%05d" % i, "z%04d" % (i % zones)) for i in range(n)]
    running = [dict(_pod("run-%d" % k, {"app": "a"}), spec=dict(_pod("x", {})["spec"], nodeName="k-%05d" % ((k * 911) % n)))
               for k in range(12)]
    queue = [_pod("q-%d" % k, {"app": "a"}) for k in range(p)]
    objs = dict(services=[{"metadata": {"namespace": "default", "name": "svc"}, "spec": {"selector": {"app": "a"}}}],
                rcs=[], rss=[], sss=[])
    return Input(nodes, running, queue, objs)
