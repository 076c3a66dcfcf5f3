"""Inputs, scenario lists and CPU oracles of the policy sweep (ksim_sweep_policy), shared by
tests/test_sweep_policy_host.py (their properties, on the CPU) and tests/test_gpu_sweep_policy.py (the
GPU cases), on the pattern of tests/volume_sweep_inputs.py and tests/spread_sweep_inputs.py.

A scenario is a prioritizer list.  Its oracle is one run of the reference on the reduced objects — the
nodes without the scenario's absent ones, the running pods without those bound to them — under the
input's predicates and that list: cpu_ref.run on the reduced cluster's own plan (`oracle`, with
histograms), ksim_ref.simulate for the message texts of the smallest input (`oracle_messages`).  Outcome
records are recounted from the oracle's placements with Python integers (`outcome_of`)."""
import copy
import functools
import random

import numpy as np

import affinity_sweep_inputs as A
import spread_sweep_inputs as X
import volume_sweep_inputs as V
from ksim import abi, scheduler, synth
from workloads import rnd_nodes, rnd_pod, rnd_spread_workload

DEFAULT_PREDICATES, DEFAULT_PRIORITIES = scheduler.provider("DefaultProvider")
RESTRICTED = ("TaintTolerationPriority", "NodeAffinityPriority", "SelectorSpreadPriority", "InterPodAffinityPriority")
MAP = ("LeastRequestedPriority", "MostRequestedPriority", "BalancedResourceAllocation")


def vary(base, **weights):
    """The prioritizer list `base` with the named weights replaced (0: the priority dropped; a name the
    list lacks is appended).  Keywords: the priority names without their "Priority" suffix."""
    full = {n[:-len("Priority")] if n.endswith("Priority") else n: n for n in RESTRICTED + MAP}
    out = [(n, w) for n, w in base]
    for short, w in weights.items():
        name = full[short]
        out = [(n, x) for n, x in out if n != name]
        if w:
            out.append((name, w))
    return out


def scenarios_of(base=DEFAULT_PRIORITIES):
    """Eleven scenarios around the default provider: the provider itself, each of the four restricted
    priorities dropped and rescaled, Balanced dropped, and packing (MostRequested for LeastRequested)."""
    b = list(base)
    return [b,
            vary(b, TaintToleration=0), vary(b, TaintToleration=3),
            vary(b, NodeAffinity=0), vary(b, NodeAffinity=4),
            vary(b, SelectorSpread=0), vary(b, SelectorSpread=3),
            vary(b, InterPodAffinity=0), vary(b, InterPodAffinity=2),
            vary(b, BalancedResourceAllocation=0),
            vary(b, LeastRequested=0, MostRequested=2)]


# (scenario, scenario) pairs of scenarios_of that differ in one restricted weight alone, per priority;
# the first of each has the weight at 0 on one side and is the one whose placements must differ (a
# rescaled weight moves fewer pods, and on the larger clusters often none)
PAIRS = {"TaintTolerationPriority": [(0, 1), (0, 2)], "NodeAffinityPriority": [(0, 3), (0, 4)],
         "SelectorSpreadPriority": [(0, 5), (0, 6)], "InterPodAffinityPriority": [(0, 7), (0, 8)]}
MAP_PAIR = (0, 9)  # differs in BalancedResourceAllocation alone


def weights_of(pri):
    """name -> weight of a prioritizer list."""
    return {n: int(w) for n, w in pri}


def differ_only_in(a, b):
    """The priority names whose weights differ between two prioritizer lists."""
    wa, wb = weights_of(a), weights_of(b)
    return {n for n in set(wa) | set(wb) if wa.get(n, 0) != wb.get(n, 0)}


def with_priorities(inp, pri):
    """The input under its own predicates and the prioritizer list `pri` (sharing its ingested clusters)."""
    preds, _ = inp.keys()
    new = V.Input(inp.nodes, inp.running, inp.queue, inp.pvs, inp.pvcs, inp.max_vols, (list(preds), list(pri)), inp.objs)
    new._cl = inp._cl
    return new


def oracle(inp, pri, absent=(), queue=None):
    """cpu_ref.run of the scenario: dict(out, counter, listed, count, pod, hist) in ranks of the loaded table."""
    return V.oracle_cpu(with_priorities(inp, pri), list(absent), queue)


def oracle_messages(inp, pri, absent=(), queue=None):
    """ksim_ref.simulate of the scenario: dict(out, counter, listed, names, msgs)."""
    return V.oracle_ref(with_priorities(inp, pri), list(absent), queue)


def least(req, cap):
    """LeastRequestedPriority's per-resource score (least_requested.go:36-53), Python integers."""
    req, cap = int(req), int(cap)
    if cap == 0 or req > cap:
        return 0
    return ((cap - req) * 10) // cap


def outcome_of(cl, absent, placed):
    """The outcome record of a scenario, recounted on the host: cl the loaded cluster, absent its node
    ranks left out, placed [(loaded queue index, node rank)] of every pod the oracle bound (prefix pods
    included).  dict(listed, used, free_cpu [11], free_mem [11]) of Python integers."""
    n = cl.n_nodes
    gone = set(int(i) for i in absent)
    nzc = [int(v) for v in cl.cols["nz_cpu"]]
    nzm = [int(v) for v in cl.cols["nz_mem"]]
    cnt = [int(v) for v in cl.cols["pod_count"]]
    for q, w in placed:
        w = int(w)
        assert w not in gone
        nzc[w] += int(cl.pods["nz_cpu"][q])
        nzm[w] += int(cl.pods["nz_mem"][q])
        cnt[w] += 1
    rec = dict(listed=0, used=0, free_cpu=[0] * abi.OUTCOME_BUCKETS, free_mem=[0] * abi.OUTCOME_BUCKETS)
    for i in range(n):
        if i in gone:
            continue
        rec["listed"] += 1
        rec["used"] += 1 if cnt[i] > 0 else 0
        rec["free_cpu"][least(nzc[i], cl.cols["alloc_cpu"][i])] += 1
        rec["free_mem"][least(nzm[i], cl.cols["alloc_mem"][i])] += 1
    return rec


def outcome_of_answer(cl, absent, out, first=0, prefix=(), prefix_out=()):
    """outcome_of from an oracle's answer over pods [first, first + len(out)) after the prefix pods."""
    placed = [(q, w) for q, w in zip(prefix, prefix_out) if w >= 0]
    placed += [(first + k, w) for k, w in enumerate(out) if w >= 0]
    return outcome_of(cl, absent, placed)


# ---- 1. the full workload: every priority of the default provider has something to read
HOSTNAME = "kubernetes.io/hostname"
# (nodes, queued pods) -> seed: the first seed for which the conditions of tests/test_sweep_policy_host.py
# hold for the reference alone (chosen there, on the CPU)
RND_SIZES = list(X.RND_SIZES) + [(1030, 80)]
SEEDS = {18: 0, 70: 0, 130: 0, 1030: 0}


def full_workload(seed, n_nodes, n_pods):
    """workloads.rnd_nodes / rnd_pod with their features (taints with PreferNoSchedule ones, preferred
    node affinity, selectors, host ports, extended resources), the nodes in three zones with hostname
    labels, the pods labelled and in the namespaces of workloads.rnd_spread_workload with its services and
    controllers, and a third of them with an inter-pod term over their own labels, per zone or hostname,
    required or preferred, affinity or anti-affinity.  One running pod per node on average: 1-cpu nodes
    under several of them are over-committed.  One queued pod asks for more cpu than any node has."""
    rng = random.Random(4000 + seed)
    nodes = rnd_nodes(rng, n_nodes, features=True)
    for x in nodes:
        x["status"]["allocatable"]["pods"] = "110"
        x["metadata"]["labels"][HOSTNAME] = x["metadata"]["name"]
        if rng.random() < 0.8:
            x["metadata"]["labels"][X.ZONE] = rng.choice(["z1", "z2", "z3"])
    _, _, _, objs = rnd_spread_workload(seed, n_nodes=1, n_pods=0, n_running=0)

    def pod(name, nn=None):
        p = rnd_pod(rng, name, features=True)
        p["metadata"]["namespace"] = rng.choice(["ns1", "ns1", "ns2"])
        lab = {}
        if rng.random() < 0.9:
            lab["app"] = rng.choice("abc")
        if rng.random() < 0.5:
            lab["tier"] = rng.choice("xy")
        p["metadata"]["labels"] = lab
        if lab and rng.random() < 0.34:
            t = {"labelSelector": {"matchLabels": dict(lab)}, "topologyKey": rng.choice([X.ZONE, HOSTNAME])}
            sec = rng.choice(["podAffinity", "podAntiAffinity", "podAntiAffinity"])
            if rng.random() < 0.3 and sec == "podAntiAffinity":
                body = {"requiredDuringSchedulingIgnoredDuringExecution": [t]}
            else:
                body = {"preferredDuringSchedulingIgnoredDuringExecution": [{"weight": rng.randint(1, 100),
                                                                             "podAffinityTerm": t}]}
            p["spec"].setdefault("affinity", {})[sec] = body
        if nn:
            p["spec"]["nodeName"] = nn
        return p
    running = [pod("run-%d" % k, rng.choice(nodes)["metadata"]["name"]) for k in range(n_nodes)]
    pods = [pod("pod-%d" % k) for k in range(n_pods)]
    # one pod no node can hold, in the middle of the queue: every scenario fails it on every listed node
    pods[n_pods // 2] = {"metadata": {"name": "pod-huge", "namespace": "ns1", "labels": {"app": "a"}},
                         "spec": {"containers": [{"resources": {"requests": {"cpu": "64", "memory": "1Gi"}}}]}}
    return nodes, running, pods, objs


@functools.lru_cache(maxsize=None)
def full_input(n_nodes, seed=None):
    n_pods = dict(RND_SIZES)[n_nodes]
    nodes, running, pods, objs = full_workload(SEEDS[n_nodes] if seed is None else seed, n_nodes, n_pods)
    return V.Input(nodes, running, pods, policy=(list(DEFAULT_PREDICATES), list(DEFAULT_PRIORITIES)), objs=objs)


@functools.lru_cache(maxsize=None)
def full_refs(n_nodes, seed=None):
    """(input, scenarios, oracle answers) of the full workload at one size, once."""
    inp = full_input(n_nodes, seed)
    scen = scenarios_of()
    return inp, scen, [oracle(inp, pri) for pri in scen]


def conditions(inp, scen, refs):
    """What tests/test_sweep_policy_host.py asks of an input, as a dict of booleans and counts."""
    cl = inp.cluster()
    pair = {}
    for name, pairs in PAIRS.items():
        pair[name] = [bool((refs[a]["out"] != refs[b]["out"]).any()) for a, b in pairs]
    a, b = MAP_PAIR
    recs = [outcome_of_answer(cl, (), r["out"]) for r in refs]
    buckets = {k for rec in recs for k, v in enumerate(rec["free_cpu"]) if v} | \
              {k for rec in recs for k, v in enumerate(rec["free_mem"]) if v}
    over = any(int(cl.cols["alloc_cpu"][i]) == 0 or int(cl.cols["nz_cpu"][i]) > int(cl.cols["alloc_cpu"][i]) or
               int(cl.cols["alloc_mem"][i]) == 0 or int(cl.cols["nz_mem"][i]) > int(cl.cols["alloc_mem"][i])
               for i in range(cl.n_nodes))
    return dict(pair=pair, map_pair=bool((refs[a]["out"] != refs[b]["out"]).any()),
                failures=sum(int(r["count"]) for r in refs), buckets=buckets, bucket0_overcommit=over and 0 in buckets)


def holds(c):
    return all(v[0] for v in c["pair"].values()) and c["map_pair"] and c["failures"] > 0 and \
        len(c["buckets"]) >= 3 and c["bucket0_overcommit"]


# ---- 2. each instantiation
@functools.lru_cache(maxsize=None)
def plain_input(n=300, p=80):
    """synth.c2_objects: taints and tolerations (several TaintToleration classes), and every third pod
    with a preferred node-affinity term over the nodes' labels, so that K > 1 in both dimensions.  No
    listers, no inter-pod terms: the plain instantiations."""
    nodes, pods = synth.c2_objects(n, p, seed=7)
    nodes, pods = copy.deepcopy(nodes), copy.deepcopy(pods)
    rng = random.Random(9)
    for x in nodes:
        x["metadata"].setdefault("labels", {})["disk"] = rng.choice(["ssd", "hdd"])
    for k, x in enumerate(pods):
        if k % 3 == 0:
            x["spec"].setdefault("affinity", {})["nodeAffinity"] = {"preferredDuringSchedulingIgnoredDuringExecution": [
                {"weight": 5, "preference": {"matchExpressions": [{"key": "disk", "operator": "In", "values": ["ssd"]}]}}]}
    return V.Input(nodes, [], pods, policy=(list(DEFAULT_PREDICATES), list(DEFAULT_PRIORITIES)))


@functools.lru_cache(maxsize=None)
def spread_input():
    """spread_sweep_inputs.rnd_input(70): a queue with services and controllers, SelectorSpread state alone."""
    inp = X.rnd_input(70, True)
    return V.Input(inp.nodes, inp.running, inp.queue, policy=(list(DEFAULT_PREDICATES), list(DEFAULT_PRIORITIES)),
                   objs=inp.objs)


@functools.lru_cache(maxsize=None)
def anti_input(n=40, zones=4, p=30):
    """Replicas of one app that repel each other per hostname (required) and prefer other zones, twelve of
    them running: affinity_sweep_inputs.caps_input at a small size.  The residents matter: a zone outage
    takes the running replicas of the zone out of every survivor's zone count."""
    inp = A.caps_input(n, zones, p)
    return V.Input(inp.nodes, inp.running, inp.queue, policy=(list(DEFAULT_PREDICATES), list(DEFAULT_PRIORITIES)))


def volume_input():
    """volume_sweep_inputs.rnd_input(16, zones=True): volumes of every kind under the default provider
    without CheckVolumeBinding."""
    return V.rnd_input(16, True)


def map_scenarios(base):
    """Scenarios for a policy without restricted priorities to rescale: the map weights alone."""
    b = list(base)
    return [b, vary(b, LeastRequested=3), vary(b, BalancedResourceAllocation=0), vary(b, LeastRequested=0, MostRequested=2)]
