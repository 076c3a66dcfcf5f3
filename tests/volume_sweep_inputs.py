"""Inputs and CPU oracles of the scenario sweep over volume queues (ksim_sweep_volumes), shared by
tests/test_sweep_volume_host.py (their properties) and tests/test_gpu_sweep_volumes.py (the GPU cases),
on the pattern of tests/affinity_sweep_inputs.py.

Every oracle works on objects: the nodes without the absent ones, the running pods without those
bound to them, ingested anew — ksim_ref.simulate with ksim_ref.volume_predicates over the input's
listers for the small inputs (`oracle_ref`), cpu_ref.run on the reduced cluster's own plan for the
large ones and for histograms (`oracle_cpu`) — and node names mapped back to the ranks of the loaded
table.  A queue is a list of pods in scheduling order; the simulator pops its list from the end, so it
is fed the reverse."""
import copy
import functools
import random

import numpy as np

import cpu_ref
import ksim_ref as R
import spread_sweep_inputs as X
from ksim import abi, ingest, scheduler, spread
from workloads import ZONE, rnd_affinity_workload, rnd_spread_workload, rnd_volume, rnd_volume_workload, volume_listers

VOLUME_KEYS = ["NoDiskConflict", "MaxEBSVolumeCount", "MaxGCEPDVolumeCount", "MaxAzureDiskVolumeCount"]
# the policies of tests/test_gpu_volumes.py, and the default provider minus CheckVolumeBinding (it errs on
# every PVC the simulator's empty listers hold) for the zone-labelled inputs
POLICIES = {
    "volumes_lr_bra": (["GeneralPredicates", "PodToleratesNodeTaints"] + VOLUME_KEYS,
                       [("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)]),
    "volumes_only": (VOLUME_KEYS, [("MostRequestedPriority", 2)]),
    "default_zone": ([k for k in scheduler.DEFAULT_PREDICATES if k != "CheckVolumeBinding"],
                     list(scheduler.DEFAULT_PRIORITIES)),
}
VOLUME_REASONS = (abi.R_DISK_CONFLICT, abi.R_MAX_VOLUME_COUNT, abi.R_VOLUME_ZONE)
MSG = {abi.R_DISK_CONFLICT: "node(s) had no available disk", abi.R_MAX_VOLUME_COUNT: "node(s) exceed max volume count",
       abi.R_VOLUME_ZONE: "node(s) had no available volume zone"}


class Input:
    """nodes, running pods, queue (scheduling order), PV / PVC listers, the MaxPD limit, a policy (a name
    of POLICIES or a pair of key lists) and spread lister objects or None; cluster() ingests them."""

    def __init__(self, nodes, running, queue, pvs=(), pvcs=(), max_vols=None, policy="volumes_lr_bra", objs=None):
        self.nodes, self.running, self.queue = list(nodes), list(running), list(queue)
        self.pvs, self.pvcs, self.max_vols, self.policy, self.objs = list(pvs), list(pvcs), max_vols, policy, objs
        self._cl = {}

    def listers(self):
        return spread.SpreadListers(**self.objs) if self.objs else None

    def ingest(self, nodes, running, queue, vol_slots=None):
        mv = None if self.max_vols is None else (self.max_vols,) * 3
        return ingest.Cluster.from_objects(nodes, running, queue, pvs=self.pvs, pvcs=self.pvcs, max_vols=mv,
                                           vol_slots=vol_slots, spread=self.listers())

    def cluster(self, extra=()):
        """The loaded cluster; extra: pods appended to the queue (the drain copies)."""
        key = len(extra)
        if key not in self._cl:
            self._cl[key] = self.ingest(self.nodes, self.running, self.queue + list(extra))
        return self._cl[key]

    def keys(self):
        """(predicates, priorities): the named policy, or the pair given in its place."""
        return POLICIES[self.policy] if isinstance(self.policy, str) else self.policy

    def without_volume_predicates(self):
        preds, prios = self.keys()
        policy = ([k for k in preds if k not in VOLUME_KEYS + ["NoVolumeZoneConflict"]], prios)
        return Input(self.nodes, self.running, self.queue, self.pvs, self.pvcs, self.max_vols, policy, self.objs)


def scheduler_of(inp, cl=None, **kw):
    preds, prios = inp.keys()
    return scheduler.GenericScheduler(cl or inp.cluster(), preds, prios, collect_reasons=False, **kw)


def sets_of(cl, zone=ZONE, seed=3):
    """(label, absent node ranks): none, the first and last node, each value of the zone label, a random
    tenth of the nodes, every node."""
    n = cl.n_nodes
    out = [("none", []), ("first", [0]), ("last", [n - 1])]
    out += [("zone-" + v, list(idx)) for v, idx in scheduler.outage_sets(cl, zone)]
    out.append(("tenth", sorted(random.Random(seed).sample(range(n), max(1, n // 10)))))
    return out + [("all", list(range(n)))]


def _nothing(m):
    return dict(out=np.full(m, -1, np.int32), counter=0, listed=0, count=m, pod=np.arange(m, dtype=np.int32),
                hist=np.zeros((m, abi.NREASONS), np.int32))


def oracle_ref(inp, absent, queue=None, bound=(), counter=0):
    """ksim_ref.simulate of `queue` (default: the input's) on the reduced snapshot: dict(out — ranks
    of the loaded table, -1 failed —, counter, listed, names, msgs [(pod name, FitError text)])."""
    from ksim.report import ERR_NO_NODES
    cl = inp.cluster()
    queue = inp.queue if queue is None else queue
    preds, prios = inp.keys()
    left, stay = X._reduced(inp, cl, absent, bound)
    names = [x["metadata"]["name"] for x in queue]
    if not left:
        return dict(_nothing(len(queue)), counter=counter, names=names, msgs=[(nm, ERR_NO_NODES) for nm in names])
    custom = {k: v for k, v in R.volume_predicates(R.VolumeListers(inp.pvs, inp.pvcs), inp.max_vols).items() if k in preds}
    lst = R.SpreadListers(**inp.objs) if inp.objs else None
    want, lni = R.simulate(left, stay, list(reversed(queue)), set(preds), list(prios), custom_predicates=custom, spread=lst,
                           last_node_index=counter)
    assert [nm for nm, _, _ in want] == names
    out = np.array([cl.index[h] if h is not None else -1 for _, h, _ in want], np.int32)
    return dict(out=out, counter=lni, listed=len(left), names=names, msgs=[(nm, m) for nm, h, m in want if h is None])


def oracle_cpu(inp, absent, queue=None):
    """cpu_ref.run on the plan of the reduced objects: dict(out, counter, listed, count, pod, hist)."""
    cl = inp.cluster()
    queue = inp.queue if queue is None else queue
    preds, prios = inp.keys()
    left, stay = X._reduced(inp, cl, absent)
    m = len(queue)
    if not left:
        return _nothing(m)
    sub = inp.ingest(left, stay, queue)
    pl = scheduler.plan(sub, preds, prios)
    ref, reasons, _, ctr, _ = cpu_ref.run(sub, None, 0, m, threads=8, plan=pl)
    back = np.array([cl.index[nm] for nm in sub.names], np.int32)
    failed = np.nonzero(ref < 0)[0].astype(np.int32)
    return dict(out=np.where(ref >= 0, back[np.maximum(ref, 0)], -1).astype(np.int32), counter=ctr, listed=len(left),
                count=len(failed), pod=failed, hist=np.ascontiguousarray(reasons[failed]))


# ---- 1. the hand cases: two to four nodes, each with the outage of nothing beside its outages
def _node(name, cpu="8", zone=None):
    labels = {"kubernetes.io/hostname": name}
    if zone:
        labels[ZONE] = zone
    return {"metadata": {"name": name, "labels": labels}, "spec": {},
            "status": {"allocatable": {"cpu": cpu, "memory": "32Gi", "pods": "110"},
                       "conditions": [{"type": "Ready", "status": "True"}]}}


def _pod(name, vols=(), cpu="1", node=None):
    pod = {"metadata": {"name": name, "namespace": "ns"},
           "spec": {"containers": [{"resources": {"requests": {"cpu": cpu, "memory": "256Mi"}}}]}}
    if vols:
        pod["spec"]["volumes"] = [dict(v) for v in vols]
    if node:
        pod["spec"]["nodeName"] = node
    return pod


def gce(name, ro=False):
    return {"gcePersistentDisk": {"pdName": name, "readOnly": ro}}


def ebs(name):
    return {"awsElasticBlockStore": {"volumeID": name}}


def pvc(name):
    return {"persistentVolumeClaim": {"claimName": name}}


def _hand(case):
    if case == "shared-rw-pd":
        # LeastRequested sends q1 to the larger n1; its mount, made by the sweep, sends q2 to n2
        return Input([_node("n1", "8"), _node("n2", "4")], [], [_pod("q1", [gce("g-x")]), _pod("q2", [gce("g-x")])]), \
            [["n2"], ["n1"]]
    if case == "running-disk-blocks-best":
        # r's EBS disk keeps q off n1, the emptiest node; p0 (no volumes) goes there.  Without n1, p0 fills
        # n2 and q moves to n3; without n2, q moves to n3 as well
        nodes = [_node("n1", "8"), _node("n2", "4"), _node("n3", "2")]
        return Input(nodes, [_pod("r", [ebs("e-x")], cpu="100m", node="n1")],
                     [_pod("p0", cpu="3"), _pod("q", [ebs("e-x")], cpu="2")]), [["n1"], ["n2"], ["n3"]]
    if case == "max-volume-count":
        # MostRequested packs n1 (r runs there, mounting g-a read-only).  q1's g-a is mounted already and
        # adds nothing, q2's claim resolves to g-pv (two distinct ids on n1), q3's g-b would be the third
        pvs = [{"metadata": {"name": "pv-g"}, "spec": {"gcePersistentDisk": {"pdName": "g-pv"}}}]
        pvcs = [{"metadata": {"name": "c1", "namespace": "ns"}, "spec": {"volumeName": "pv-g"}}]
        return Input([_node("n1"), _node("n2")], [_pod("r", [gce("g-a", True)], cpu="2", node="n1")],
                     [_pod("q1", [gce("g-a", True)]), _pod("q2", [pvc("c1")]), _pod("q3", [gce("g-b", True)])],
                     pvs, pvcs, 2, "volumes_only"), [["n2"], ["n1"]]
    if case == "pv-zone":
        pvs = [{"metadata": {"name": "pv-a", "labels": {ZONE: "a"}}, "spec": {"nfs": {"server": "s"}}}]
        pvcs = [{"metadata": {"name": "c1", "namespace": "ns"}, "spec": {"volumeName": "pv-a"}}]
        nodes = [_node("a1", zone="a"), _node("a2", zone="a"), _node("b1", zone="b"), _node("b2", zone="b")]
        return Input(nodes, [], [_pod("q", [pvc("c1")]), _pod("plain")], pvs, pvcs, None, "default_zone"), \
            [["a1", "a2"], ["b1", "b2"]]
    raise KeyError(case)


HAND = ["shared-rw-pd", "running-disk-blocks-best", "max-volume-count", "pv-zone"]
# the reference's answers, per case: the outage of nothing first, then the case's outages in order;
# (pod, node or the reason every listed node gives)
HAND_WANT = {
    "shared-rw-pd": [[("q1", "n1"), ("q2", "n2")], [("q1", "n1"), ("q2", abi.R_DISK_CONFLICT)],
                     [("q1", "n2"), ("q2", abi.R_DISK_CONFLICT)]],
    "running-disk-blocks-best": [[("p0", "n1"), ("q", "n2")], [("p0", "n2"), ("q", "n3")], [("p0", "n1"), ("q", "n3")],
                                 [("p0", "n1"), ("q", "n2")]],
    "max-volume-count": [[("q1", "n1"), ("q2", "n1"), ("q3", "n2")], [("q1", "n1"), ("q2", "n1"), ("q3", abi.R_MAX_VOLUME_COUNT)],
                         [("q1", "n2"), ("q2", "n2"), ("q3", abi.R_MAX_VOLUME_COUNT)]],
    "pv-zone": [[("q", "a2"), ("plain", "b1")], [("q", abi.R_VOLUME_ZONE), ("plain", "b2")], [("q", "a2"), ("plain", "a1")]],
}


@functools.lru_cache(maxsize=None)
def hand_input(case):
    return _hand(case)[0]


def hand_sets(case):
    inp, outages = _hand(case)
    cl = hand_input(case).cluster()
    return [("none", [])] + [("-".join(o), [cl.index[nm] for nm in o]) for o in outages]


def hand_message(listed, reason):
    return "0/%d nodes are available: %d %s." % (listed, listed, MSG[reason])


# ---- 1b. drain: the evicted pods carry their disks
@functools.lru_cache(maxsize=None)
def drain_input(case):
    if case == "rehost-keeps-off":
        # r (read-write g-x) is evicted from n1 and re-hosts on the emptier of n2 / n3; q, with the same
        # disk, is then kept off that survivor
        nodes = [_node("n1", "8"), _node("n2", "8"), _node("n3", "4")]
        return Input(nodes, [_pod("r", [gce("g-x")], node="n1")], [_pod("q", [gce("g-x")])])
    if case == "stranded-by-maxpd":
        # one EBS volume per node allowed and every node has one: no survivor takes the evicted pod
        nodes = [_node("n1"), _node("n2"), _node("n3")]
        running = [_pod("r%d" % k, [ebs("e-%d" % k)], node="n%d" % k) for k in (1, 2, 3)]
        return Input(nodes, running, [_pod("plain")], max_vols=1)
    raise KeyError(case)


DRAIN = ["rehost-keeps-off", "stranded-by-maxpd"]


def drain_plan(inp, sets_):
    """(copies appended to the queue, per set the loaded-queue indices of its copies, per set the
    scenario's own prefix as objects): running pods in their order, those on a node of some set."""
    cl = inp.cluster()
    lost = set().union(*[set(a) for _, a in sets_]) if sets_ else set()
    evicted = [(cl.index[x["spec"]["nodeName"]], x) for x in inp.running
               if cl.index[x["spec"]["nodeName"]] in lost and scheduler.default_evictable(x)]
    copies = [scheduler.requeue_copy(x) for _, x in evicted]
    nq = len(inp.queue)
    requeue = [[nq + k for k, (w, _) in enumerate(evicted) if w in set(a)] for _, a in sets_]
    return copies, requeue, [[copies[q - nq] for q in rq] for rq in requeue]


# ---- 2. the random workloads: nodes -> (queued pods, running pods, seed, max_vols, policy).  The queues
# are long enough for the volume predicates to fail pods on every listed node; seed 0 is the first seed
# at every size for which the conditions of tests/test_sweep_volume_host.py hold
RND = {16: (120, 14, 0, 4, "volumes_lr_bra"), 70: (700, 50, 0, 3, "volumes_only"), 130: (1300, 90, 0, 2, "volumes_lr_bra")}
RND_ZONE = {n: t[:4] for n, t in RND.items()}  # zone-labelled, resolvable claims only, under "default_zone"


@functools.lru_cache(maxsize=None)
def rnd_input(n_nodes, zones=False, seed=None):
    if zones:
        n_pods, n_running, s, mv = RND_ZONE[n_nodes]
        policy = "default_zone"
    else:
        n_pods, n_running, s, mv, policy = RND[n_nodes]
    s = s if seed is None else seed
    nodes, running, pods, pvs, pvcs = rnd_volume_workload(s, n_nodes=n_nodes, n_pods=n_pods, n_running=n_running,
                                                          zones=zones, resolvable_only=zones)
    return Input(nodes, running, pods, pvs, pvcs, mv, policy)


@functools.lru_cache(maxsize=None)
def rnd_refs(n_nodes, zones=False, seed=None):
    """(input, sets, cpu_ref answers with histograms) of one random workload, once."""
    inp = rnd_input(n_nodes, zones, seed)
    sets_ = sets_of(inp.cluster())
    return inp, sets_, [oracle_cpu(inp, a) for _, a in sets_]


def reasons_seen(refs):
    """Which of the three volume reasons occur among the failed pods of the answers."""
    return {bit for bit in VOLUME_REASONS if sum(int((r["hist"][:, bit] > 0).sum()) for r in refs) > 0}


# ---- 3. geometry: one node, the wave and block edges, two rows per thread
@functools.lru_cache(maxsize=None)
def geometry_input(n, p=24):
    """n equal nodes, a fifth of them with a running pod that mounts a read-write disk of the queue's;
    the queue mixes pods that share four GCE disks read-write (so they spread over distinct nodes and
    fail once every listed node holds the disk) with EBS pods under MaxEBSVolumeCount = 2."""
    rng = random.Random(n)
    nodes = [_node("g-%05d" % i, "16") for i in range(n)]
    running = [_pod("run-%d" % i, [gce("d%d" % (i % 4))], cpu="100m", node="g-%05d" % i) for i in range(0, n, 5)]
    queue = []
    for k in range(p):
        t = rng.random()
        vols = [gce("d%d" % rng.randrange(4))] if t < 0.5 else [ebs("e%d" % rng.randrange(6)) for _ in range(rng.randint(1, 2))]
        queue.append(_pod("q-%d" % k, vols if t < 0.9 else (), cpu="500m"))
    return Input(nodes, running, queue, max_vols=2)


def geometry_sets(n):
    out = [("none", [])]
    if n > 1:
        out += [("first", [0]), ("last", [n - 1]), ("odd", list(range(1, n, 2)))]
    else:
        out += [("all", [0])]
    return out


# ---- 3b. a node with more mounted keys than the register form holds
@functools.lru_cache(maxsize=None)
def many_mounts_input(keys=17):
    """busy (16 cpu, the emptiest node, so LeastRequested prefers it) runs one pod with `keys` distinct
    read-only GCE disks; small is the alternative.  q1 adds an 18th key to busy, q2 mounts one of the
    first 17 read-write and conflicts there, q3 reads one of them again (nothing new)."""
    nodes = [_node("busy", "64"), _node("small", "2")]
    running = [_pod("r", [gce("k%02d" % k, True) for k in range(keys)], cpu="100m", node="busy")]
    queue = [_pod("q1", [gce("new", True)]), _pod("q2", [gce("k16")]), _pod("q3", [gce("k16", True)]),
             _pod("q4", [gce("new")])]
    return Input(nodes, running, queue, max_vols=40)  # (the default limit of 16 GCE disks would close busy)


# ---- 3c. the node cap
@functools.lru_cache(maxsize=None)
def caps_input(n=abi.SWEEP_GENERAL_MAX_NODES, p=6):
    """n equal nodes.  The eight at the top of the name order, where selectHost starts, each run a small
    pod that mounts d0 or d1 read-write; they score as the empty nodes do for the queue's pods, which
    mount the same two disks: NoDiskConflict alone moves them."""
    nodes = [_node("k-%05d" % i, "8") for i in range(n)]
    running = [_pod("run-%d" % k, [gce("d%d" % (k % 2))], cpu="100m", node="k-%05d" % (n - 1 - k)) for k in range(8)]
    queue = [_pod("q-%d" % k, [gce("d%d" % (k % 2))]) for k in range(p)]
    return Input(nodes, running, queue)


# ---- 4. combinations
def _listers_for(*pod_lists):
    """volume_listers(resolvable_only=True) with its claims repeated in every namespace of the pods."""
    pvs, pvcs, _ = volume_listers(resolvable_only=True)
    spaces = sorted({(x["metadata"].get("namespace") or "default") for pods in pod_lists for x in pods})
    return pvs, [dict(c, metadata=dict(c["metadata"], namespace=ns)) for ns in spaces for c in pvcs]


def _with_volumes(pods, seed, p_vol=0.5):
    """The pods, about p_vol of them with one or two random volumes (claims of volume_listers)."""
    rng = random.Random(seed)
    _, _, claims = volume_listers(resolvable_only=True)
    pods = copy.deepcopy(list(pods))
    for x in pods:
        if rng.random() < p_vol:
            x["spec"]["volumes"] = [rnd_volume(rng, claims) for _ in range(rng.randint(1, 2))]
    return pods


@functools.lru_cache(maxsize=None)
def spread_input(n_nodes=70, n_pods=90):
    """workloads.rnd_spread_workload with its listers (SelectorSpread state alone: the SPR + VOL kernels),
    half of the pods with volumes."""
    nodes, running, pods, objs = rnd_spread_workload(1, n_nodes=n_nodes, n_pods=n_pods, n_running=n_nodes, zones=True)
    pvs, pvcs = _listers_for(running, pods)
    return Input(nodes, _with_volumes(running, 11), _with_volumes(pods, 12), pvs, pvcs, 3, "default_zone", objs)


@functools.lru_cache(maxsize=None)
def affinity_input(n_nodes=70, n_pods=90, n_running=70):
    """A C2x-shaped queue: workloads.rnd_affinity_workload (required and preferred terms, carried terms of
    the running pods: the IPA + VOL kernels), half of the pods with volumes."""
    nodes, running, pods = rnd_affinity_workload(1, n_nodes, n_pods, n_running)
    pvs, pvcs = _listers_for(running, pods)
    return Input(nodes, _with_volumes(running, 21), _with_volumes(pods, 22), pvs, pvcs, 3, "default_zone")


AFF_ZONE = "zone"  # the topology label of workloads.rnd_affinity_nodes


@functools.lru_cache(maxsize=None)
def classes_input(n=300, p=80):
    """synth.c2_objects (taints and tolerations: several TaintToleration classes), a third of the pods with
    volumes."""
    from ksim import synth
    nodes, pods = synth.c2_objects(n, p, seed=7)
    pvs, pvcs = _listers_for(pods)
    return Input(nodes, [], _with_volumes(pods, 31, 0.4), pvs, pvcs, 2, "default_zone")
