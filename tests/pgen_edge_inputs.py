"""Designed inputs for the general persistent kernels' edge tests (tests/test_gpu_pgen_edges.py; pinned on
the CPU by tests/test_pgen_edges_host.py).  No device is needed to build them.

A Case is the ingested cluster, the policy and the environment its GPU test sets (the diagnostic caps
that select a plan); reference() is the table-level C oracle (oracle/cpu_ref.c) over the scheduler's
plan, whole or in pieces with carried state, computed once per case and shared.

Who publishes first.  The tag-cycle cases must not depend on winning a race, so the rows of every
workgroup but the first carry ordinary predicate work the first workgroup's rows lack (late_rows: running
pods with host ports there, and every queued pod brings host ports of its own, so PodFitsHostPorts walks
port pairs on the late rows and nothing on the first LATE_FROM).  The first workgroup then publishes and
sweeps first by data alone; nothing is held and no spin bound changes."""
import functools

import numpy as np

import cpu_ref
from ksim import ingest, scheduler, spread as kspread, synth
from workloads import sixteen_class_workload, uniform_selector_workload

ZONE = "failure-domain.beta.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"
GPU = "alpha.kubernetes.io/nvidia-gpu"
EPH = "ephemeral-storage"
EXT = "example.com/widget"


class Case:
    def __init__(self, cl, preds=None, prios=None, env=None, custom=None, **marks):
        d = scheduler.provider("DefaultProvider")
        self.cl, self.preds, self.prios = cl, list(d[0] if preds is None else preds), list(d[1] if prios is None else prios)
        self.env = dict(env or {})
        self.custom = custom  # a Policy's priorities with an argument, by name (GenericScheduler's custom_priorities)
        self.marks = marks  # what the host test asserts about the input (queue indices, node names)
        self._ref = {}

    @property
    def n(self):
        return self.cl.n_nodes

    @property
    def m(self):
        return len(self.cl.pods)

    @functools.cached_property
    def plan(self):
        return scheduler.plan(self.cl, self.preds, self.prios, custom_priorities=self.custom)

    def reference(self, pieces=None):
        """dict(out, reasons, state, ctr, extra) of the C oracle over the whole queue; pieces (counts, the
        last one None = the rest): one oracle call per piece on the carried state."""
        key = tuple(pieces) if pieces else None
        if key not in self._ref:
            counts = list(pieces or [None])
            outs, reas, state, ctr, extra, first = [], [], None, 0, None, 0
            for cnt in counts:
                cnt = self.m - first if cnt is None else cnt
                r = cpu_ref.run(self.cl, None, first=first, count=cnt, threads=4, state=state, counter=ctr, plan=self.plan,
                                extra=extra)
                out, re_, state, ctr, extra = r
                outs.append(out)
                reas.append(re_)
                first += cnt
            assert first == self.m
            self._ref[key] = dict(out=np.concatenate(outs), reasons=np.concatenate(reas), state=state, ctr=ctr, extra=extra)
        return self._ref[key]


def pod_classes(case):
    """n_tt x n_na of every queue pod (the reduce classes K of its decision)."""
    t = case.plan.tables
    return (np.asarray(t["n_tt"]) * np.asarray(t["n_na"]))[np.asarray(case.cl.pods["cls"])]


# ---------------------------------------------------------------------------------- plan geometry
@functools.lru_cache(maxsize=None)
def geometry(n, per_node=2, slack=24, seed=6, light=False):
    """synth.c2x_objects on n nodes (SelectorSpread over 20 services, hostname anti-affinity, volumes, host
    ports, selectors, taints), every node with room for `per_node` pods and a queue of per_node * n + slack:
    it saturates, so the last rows of the last workgroup are chosen and the tail is FitErrors.
    light: the same objects with three services instead of 20 (four counted pairs instead of 40, one carried
    anti-affinity term), no host
    ports and three volume slots a node, so that a workgroup's LDS holds 768 dual-form rows or 1,024
    single-form ones (the full shape fits about 340)."""
    m = per_node * n + slack
    nodes, pods, pvs, pvcs, services = synth.c2x_objects(n, m, seed)
    for x in nodes:
        x["status"]["allocatable"]["pods"] = str(per_node)
        if n <= 4:  # (the smallest tables: every node takes pods)
            x["spec"].pop("taints", None)
            x["spec"].pop("unschedulable", None)
            x["status"]["conditions"][0]["status"] = "True"
    if light:
        services = services[:3]
        for k, p in enumerate(pods):
            app = "a%d" % (k % 3)
            p["metadata"]["labels"] = {"app": app}
            p["spec"]["containers"][0].pop("ports", None)
            if "affinity" in p["spec"]:  # (one carried term: the anti-affinity pods of one app)
                p["spec"]["affinity"] = anti(HOST, app="a0")
                p["metadata"]["labels"] = {"app": "a0"}
    cl = ingest.Cluster.from_objects(nodes, (), pods, pvs=pvs, pvcs=pvcs, spread=kspread.SpreadListers(services=services),
                                     vol_slots=3 if light else None)
    return Case(cl, objs=dict(nodes=nodes, pods=pods, pvs=pvs, pvcs=pvcs, services=services))


# ---------------------------------------------------------------------------------- building blocks
def node(i, zone=None, labels=None, pods=110, cpu="64", mem="256Gi", extra=None, taints=()):
    name = "e-%05d" % i
    lab = {HOST: name}
    if zone is not None:
        lab[ZONE] = zone
    lab.update(labels or {})
    alloc = {"cpu": cpu, "memory": mem, "pods": str(pods)}
    alloc.update(extra or {})
    x = {"metadata": {"name": name, "labels": lab}, "spec": {},
         "status": {"allocatable": alloc, "conditions": [{"type": "Ready", "status": "True"}]}}
    if taints:
        x["spec"]["taints"] = [{"key": k, "value": "true", "effect": "PreferNoSchedule"} for k in taints]
    return x


def pod(name, labels=None, cpu="100m", mem="64Mi", ports=(), requests=None, node_name=None, **spec):
    req = {"cpu": cpu, "memory": mem}
    req.update(requests or {})
    ctr = {"resources": {"requests": req}}
    if ports:
        ctr["ports"] = [{"hostPort": p, "protocol": "TCP"} for p in ports]
    s = {"containers": [ctr]}
    if node_name is not None:
        s["nodeName"] = node_name
    s.update(spec)
    return {"metadata": {"name": name, "namespace": "default", "labels": dict(labels or {})}, "spec": s}


def term(key, **match):
    return {"labelSelector": {"matchLabels": match}, "topologyKey": key}


def anti(key, **match):
    return {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [term(key, **match)]}}


def prefer(key, weight, **match):
    return {"podAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": weight, "podAffinityTerm": term(key, **match)}]}}


def gce(disk, read_only=False):
    return [{"name": "v", "gcePersistentDisk": {"pdName": disk, "readOnly": read_only}}]


LATE_FROM = 192  # rows below: the first workgroup's at KSIM_PGEN_CHUNK=192


def late_rows(n, first=LATE_FROM, per_node=2):
    """Running pods with 4 host ports each on every node from rank `first` up."""
    return [pod("late-%d-%d" % (i, j), ports=range(20000 + 4 * j, 20004 + 4 * j), node_name="e-%05d" % i)
            for i in range(first, n) for j in range(per_node)]


def port_set(k):
    """The host ports queue pod k brings (two, one of 8 sets: a node takes at most 8 such pods)."""
    return range(9000 + 2 * (k % 8), 9002 + 2 * (k % 8))


# ---------------------------------------------------------------------------------- ring and call edges
PIECES = (1, 2, 3, 5, 250, None)


@functools.lru_cache(maxsize=None)
def ring(n=400, m=540, seed=9):
    """A C2x-shaped queue scheduled whole, in PIECES, and in calls of 1..5 pods (the two-record preload,
    the copy of pod p+2, the deferred commit of a call's last pod)."""
    nodes, pods, pvs, pvcs, services = synth.c2x_objects(n, m, seed)
    for x in nodes:
        x["status"]["allocatable"]["pods"] = "3"
    cl = ingest.Cluster.from_objects(nodes, (), pods, pvs=pvs, pvcs=pvcs, spread=kspread.SpreadListers(services=services))
    return Case(cl, objs=dict(nodes=nodes, pods=pods, pvs=pvs, pvcs=pvcs, services=services))


# ---------------------------------------------------------------------------------- commits that leave the LDS image
@functools.lru_cache(maxsize=None)
def nohyp(n=400, m=420, Z=25):
    """Pods whose commit is no hypothesis (PGF_NOHYP: gpu, ephemeral-storage and extended-resource
    requests; zone-keyed required and preferred terms, i.e. shared-domain commits) between node-keyed
    pods (hostname anti-affinity) and plain ones; the first and the last pod of the queue are such pods, and
    runs of consecutive zone-keyed pods land in different workgroups (their zone anti-affinity spreads them
    over zones, zone = rank % Z, and the round-robin walks the table)."""
    extra = {GPU: "2", EPH: "100Gi", EXT: "3"}
    nodes = [node(i, zone="z%d" % (i % Z), pods=8, extra=extra) for i in range(n)]
    pods = []
    kinds = []
    for k in range(m):
        r = k % 12
        name = "h-%d" % k
        if k == 0 or k == m - 1 or r == 3:
            kinds.append("gpu")
            pods.append(pod(name, {"app": "g"}, requests={GPU: "1"}))
        elif r == 5:
            kinds.append("eph")
            pods.append(pod(name, {"app": "e"}, requests={EPH: "30Gi"}))
        elif r == 7:
            kinds.append("ext")
            pods.append(pod(name, {"app": "x"}, requests={EXT: "1"}))
        elif r in (8, 9, 10):  # three consecutive shared-domain commits
            kinds.append("zone")
            grp = "zq%d" % (k // 12 % 3)
            pods.append(pod(name, {"grp": grp}, affinity=dict(anti(ZONE, grp=grp)) if k // 12 % 2 == 0 else
                            dict(prefer(ZONE, 40, app="g"), **anti(ZONE, grp=grp))))
        elif r in (1, 6):
            kinds.append("host")
            pods.append(pod(name, {"app": "n%d" % (k % 3)}, affinity=anti(HOST, app="n%d" % (k % 3))))
        else:
            kinds.append("plain")
            pods.append(pod(name, {"app": "p"}))
    services = [{"metadata": {"name": "svc-p", "namespace": "default"}, "spec": {"selector": {"app": "p"}}}]
    cl = ingest.Cluster.from_objects(nodes, (), pods, spread=kspread.SpreadListers(services=services))
    return Case(cl, kinds=kinds, objs=dict(nodes=nodes, pods=pods, services=services))


# ---------------------------------------------------------------------------------- caps
@functools.lru_cache(maxsize=None)
def zones(Z, n=232, m=300):
    """SelectorSpread over Z zones (the pass-A record holds 28): every pod under one of three services."""
    nodes = [node(i, zone="z%02d" % (i % Z), pods=2) for i in range(n)]
    pods = [pod("s-%d" % k, {"app": "a%d" % (k % 3)}, affinity=anti(HOST, app="a0") if k % 7 == 0 else None)
            for k in range(m)]
    for p in pods:
        if p["spec"].get("affinity") is None:
            p["spec"].pop("affinity", None)
    services = [{"metadata": {"name": "svc-%d" % a, "namespace": "default"}, "spec": {"selector": {"app": "a%d" % a}}}
                for a in range(3)]
    cl = ingest.Cluster.from_objects(nodes, (), pods, spread=kspread.SpreadListers(services=services))
    return Case(cl)


@functools.lru_cache(maxsize=None)
def aux_domains(D, Z=0, n=240, m=120):
    """A Policy's serviceAntiAffinity priority over the node label rack (D values, rack = rank % D), every pod
    under one of three services; Z > 0: SelectorSpreadPriority too, over Z zones.  The pass-A record then
    holds 4 + Z + 3 + D words, of which a workgroup publishes 64."""
    nodes = [node(i, zone=("z%02d" % (i % Z)) if Z else None, labels={"rack": "r%02d" % (i % D)}, pods=4) for i in range(n)]
    pods = [pod("x-%d" % k, {"app": "a%d" % (k % 3)}) for k in range(m)]
    services = [{"metadata": {"name": "svc-%d" % a, "namespace": "default"}, "spec": {"selector": {"app": "a%d" % a}}}
                for a in range(3)]
    cl = ingest.Cluster.from_objects(nodes, (), pods, spread=kspread.SpreadListers(services=services),
                                     aux=("service_anti_affinity", "rack"))
    prios = [("SAA", 2), ("LeastRequestedPriority", 1)] + ([("SelectorSpreadPriority", 1)] if Z else [])
    return Case(cl, prios=prios, custom={"SAA": ("serviceAntiAffinity", "rack")})


@functools.lru_cache(maxsize=None)
def record_bound(refs, n=64, m=60):
    """Pod-context records around PG_REC_MAX (6,144 bytes: 592 fixed, 16 per volume ref): every fifth pod
    mounts `refs` EBS volumes of its own (the MaxPD limits are lifted), the others one."""
    nodes = [node(i, zone="z%d" % (i % 3), pods=3) for i in range(n)]
    pods = []
    for k in range(m):
        r = refs if k % 5 == 2 else 1
        pods.append(pod("b-%d" % k, volumes=[{"name": "e%d" % j, "awsElasticBlockStore": {"volumeID": "big-%d-%d" % (k, j)}}
                                             for j in range(r)]))
    cl = ingest.Cluster.from_objects(nodes, (), pods, max_vols=(2000, 2000, 2000))
    return Case(cl)


@functools.lru_cache(maxsize=None)
def volumes9(n=210, m=330):
    """More than eight mounts on a node (the 9th and later volume slots stay in HBM): 200 nodes take no
    pods (pods = 0 above rank 9), ten take up to 40, every pod mounts its own EBS volume and, from pod 84 on
    (the ten nodes then hold eight mounts or more), one of six GCE PDs read-write: its first mount lands in
    slot 8 or later, and NoDiskConflict must find it there for the pods that bring the same disk again.  The
    EBS MaxPD limit is 11 (the count crosses slot 8 before it refuses)."""
    nodes = [node(i, zone="z%d" % (i % 3), pods=40 if i < 10 else 0) for i in range(n)]
    pods = []
    for k in range(m):
        vols = [{"name": "e", "awsElasticBlockStore": {"volumeID": "ebs-%d" % k}}]
        if k >= 84:
            vols.append({"name": "g", "gcePersistentDisk": {"pdName": "pd-%d" % (k % 6), "readOnly": False}})
        pods.append(pod("v-%d" % k, volumes=vols))
    cl = ingest.Cluster.from_objects(nodes, (), pods, max_vols=(11, 16, 16))
    return Case(cl, objs=dict(nodes=nodes, pods=pods))


# ---------------------------------------------------------------------------------- tag cycle
def _tag_nodes(n, Z=4):
    return [node(i, zone="z%d" % (i % Z), pods=110) for i in range(n)]


def _filler(k):
    """A pod without pass A, a one-class decision and no shared commit: it mounts a volume of its own
    (so it is no resource-only pod) and brings host ports (the late rows' work)."""
    return pod("f-%d" % k, ports=port_set(k), volumes=[{"name": "e", "awsElasticBlockStore": {"volumeID": "fill-%d" % k}}])


@functools.lru_cache(maxsize=None)
def tag_ipa(lead, n=400, stale=False):
    """InterPodAffinity priority pods one tag cycle apart: the pod at queue index `lead` prefers (weight
    100, per hostname) pods labelled grp=a, of which three run on node A; the pod at lead + 256 prefers
    grp=b, five on node B and three on node E; A and B sit in different late workgroups, E in the first
    one, and B carries 8 cpu more than E.  The second pod's maximum is B's 5, so E scores 10 * 3 / 5 = 6
    and B, at 10, wins against E's better LeastRequested score; a first workgroup that took the late
    workgroups' records of 256 calls back would read the first pod's maximum 3, score E 10 and choose it.
    stale=True is that reading as an input of its own (B holds three grp=b pods, the first pod's maximum):
    the host test shows that it moves the second pod to E.  The 255 pods between (and the `lead` before)
    have no pass A.  lead = 255: the first pass-A pod of the call has tag 0, the cleared word's."""
    A, B, E = 210, 390, 100
    running = late_rows(n)
    running += [pod("ra-%d" % j, {"grp": "a"}, node_name="e-%05d" % A) for j in range(3)]
    running += [pod("rb-%d" % j, {"grp": "b"} if j < (3 if stale else 5) else {}, node_name="e-%05d" % B) for j in range(5)]
    running += [pod("re-%d" % j, {"grp": "b"}, node_name="e-%05d" % E) for j in range(3)]
    running += [pod("load-b", cpu="8", mem="32Gi", node_name="e-%05d" % B)]
    pods = [_filler(k) for k in range(lead + 256 + 6)]
    pods[lead] = pod("ipa-a", ports=port_set(lead), affinity=prefer(HOST, 100, grp="a"))
    pods[lead + 256] = pod("ipa-b", ports=port_set(lead), affinity=prefer(HOST, 100, grp="b"))
    nodes = _tag_nodes(n)
    cl = ingest.Cluster.from_objects(nodes, running, pods)
    return Case(cl, first=lead, second=lead + 256, A=A, B=B, E=E, objs=dict(nodes=nodes, running=running, pods=pods))


@functools.lru_cache(maxsize=None)
def tag_spread(lead, n=400, stale=False, load=True):
    """SelectorSpread pods one tag cycle apart, with InterPodAffinity-only pods in the same slot between
    them (words 0-3 of the slot's pass-A record are rewritten every 4th call, the zone words 4.. are not):
    the pod at `lead` is selected by service sa, whose 12 running pods sit in zones z0 / z1 of late rows;
    the pod at lead + 256 by service sb, 20 running pods in zones z2 / z3."""
    running = late_rows(n)
    for j in range(12):
        running.append(pod("sa-%d" % j, {"app": "sa"}, node_name="e-%05d" % (200 + 4 * j + (j % 2))))        # z0, z1
    for j in range(20):  # z2, z3 (stale: in the first service's zones z0, z1, what its zone words say)
        running.append(pod("sb-%d" % j, {"app": "sb"}, node_name="e-%05d" % (202 + 4 * j + (j % 2) - (2 if stale else 0))))
    # every late row carries 16 of 64 cpu, so the rows that take the designed pods are the first workgroup's:
    # its z0 / z1 rows for the second pod (its service counts in z2 / z3), its z2 / z3 rows on the stale sums
    # (load=False: without that load, the layout whose designed pods land on late rows)
    if load:
        running += [pod("load-%d" % i, cpu="16", mem="64Gi", node_name="e-%05d" % i) for i in range(LATE_FROM, n)]
    running += [pod("rc-%d" % j, {"grp": "c"}, node_name="e-%05d" % 301) for j in range(2)]
    pods = [_filler(k) for k in range(lead + 256 + 6)]
    for k in range(lead + 4, lead + 256, 4):  # the same slot: IPA-only pods
        pods[k] = pod("ipa-%d" % k, ports=port_set(k), affinity=prefer(HOST, 10, grp="c"))
    pods[lead] = pod("spr-a", {"app": "sa"}, ports=port_set(lead))
    pods[lead + 256] = pod("spr-b", {"app": "sb"}, ports=port_set(lead))
    services = [{"metadata": {"name": "svc-" + a, "namespace": "default"}, "spec": {"selector": {"app": a}}} for a in ("sa", "sb")]
    cl = ingest.Cluster.from_objects(_tag_nodes(n), running, pods, spread=kspread.SpreadListers(services=services))
    return Case(cl, first=lead, second=lead + 256, objs=dict(running=running))


@functools.lru_cache(maxsize=None)
def tag_classes(lead, n=400):
    """A four-class decision, 255 one-class decisions, a four-class decision: node i carries i % 4
    PreferNoSchedule taints; the fillers tolerate every taint (K = 1), the pods at `lead` and lead + 256 none
    (K = 4), and the nodes without taints that still take them sit in a late workgroup (the rows below
    LATE_FROM and the untainted rows of the second workgroup are full)."""
    nodes = [node(i, zone="z%d" % (i % 4), pods=110, taints=["t%d" % t for t in range(i % 4)]) for i in range(n)]
    for i in range(0, 300, 4):   # untainted rows below 300: no room (one pod allowed, one running)
        nodes[i]["status"]["allocatable"]["pods"] = "1"
    running = late_rows(n) + [pod("full-%d" % i, node_name="e-%05d" % i) for i in range(0, 300, 4)]
    tol = [{"operator": "Exists"}]
    pods = []
    for k in range(lead + 256 + 6):
        p = _filler(k)
        p["spec"]["tolerations"] = tol
        pods.append(p)
    for k in (lead, lead + 256):
        pods[k] = pod("k4-%d" % k, ports=port_set(k), volumes=[{"name": "e", "awsElasticBlockStore": {"volumeID": "k4-%d" % k}}])
    cl = ingest.Cluster.from_objects(nodes, running, pods)
    return Case(cl, first=lead, second=lead + 256)


@functools.lru_cache(maxsize=None)
def tag_commit(lead, n=400, stale=False):
    """Shared-domain commits one tag cycle apart: the pods at `lead` and lead + 256 carry a required
    anti-affinity term per zone against their own label (grp=x / grp=y; the second against grp=x too, so
    it leaves the first one's zone), and two probes of each label follow at the end of the queue.  Zone =
    rank % 4, so every workgroup holds rows of every zone.  Loads (cpu a node) draw the pods by the
    least-requested priority: z2 rows carry none in the first workgroup and 16 in the late ones, z3 rows 24
    in the late workgroups and 40 in the first, z0 / z1 rows 32 (of 64).  So the first commit lands on a z2 row
    of the first workgroup, the second (barred from z2) on a z3 row of a late workgroup — its owner writes
    the commit word after the first workgroup has looked at it —, and the grp=y probes, barred from z3,
    on z2 rows of the first workgroup: exactly the rows where a first workgroup that took the node of the
    commit 256 calls back (a z2 node) would have counted grp=y, and would refuse them.
    stale=True is that miscount as an input of its own (the second pod is sent to the first one's node
    by a nodeSelector): the host test shows that it moves the grp=y probes."""
    nodes = [node(i, zone="z%d" % (i % 4), pods=110) for i in range(n)]
    running = late_rows(n)
    for i in range(n):
        z, early = i % 4, i < LATE_FROM
        cpu = {0: 32, 1: 32, 2: 0 if early else 16, 3: 40 if early else 24}[z]
        if cpu:  # (of 64 cpu and 256Gi: whole steps of the 0-10 least-requested score, cpu and memory alike)
            running.append(pod("load-%d" % i, cpu=str(cpu), mem="%dGi" % (4 * cpu), node_name="e-%05d" % i))
    pods = [_filler(k) for k in range(lead + 256 + 6)]
    pods[lead] = pod("cm-x", {"grp": "x"}, affinity=anti(ZONE, grp="x"))
    both = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [term(ZONE, grp="y"), term(ZONE, grp="x")]}}
    pods[lead + 256] = pod("cm-y", {"grp": "y"}, affinity=both)
    if stale:
        fresh = tag_commit(lead, n)
        at = fresh.cl.names[int(fresh.reference()["out"][lead])]
        pods[lead + 256] = pod("cm-y", {"grp": "y"}, affinity=anti(ZONE, grp="y"),
                               nodeSelector={HOST: at})
    for j, g in enumerate("xyxy"):
        pods[lead + 258 + j] = pod("probe-%s-%d" % (g, j), {"grp": g}, affinity=anti(ZONE, grp=g))
    cl = ingest.Cluster.from_objects(nodes, running, pods)
    return Case(cl, first=lead, second=lead + 256, probes=list(range(lead + 258, lead + 262)),
                objs=dict(nodes=nodes, running=running, pods=pods))


# ---------------------------------------------------------------------------------- C2 (ksim_persistent.hip)
@functools.lru_cache(maxsize=None)
def c2_uniform(n, m=None, taint_every=2):
    """workloads.uniform_selector_workload: selector pods that tie on every fit node (two TaintToleration
    classes), n + 40 pods of which a node takes one (cpu 5 of 8)."""
    nodes, pods = uniform_selector_workload(n, n + 40 if m is None else m, taint_every=taint_every, cpu="5", mem="1Gi")
    return Case(ingest.Cluster.from_objects(nodes, (), pods))


@functools.lru_cache(maxsize=None)
def c2_sixteen(n=203):
    nodes, pods = sixteen_class_workload(n)
    return Case(ingest.Cluster.from_objects(nodes, (), pods))


@functools.lru_cache(maxsize=None)
def c2_ports(n, m):
    """synth.c2_objects (selectors, taints, host ports, tolerations)."""
    nodes, pods = synth.c2_objects(n, m)
    return Case(ingest.Cluster.from_objects(nodes, (), pods))


@functools.lru_cache(maxsize=None)
def c2_tag_classes(lead, n=203):
    """sixteen_class_workload's nodes; a sixteen-class pod at `lead` and at lead + 256, between them pods
    that tolerate every taint and prefer no tier (K = 1; their selector keeps them off the fast kernel)."""
    nodes, p16 = sixteen_class_workload(n)
    one = {"containers": [{"resources": {"requests": {"cpu": "10m", "memory": "1Mi"}}}], "nodeSelector": {"pool": "a"},
           "tolerations": [{"operator": "Exists"}]}
    pods = [{"metadata": {"name": "one-%d" % k, "namespace": "default"}, "spec": dict(one)} for k in range(lead + 256 + 6)]
    pods[lead], pods[lead + 256] = p16[0], p16[1]
    return Case(ingest.Cluster.from_objects(nodes, (), pods), first=lead, second=lead + 256)


@functools.lru_cache(maxsize=None)
def c2_many_classes(n=1059, classes=1500):
    """One pod class per pod (each tolerates a taint key of its own) on a table that fills a workgroup's row
    budget: the pod-class tables do not fit LDS beside the rows and are read from HBM (PLayout.tables = 0)."""
    nodes, _ = uniform_selector_workload(n, 1, taint_every=2)
    pods = [{"metadata": {"name": "mc-%d" % k, "namespace": "default"},
             "spec": {"containers": [{"resources": {"requests": {"cpu": "3", "memory": "1Gi"}}}], "nodeSelector": {"pool": "a"},
                      "tolerations": [{"key": "own-%d" % k, "operator": "Exists", "effect": "PreferNoSchedule"}]}}
            for k in range(classes)]
    return Case(ingest.Cluster.from_objects(nodes, (), pods))
