"""What sweeping a volume queue costs and what it replaces, on a C2x-shaped snapshot: the C2 objects
(2,000 nodes, 2,000 pods) with the nodes in 8 zones (a tenth in none), every pod labelled app=<one of
40> and selected by that app's service, the replicas of every other app repelling each other per
hostname (required); about half of the pods mount one or two volumes — EBS or GCE PD disks from pools
of 300 ids (GCE read-only in 3 of 10), or one of 64 claims bound to zone-labelled PVs — and 300 such
pods are running.  The policy is DefaultProvider without CheckVolumeBinding.  Outages: N-1 of the first
S nodes, then every zone.
    python tools/sweep_volume_rate.py LEGS [S ...]      (default S: 1 16)
LEGS is a comma-separated list, run alternating:
    volumes   sweep_volumes(absent) on the snapshot: every outage on its own mounts and affinity state
    plain     the same queue with the volumes stripped, through sweep_affinity (the existing entry for
              this snapshot): what the volumes cost on top
    seq       what a user does without it: one ClusterCapacity run per outage on the reduced objects
`plain` and `seq` use nothing of the volume sweep, so they also run from a checkout without it.  With
`volumes` and `seq` both given, every run asserts that they agree pod for pod.
One JSON line per measurement (profiles/sweep_volumes/)."""
import copy
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "kubernetes-schedule-simulator_amd")]
from ksim import ingest, scheduler, synth  # noqa: E402
from ksim.spread import SpreadListers  # noqa: E402

legs = sys.argv[1].split(",")
sizes = [int(x) for x in sys.argv[2:]] or [1, 16]
N, P, RUNS, APPS, ZONES, RUNNING, DISKS, CLAIMS = 2_000, 2_000, 3, 40, 8, 300, 300, 64
ZONE = "failure-domain.beta.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"
nodes, pods = synth.c2_objects(N, P)
nodes, pods = copy.deepcopy(nodes), copy.deepcopy(pods)
rng = random.Random(21)
for node in nodes:
    node["metadata"]["labels"][HOST] = node["metadata"]["name"]
    if rng.random() < 0.9:
        node["metadata"]["labels"][ZONE] = "zone-%d" % rng.randrange(ZONES)
pvs, pvcs = [], []
for k in range(CLAIMS):
    src = {"awsElasticBlockStore": {"volumeID": "pv-ebs-%d" % k}} if k % 2 else {"gcePersistentDisk": {"pdName": "pv-gce-%d" % k}}
    pvs.append({"metadata": {"name": "pv-%d" % k, "labels": {ZONE: "zone-%d" % (k % ZONES)}}, "spec": src})
    pvcs.append({"metadata": {"name": "claim-%d" % k, "namespace": "default"}, "spec": {"volumeName": "pv-%d" % k}})


def volume():
    t = rng.random()
    if t < 0.4:
        return {"awsElasticBlockStore": {"volumeID": "ebs-%d" % rng.randrange(DISKS)}}
    if t < 0.8:
        return {"gcePersistentDisk": {"pdName": "gce-%d" % rng.randrange(DISKS), "readOnly": rng.random() < 0.3}}
    return {"persistentVolumeClaim": {"claimName": "claim-%d" % rng.randrange(CLAIMS)}}


for pod in pods:
    k = rng.randrange(APPS)
    pod["metadata"]["namespace"] = "default"
    pod["metadata"]["labels"] = {"app": "app-%d" % k}
    if k % 2 == 0:
        pod["spec"]["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
            {"labelSelector": {"matchLabels": {"app": "app-%d" % k}}, "topologyKey": HOST}]}}
    if rng.random() < 0.5:
        pod["spec"]["volumes"] = [volume() for _ in range(rng.randint(1, 2))]
running = []
for j in range(RUNNING):
    pod = copy.deepcopy(pods[rng.randrange(P)])
    pod["metadata"]["name"] = "run-%d" % j
    pod["spec"]["volumes"] = [volume()]
    pod["spec"]["nodeName"] = nodes[rng.randrange(N)]["metadata"]["name"]
    running.append(pod)
stripped, bare = copy.deepcopy(pods), copy.deepcopy(running)
for pod in stripped + bare:
    pod["spec"].pop("volumes", None)
md = lambda k: {"namespace": "default", "name": "app-%d" % k}  # noqa: E731
objs = dict(services=[{"metadata": md(k), "spec": {"selector": {"app": "app-%d" % k}}} for k in range(APPS)])
preds = [k for k in scheduler.DEFAULT_PREDICATES if k != "CheckVolumeBinding"]
prios = list(scheduler.DEFAULT_PRIORITIES)
Q = len(pods)


def emit(**kw):
    print(json.dumps(dict(kw, nodes=N, queue=Q, running=RUNNING)), flush=True)


def run_sweep(g, sets_, run, leg, what):
    t = time.perf_counter()
    if leg == "volumes":
        out, ctr, st = g.sweep_volumes(sets_, None, 0, Q)
    else:
        out, ctr, st = g.sweep_affinity(sets_, None, 0, Q)
    wall = time.perf_counter() - t
    S = len(sets_)
    emit(case=leg, outages=what, scenarios=S, run=run, wall_ms=round(wall * 1e3, 3), kernel_ms=round(st.kernel_ms, 3),
         launches=st.kernel_launches, failed=int((out < 0).sum()), scenario_pods_per_s=round(S * Q / wall, 1))
    return list(out)


def run_seq(cl, sets_, run, what):
    build_s = run_s = 0.0
    rows = []
    for a in sets_:
        gone = {cl.names[i] for i in a}
        t0 = time.perf_counter()
        left = [x for x in nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in running if x["spec"]["nodeName"] not in gone]
        cc = scheduler.ClusterCapacity(left, stay, list(reversed(pods)), predicates=preds, priorities=prios,
                                       collect_reasons=False, spread=SpreadListers(**objs), pvs=pvs, pvcs=pvcs)
        t1 = time.perf_counter()
        rep = cc.run()
        t2 = time.perf_counter()
        cc.scheduler.close()
        build_s += t1 - t0
        run_s += t2 - t1
        host = dict(rep.successful)
        rows.append(np.array([cl.index[host[nm]] if nm in host else -1 for nm in cl.pod_names[:Q]], np.int32))
    S = len(sets_)
    emit(case="sequential", outages=what, scenarios=S, run=run, run_ms=round(run_s * 1e3, 3), build_ms=round(build_s * 1e3, 3),
         with_build_ms=round((build_s + run_s) * 1e3, 3), failed=int(sum(int((r < 0).sum()) for r in rows)),
         scenario_pods_per_s=round(S * Q / run_s, 1))
    return rows


cl = ingest.Cluster.from_objects(nodes, running, pods, spread=SpreadListers(**objs), pvs=pvs, pvcs=pvcs)
gs = {}
if "volumes" in legs:
    gs["volumes"] = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
if "plain" in legs:
    gs["plain"] = scheduler.GenericScheduler(ingest.Cluster.from_objects(nodes, bare, stripped, spread=SpreadListers(**objs)),
                                             preds, prios, collect_reasons=False)
zones = [idx for _, idx in scheduler.outage_sets(cl, ZONE)]
plans = [("n-1", [[i] for i in range(S)]) for S in sizes] + [("zones", zones)]
emit(case="workload", volume_pods=int((np.asarray(cl.pods)["vol_class"] > 0).sum()),
     mounted_nodes=int((np.asarray(cl.volumes["slot_count"]) > 0).sum()), vol_slots=int(cl.volumes["vol_slots"]))
for leg, g in gs.items():  # warm-up
    run_sweep(g, [[0]], 0, leg, "warm-up")
if "seq" in legs:
    run_seq(cl, [[0]], 0, "warm-up")
for what, sets_ in plans:
    for run in range(1, RUNS + 1):  # alternating
        got = {}
        for leg in legs:
            got[leg] = run_seq(cl, sets_, run, what) if leg == "seq" else run_sweep(gs[leg], sets_, run, leg, what)
        if "volumes" in got and "seq" in got:  # the same question, pod for pod
            equal = bool(all(np.array_equal(x, y) for x, y in zip(got["volumes"], got["seq"])))
            emit(case="agree", legs=["volumes", "seq"], outages=what, scenarios=len(sets_), run=run, equal=equal)
            assert equal, "sweep_volumes and the sequential runs disagree (%s, run %d)" % (what, run)
        if "volumes" in got and "plain" in got:
            emit(case="volumes-change", legs=["volumes", "plain"], outages=what, scenarios=len(sets_), run=run,
                 placements=int(sum(int((x != y).sum()) for x, y in zip(got["volumes"], got["plain"]))))
for g in gs.values():
    g.close()
