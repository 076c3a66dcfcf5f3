"""What sweeping an inter-pod affinity queue costs and what it replaces, on a C2x-shaped snapshot: the
C2 objects (2,000 nodes, 2,000 pods; DefaultProvider) with the nodes in 8 zones (a tenth in none),
every pod labelled app=<one of 40> and selected by that app's service; the replicas of every other
app repel each other per hostname (required), every fourth app's per zone (required), and every third
app prefers zones without its replicas; 200 replicas are running.  Outages: N-1 of the first S nodes,
then every zone.
    python tools/sweep_affinity_rate.py LEGS [S ...]      (default S: 1 16)
LEGS is a comma-separated list, run alternating:
    affinity  sweep_affinity(absent) on the snapshot: every outage on its own affinity state
    plain     the same queue with the affinity terms stripped, through sweep(None, absent=...)
              (ksim_sweep_nodes over a SelectorSpread queue): what the terms cost on top
    seq       what a user does without it: one ClusterCapacity run per outage on the reduced objects
`plain` and `seq` use nothing of the affinity sweep, so they also run from a checkout without it.
One JSON line per measurement (profiles/sweep_affinity/)."""
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
N, P, RUNS, APPS, ZONES, RUNNING = 2_000, 2_000, 3, 40, 8, 200
ZONE = "failure-domain.beta.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"
nodes, pods = synth.c2_objects(N, P)
nodes, pods = copy.deepcopy(nodes), copy.deepcopy(pods)
rng = random.Random(20)
for node in nodes:
    node["metadata"]["labels"][HOST] = node["metadata"]["name"]
    if rng.random() < 0.9:
        node["metadata"]["labels"][ZONE] = "zone-%d" % rng.randrange(ZONES)


def terms(k):
    sel = {"matchLabels": {"app": "app-%d" % k}}
    anti = {}
    req = [{"labelSelector": sel, "topologyKey": key} for key, on in ((HOST, k % 2 == 0), (ZONE, k % 4 == 1)) if on]
    if req:
        anti["requiredDuringSchedulingIgnoredDuringExecution"] = req
    if k % 3 == 0:
        anti["preferredDuringSchedulingIgnoredDuringExecution"] = [
            {"weight": 50, "podAffinityTerm": {"labelSelector": sel, "topologyKey": ZONE}}]
    return {"podAntiAffinity": anti} if anti else None


for pod in pods:
    k = rng.randrange(APPS)
    pod["metadata"]["labels"] = {"app": "app-%d" % k}
    if terms(k):
        pod["spec"]["affinity"] = terms(k)
running = []
for j in range(RUNNING):
    pod = copy.deepcopy(pods[rng.randrange(P)])
    pod["metadata"]["name"] = "run-%d" % j
    pod["spec"]["nodeName"] = nodes[rng.randrange(N)]["metadata"]["name"]
    running.append(pod)
stripped = copy.deepcopy(pods)
for pod in stripped:
    pod["spec"].pop("affinity", None)
bare = copy.deepcopy(running)
for pod in bare:
    pod["spec"].pop("affinity", None)
md = lambda k: {"namespace": "default", "name": "app-%d" % k}  # noqa: E731
objs = dict(services=[{"metadata": md(k), "spec": {"selector": {"app": "app-%d" % k}}} for k in range(APPS)])
preds, prios = scheduler.provider("DefaultProvider")
Q = len(pods)


def emit(**kw):
    print(json.dumps(dict(kw, nodes=N, queue=Q, running=RUNNING)), flush=True)


def run_sweep(g, sets_, run, leg, what):
    t = time.perf_counter()
    if leg == "affinity":
        out, ctr, st = g.sweep_affinity(sets_, None, 0, Q)
    else:
        out, ctr, st = g.sweep(None, 0, Q, absent=sets_)
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
        cc = scheduler.ClusterCapacity(left, stay, list(reversed(pods)), provider_name="DefaultProvider", collect_reasons=False,
                                       spread=SpreadListers(**objs))
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


cl = ingest.Cluster.from_objects(nodes, running, pods, spread=SpreadListers(**objs))
gs = {}
if "affinity" in legs:
    gs["affinity"] = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
if "plain" in legs:
    gs["plain"] = scheduler.GenericScheduler(ingest.Cluster.from_objects(nodes, bare, stripped, spread=SpreadListers(**objs)),
                                             preds, prios, collect_reasons=False)
zones = [idx for _, idx in scheduler.outage_sets(cl, ZONE)]
plans = [("n-1", [[i] for i in range(S)]) for S in sizes] + [("zones", zones)]
for leg, g in gs.items():  # warm-up
    run_sweep(g, [[0]], 0, leg, "warm-up")
if "seq" in legs:
    run_seq(cl, [[0]], 0, "warm-up")
for what, sets_ in plans:
    for run in range(1, RUNS + 1):  # alternating
        got = {}
        for leg in legs:
            got[leg] = run_seq(cl, sets_, run, what) if leg == "seq" else run_sweep(gs[leg], sets_, run, leg, what)
        if "affinity" in got and "seq" in got:  # the same question, pod for pod
            emit(case="agree", legs=["affinity", "seq"], outages=what, scenarios=len(sets_), run=run,
                 equal=bool(all(np.array_equal(x, y) for x, y in zip(got["affinity"], got["seq"]))))
        if "affinity" in got and "plain" in got:
            emit(case="terms-change", legs=["affinity", "plain"], outages=what, scenarios=len(sets_), run=run,
                 placements=int(sum(int((x != y).sum()) for x, y in zip(got["affinity"], got["plain"]))))
for g in gs.values():
    g.close()
