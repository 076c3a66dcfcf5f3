"""What sweeping full-provider policies costs and what it replaces, on a C2x-shaped snapshot: the C2
objects (2,000 nodes, 2,000 pods; taints, tolerations, selectors) with the nodes in 8 zones (a tenth in
none), every pod labelled app=<one of 40> and selected by that app's service, the replicas of every other
app repelling each other per hostname (required) and preferring other zones, every third pod with a
preferred node-affinity term, and 300 such pods running.  The handle's policy is DefaultProvider; the S
policies rescale or drop its TaintToleration, NodeAffinity, SelectorSpread and InterPodAffinity weights
and vary the map priorities (spread 3x, no Balanced, packing, ...).
    python tools/sweep_policy_rate.py LEGS [S ...]      (default S: 1 16)
LEGS is a comma-separated list, run alternating:
    policy    sweep_policy(scenarios): every policy on its own copy of the node and affinity state
    outcome   the same sweep with outcome=True: the outcome kernel and its records on top
    seq       what a user does without it: one ClusterCapacity run per policy
`seq` uses nothing of the policy sweep, so it also runs from a checkout without it.  With `policy` (or
`outcome`) and `seq` both given, every run asserts that they agree pod for pod, and with `outcome` that
the records equal a host recount from the sequential runs' placements.
One JSON line per measurement (profiles/sweep_policy/)."""
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
N, P, RUNS, APPS, ZONES, RUNNING = 2_000, 2_000, 3, 40, 8, 300
ZONE = "failure-domain.beta.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"
nodes, pods = synth.c2_objects(N, P)
nodes, pods = copy.deepcopy(nodes), copy.deepcopy(pods)
rng = random.Random(23)
for node in nodes:
    node["metadata"]["labels"][HOST] = node["metadata"]["name"]
    node["metadata"]["labels"]["disk"] = rng.choice(["ssd", "hdd"])
    if rng.random() < 0.9:
        node["metadata"]["labels"][ZONE] = "zone-%d" % rng.randrange(ZONES)
for j, pod in enumerate(pods):
    k = rng.randrange(APPS)
    pod["metadata"]["namespace"] = "default"
    pod["metadata"]["labels"] = {"app": "app-%d" % k}
    if k % 2 == 0:
        sel = {"matchLabels": {"app": "app-%d" % k}}
        pod["spec"]["affinity"] = {"podAntiAffinity": {
            "requiredDuringSchedulingIgnoredDuringExecution": [{"labelSelector": sel, "topologyKey": HOST}],
            "preferredDuringSchedulingIgnoredDuringExecution": [
                {"weight": 50, "podAffinityTerm": {"labelSelector": sel, "topologyKey": ZONE}}]}}
    if j % 3 == 0:
        pod["spec"].setdefault("affinity", {})["nodeAffinity"] = {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 5, "preference": {"matchExpressions": [{"key": "disk", "operator": "In", "values": ["ssd"]}]}}]}
running = []
for j in range(RUNNING):
    pod = copy.deepcopy(pods[rng.randrange(P)])
    pod["metadata"]["name"] = "run-%d" % j
    pod["spec"]["nodeName"] = nodes[rng.randrange(N)]["metadata"]["name"]
    running.append(pod)
md = lambda k: {"namespace": "default", "name": "app-%d" % k}  # noqa: E731
objs = dict(services=[{"metadata": md(k), "spec": {"selector": {"app": "app-%d" % k}}} for k in range(APPS)])
preds, base = scheduler.provider("DefaultProvider")
Q = len(pods)
SHORT = {"TT": "TaintTolerationPriority", "NA": "NodeAffinityPriority", "SS": "SelectorSpreadPriority",
         "IPA": "InterPodAffinityPriority", "LR": "LeastRequestedPriority", "MR": "MostRequestedPriority",
         "BRA": "BalancedResourceAllocation"}
VARIANTS = [{}, {"TT": 0}, {"TT": 3}, {"NA": 0}, {"NA": 4}, {"SS": 0}, {"SS": 3}, {"IPA": 0}, {"IPA": 2}, {"BRA": 0},
            {"LR": 0, "MR": 2}, {"SS": 3, "BRA": 0}, {"TT": 0, "NA": 0}, {"LR": 3}, {"MR": 1}, {"SS": 2, "IPA": 2}]


def policy(k):
    """The k-th policy: the provider's list with variant k's weights (0 drops the priority); past the
    variants, their LeastRequested weight grows so that the lists stay distinct."""
    w = {n: x for n, x in base}
    for short, x in VARIANTS[k % len(VARIANTS)].items():
        w[SHORT[short]] = x
    if k >= len(VARIANTS) and w.get("LeastRequestedPriority"):
        w["LeastRequestedPriority"] += k // len(VARIANTS)
    return [(n, x) for n, x in w.items() if x]


def emit(**kw):
    print(json.dumps(dict(kw, nodes=N, queue=Q, running=RUNNING)), flush=True)


def least(req, cap):
    req, cap = int(req), int(cap)
    return 0 if cap == 0 or req > cap else ((cap - req) * 10) // cap


def recount(cl, row):
    """The outcome record of one policy from its placements, on the host."""
    nzc, nzm, cnt = (np.asarray(cl.cols[k]).astype(np.int64).copy() for k in ("nz_cpu", "nz_mem", "pod_count"))
    for q, w in enumerate(row):
        if w >= 0:
            nzc[w] += int(cl.pods["nz_cpu"][q])
            nzm[w] += int(cl.pods["nz_mem"][q])
            cnt[w] += 1
    fc, fm = [0] * 11, [0] * 11
    for i in range(cl.n_nodes):
        fc[least(nzc[i], cl.cols["alloc_cpu"][i])] += 1
        fm[least(nzm[i], cl.cols["alloc_mem"][i])] += 1
    return dict(listed=cl.n_nodes, used=int((cnt > 0).sum()), free_cpu=fc, free_mem=fm)


def run_sweep(g, scen, run, leg):
    t = time.perf_counter()
    out, ctr, st = g.sweep_policy(scen, outcome=(leg == "outcome"))
    wall = time.perf_counter() - t
    S = len(scen)
    emit(case=leg, scenarios=S, run=run, wall_ms=round(wall * 1e3, 3), device_ms=round(st.device_ms, 3),
         launches=st.kernel_launches, failed=int((out < 0).sum()), distinct=len({o.tobytes() for o in out}),
         scenario_pods_per_s=round(S * Q / wall, 1))
    rec = None
    if leg == "outcome":
        rec = [dict(listed=int(g.last_outcome["listed"][s]), used=int(g.last_outcome["used"][s]),
                    free_cpu=[int(v) for v in g.last_outcome["free_cpu"][s]],
                    free_mem=[int(v) for v in g.last_outcome["free_mem"][s]]) for s in range(S)]
    return list(out), rec


def run_seq(cl, scen, run):
    build_s = run_s = 0.0
    rows = []
    for pri in scen:
        t0 = time.perf_counter()
        cc = scheduler.ClusterCapacity(nodes, running, list(reversed(pods)), predicates=preds, priorities=pri,
                                       collect_reasons=False, spread=SpreadListers(**objs))
        t1 = time.perf_counter()
        rep = cc.run()
        t2 = time.perf_counter()
        cc.scheduler.close()
        build_s += t1 - t0
        run_s += t2 - t1
        host = dict(rep.successful)
        rows.append(np.array([cl.index[host[nm]] if nm in host else -1 for nm in cl.pod_names[:Q]], np.int32))
    S = len(scen)
    emit(case="sequential", scenarios=S, run=run, run_ms=round(run_s * 1e3, 3), build_ms=round(build_s * 1e3, 3),
         with_build_ms=round((build_s + run_s) * 1e3, 3), failed=int(sum(int((r < 0).sum()) for r in rows)),
         scenario_pods_per_s=round(S * Q / run_s, 1))
    return rows, None


cl = ingest.Cluster.from_objects(nodes, running, pods, spread=SpreadListers(**objs))
g = None
if "policy" in legs or "outcome" in legs:
    g = scheduler.GenericScheduler(cl, preds, base, collect_reasons=False)
    emit(case="workload", affinity_terms=bool(g.has_affinity_terms()), spread=bool(cl.spread_active))
    for leg in legs:  # warm-up
        if leg != "seq":
            run_sweep(g, [policy(0)], 0, leg)
if "seq" in legs:
    run_seq(cl, [policy(0)], 0)
for S in sizes:
    scen = [policy(k) for k in range(S)]
    for run in range(1, RUNS + 1):  # alternating
        got = {}
        for leg in legs:
            got[leg] = run_seq(cl, scen, run) if leg == "seq" else run_sweep(g, scen, run, leg)
        for leg in ("policy", "outcome"):
            if leg in got and "seq" in got:  # the same question, pod for pod
                equal = bool(all(np.array_equal(x, y) for x, y in zip(got[leg][0], got["seq"][0])))
                emit(case="agree", legs=[leg, "seq"], scenarios=S, run=run, equal=equal)
                assert equal, "sweep_policy and the sequential runs disagree (S = %d, run %d)" % (S, run)
        if "outcome" in got and "seq" in got and run == 1:
            equal = got["outcome"][1] == [recount(cl, row) for row in got["seq"][0]]
            emit(case="outcome-agrees", scenarios=S, run=run, equal=equal)
            assert equal, "outcome records and the host recount disagree (S = %d)" % S
if g is not None:
    g.close()
