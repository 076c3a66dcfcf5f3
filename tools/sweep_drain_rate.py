"""What re-queueing the pods of lost nodes costs in a sweep and what it replaces, on the tightened C2
objects (every node's allocatable cut to cpu // 8, memory // 32, 2 + i % 3 pods; DefaultProvider) with
the first half of the queue pre-bound as running pods (scheduled once, on the GPU, and bound to the
nodes they got): N-1 what-ifs of the first S nodes.
    python tools/sweep_drain_rate.py LEGS [S ...]      (default S: 1 16 256)
LEGS is a comma-separated list, run alternating:
    drain    one sweep_drain: per outage the evicted pods' copies, then the queue
    drain0   the same with count=0: only re-host the evicted pods
    plain    sweep(None, absent=...) of the queue without re-queueing: what the prefix costs
    seq      what a user does without it: per outage one scheduler loaded with the reduced cluster and
             one schedule() of the evicted copies + queue
`plain` and `seq` use nothing of ksim_sweep_drain, so they also run from a checkout without it.
One JSON line per measurement (profiles/sweep_drain/)."""
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "kubernetes-schedule-simulator_amd")]
from ksim import ingest, scheduler, synth  # noqa: E402

legs = sys.argv[1].split(",")
sizes = [int(x) for x in sys.argv[2:]] or [1, 16, 256]
N, P, R, RUNS = 5_000, 16_000, 8_000, 3
nodes, pods = synth.c2_objects(N, P)
for i, node in enumerate(nodes):
    a = node["status"]["allocatable"]
    a["cpu"] = str(int(a["cpu"]) // 8)
    a["memory"] = "%dGi" % (int(a["memory"][:-2]) // 32)
    a["pods"] = str(2 + i % 3)
preds, prios = scheduler.provider("DefaultProvider")


def recreated(pod):
    """The evicted pod as its controller recreates it (scheduler.requeue_copy, spelled out so that the
    plain and seq legs run from a checkout without it)."""
    new = copy.deepcopy({k: v for k, v in pod.items() if k != "status"})
    new["spec"].pop("nodeName", None)
    return new


# the running pods: the first R pods where one schedule() puts them
cl0 = ingest.Cluster.from_objects(nodes, (), pods)
g0 = scheduler.GenericScheduler(cl0, preds, prios, collect_reasons=False)
bound, _, _ = g0.schedule(0, R)
g0.close()
running = []
for pod, w in zip(pods[:R], bound):
    if w >= 0:
        pod = copy.deepcopy(pod)
        pod["spec"]["nodeName"] = cl0.names[int(w)]
        running.append(pod)
queue = pods[R:]
Q = len(queue)
cl = ingest.Cluster.from_objects(nodes, running, queue + [recreated(x) for x in running])
host = np.array([cl.index[x["spec"]["nodeName"]] for x in running], np.int64)


def requeue_of(i):
    """Loaded-queue indices of the copies of the pods running on node i, in running order."""
    return Q + np.nonzero(host == i)[0]


def reduced(keep, order):
    """The cluster without the nodes outside `keep`, its pod queue the loaded pods `order`."""
    sub = copy.copy(cl)
    sub.cols = {k: (np.ascontiguousarray(v[..., keep]) if isinstance(v, np.ndarray) else v) for k, v in cl.cols.items()}
    sub.names = [cl.names[i] for i in np.nonzero(keep)[0]]
    sub.index = {}
    rank = np.where(keep, np.cumsum(keep) - 1, -2).astype(np.int32)
    p = np.ascontiguousarray(cl.pods[order]).copy()
    p["host"] = np.where(p["host"] >= 0, rank[np.maximum(p["host"], 0)], p["host"])
    sub.pods = p
    return sub


def emit(**kw):
    print(json.dumps(dict(kw, nodes=N, running=len(running), queue=Q)), flush=True)


def run_drain(g, S, run, leg):
    sets_ = [[i] for i in range(S)]
    requeue = [requeue_of(i) for i in range(S)]
    count = 0 if leg == "drain0" else Q
    t = time.perf_counter()
    out, pre, ctr, st = g.sweep_drain(sets_, requeue, 0, count)
    wall = time.perf_counter() - t
    total = sum(len(x) for x in pre) + S * count
    emit(case=leg, scenarios=S, run=run, wall_ms=round(wall * 1e3, 3), kernel_ms=round(st.kernel_ms, 3),
         launches=st.kernel_launches, evicted=int(sum(len(x) for x in pre)),
         stranded=int(sum(int((x < 0).sum()) for x in pre)), failed=int((out < 0).sum()),
         scenario_pods_per_s=round(total / wall, 1))
    return [np.concatenate([x, o]) for x, o in zip(pre, out)]


def run_plain(g, S, run):
    t = time.perf_counter()
    out, ctr, st = g.sweep(None, 0, Q, absent=[[i] for i in range(S)])
    wall = time.perf_counter() - t
    emit(case="plain", scenarios=S, run=run, wall_ms=round(wall * 1e3, 3), kernel_ms=round(st.kernel_ms, 3),
         launches=st.kernel_launches, failed=int((out < 0).sum()), scenario_pods_per_s=round(S * Q / wall, 1))
    return list(out)


def run_seq(S, run):
    load_s = sched_s = kern_ms = 0.0
    rows, total = [], 0
    for i in range(S):
        keep = np.ones(N, bool)
        keep[i] = False
        order = np.concatenate([requeue_of(i), np.arange(Q)])
        sub = reduced(keep, order)
        t1 = time.perf_counter()
        g = scheduler.GenericScheduler(sub, preds, prios, collect_reasons=False)
        t2 = time.perf_counter()
        out, _, st = g.schedule(0, len(order))
        t3 = time.perf_counter()
        g.close()
        load_s += t2 - t1
        sched_s += t3 - t2
        kern_ms += st.kernel_ms
        total += len(order)
        back = np.nonzero(keep)[0].astype(np.int32)
        rows.append(np.where(out >= 0, back[np.maximum(out, 0)], -1).astype(np.int32))
    emit(case="sequential", scenarios=S, run=run, schedule_ms=round(sched_s * 1e3, 3), load_ms=round(load_s * 1e3, 3),
         with_load_ms=round((load_s + sched_s) * 1e3, 3), kernel_ms=round(kern_ms, 3),
         failed=int(sum(int((r < 0).sum()) for r in rows)), scenario_pods_per_s=round(total / sched_s, 1))
    return rows


def same(a, b):
    """Equal placements over the rows of a: all of b's, or (drain0) their prefix part."""
    return all(np.array_equal(x, y[:len(x)]) for x, y in zip(a, b))


g = None
sweeps = [leg for leg in legs if leg != "seq"]
if sweeps:
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    for leg in sweeps:  # warm-up
        if leg == "plain":
            g.sweep(None, 0, Q, absent=[[0]])
        else:
            g.sweep_drain([[0]], [requeue_of(0)], 0, 0 if leg == "drain0" else Q)
if "seq" in legs:
    run_seq(1, 0)  # warm-up
for S in sizes:
    for run in range(1, RUNS + 1):  # alternating
        got = {}
        for leg in legs:
            got[leg] = run_seq(S, run) if leg == "seq" else (run_plain(g, S, run) if leg == "plain" else run_drain(g, S, run, leg))
        # drain and seq answer the same question pod for pod; drain0 is their prefix part
        if "drain" in got and "seq" in got:
            emit(case="agree", legs=["drain", "seq"], scenarios=S, run=run, equal=bool(same(got["drain"], got["seq"])))
        for full in ("drain", "seq"):
            if "drain0" in got and full in got:
                emit(case="agree", legs=["drain0", full], part="prefix", scenarios=S, run=run,
                     equal=bool(same(got["drain0"], got[full])))
        if "plain" in got:
            for full in ("drain", "seq"):
                if full in got:  # how many outages' queue placements the re-queued pods change
                    moved = sum(1 for x, y in zip(got["plain"], got[full]) if not np.array_equal(x, y[-Q:]))
                    emit(case="prefix-changes-queue", legs=["plain", full], scenarios=S, run=run, outages_changed=moved)
if g is not None:
    g.close()
