"""General sweep rate on C2 (selectors, tolerations, host ports; DefaultProvider): N-1 what-ifs of
the first S nodes in one sweep, against the same what-ifs answered one at a time — the reduced
cluster loaded into a scheduler of its own and the queue scheduled once per outage.
    python tools/sweep_general_rate.py sweep|seq|both [S ...]      (default S: 1 16 256)
`seq` uses nothing of the sweep, so it also runs on a library without the general form (KSIM_LIB).
One JSON line per measurement (profiles/sweep_general/)."""
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "kubernetes-schedule-simulator_amd")]
from ksim import ingest, scheduler, synth  # noqa: E402

what = sys.argv[1]            # sweep | seq | both
sizes = [int(x) for x in sys.argv[2:]] or [1, 16, 256]
N, P, RUNS = 5_000, 5_000, 3
nodes, pods = synth.c2_objects(N, P)
cl = ingest.Cluster.from_objects(nodes, (), pods)
preds, prios = scheduler.provider("DefaultProvider")


def reduced(keep):
    """The cluster without the nodes outside `keep`; nodeName indices follow the reduced table."""
    sub = copy.copy(cl)
    sub.cols = {k: (np.ascontiguousarray(v[..., keep]) if isinstance(v, np.ndarray) else v) for k, v in cl.cols.items()}
    sub.names = [cl.names[i] for i in np.nonzero(keep)[0]]
    sub.index = {}
    rank = np.where(keep, np.cumsum(keep) - 1, -2).astype(np.int32)
    p = np.ascontiguousarray(cl.pods).copy()
    p["host"] = np.where(p["host"] >= 0, rank[np.maximum(p["host"], 0)], p["host"])
    sub.pods = p
    return sub


def emit(**kw):
    print(json.dumps(dict(kw, nodes=N, pods=P)), flush=True)


def run_sweep(g, S, run):
    sets_ = [[i] for i in range(S)]
    t = time.perf_counter()
    out, ctr, st = g.sweep(None, 0, P, absent=sets_)
    wall = time.perf_counter() - t
    emit(case="sweep", scenarios=S, run=run, wall_ms=round(wall * 1e3, 3), kernel_ms=round(st.kernel_ms, 3),
         launches=st.kernel_launches, mode=st.mode, bound=int((out >= 0).sum()),
         scenario_pods_per_s=round(S * P / wall, 1), kernel_scenario_pods_per_s=round(S * P / (st.kernel_ms * 1e-3), 1))
    return out


def run_seq(S, run):
    host_s = load_s = sched_s = kern_ms = 0.0
    bound = 0
    rows = []
    for i in range(S):
        t0 = time.perf_counter()
        keep = np.ones(N, bool)
        keep[i] = False
        sub = reduced(keep)
        t1 = time.perf_counter()
        g = scheduler.GenericScheduler(sub, preds, prios, collect_reasons=False)
        t2 = time.perf_counter()
        out, _, st = g.schedule(0, P)
        t3 = time.perf_counter()
        g.close()
        host_s += t1 - t0
        load_s += t2 - t1
        sched_s += t3 - t2
        kern_ms += st.kernel_ms
        bound += int((out >= 0).sum())
        back = np.nonzero(keep)[0].astype(np.int32)
        rows.append(np.where(out >= 0, back[np.maximum(out, 0)], -1).astype(np.int32))
    emit(case="sequential", scenarios=S, run=run, schedule_ms=round(sched_s * 1e3, 3), load_ms=round(load_s * 1e3, 3),
         with_load_ms=round((load_s + sched_s) * 1e3, 3), host_slicing_ms=round(host_s * 1e3, 3),
         kernel_ms=round(kern_ms, 3), bound=bound, scenario_pods_per_s=round(S * P / sched_s, 1),
         scenario_pods_per_s_with_load=round(S * P / (load_s + sched_s), 1))
    return np.stack(rows)


g = None
if what in ("sweep", "both"):
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    g.sweep(None, 0, P, absent=[[0]])  # warm-up
if what in ("seq", "both"):
    run_seq(1, 0)  # warm-up
for S in sizes:
    for run in range(1, RUNS + 1):  # alternating
        a = run_sweep(g, S, run) if g is not None else None
        b = run_seq(S, run) if what in ("seq", "both") else None
        if a is not None and b is not None:
            emit(case="agree", scenarios=S, run=run, equal=bool(np.array_equal(a, b)))
if g is not None:
    g.close()
