"""Masked sweep rate on C5's cluster: 4,096 scenarios, each with a different 1 % of the nodes
absent, against the unmasked sweep of the same scenarios; and the N-1 case (20,000 scenarios x 300 pods).
    python tools/sweep_nodes_rate.py tree|scan
One JSON line per measurement (profiles/sweep_nodes/masked_rate.jsonl)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "kubernetes-schedule-simulator_amd")]
from ksim import scheduler, synth  # noqa: E402

form = sys.argv[1]            # tree | scan
if form == "scan":
    os.environ["KSIM_SWEEP_SCAN"] = "1"
N, P, S = 20_000, 5_000, 4_096
cl, preds, scen = synth.config_c5(N, P)
scen = scen[:S]
rng = np.random.default_rng(5)
sets_ = [np.sort(rng.choice(N, N // 100, replace=False)) for _ in range(S)]
t0 = time.perf_counter()
scheduler.absent_mask(N, sets_)
mask_s = time.perf_counter() - t0
g = scheduler.GenericScheduler(cl, preds, scen[0], collect_reasons=False)


def timed(fn, reps):
    fn()  # warm-up
    rows = []
    for _ in range(reps):
        t = time.perf_counter()
        out, ctr, st = fn()
        rows.append((time.perf_counter() - t, st.kernel_ms, st.device_ms, st.kernel_launches, st.mode, int((out >= 0).sum())))
    return rows


def emit(case, rows, pods, nscen):
    for k, (wall, kms, dms, launches, mode, bound) in enumerate(rows):
        print(json.dumps({"case": case, "form": form, "run": k + 1, "scenarios": nscen, "pods": pods, "nodes": N,
                          "wall_ms": round(wall * 1e3, 3), "kernel_ms": round(kms, 3), "device_ms": round(dms, 3),
                          "launches": launches, "mode": mode, "bound": bound,
                          "scenario_pods_per_s": round(nscen * pods / wall, 1)}), flush=True)


emit("unmasked", timed(lambda: g.sweep(scen, 0, P), 3), P, S)
emit("masked-1pct", timed(lambda: g.sweep(scen, 0, P, absent=sets_), 3), P, S)
emit("unmasked", timed(lambda: g.sweep(scen, 0, P), 3), P, S)
# N-1: every node in turn, the scheduler's own policy, 300 pods
n1 = [[i] for i in range(N)]
emit("n-1", timed(lambda: g.sweep(None, 0, 300, absent=n1), 2), 300, N)
print(json.dumps({"case": "absent_mask", "seconds_for_4096x1pct": round(mask_s, 3)}), flush=True)
