"""The input of tests/test_gpu_sweep_scratch.py: one cluster whose queue holds a resource-only range
and a general range, so that one scheduler can be taken through every sweep form.

1,100 nodes of synth.c2_objects (above 1,024: select segments of two rows, and 1100 % 32 != 0: a
ragged last node-set word).  Pods 0-39 request cpu and memory only and tolerate every taint, so no
taint predicate or reduce priority tells nodes apart for them: the tree and scan forms.  Pods 40-79
are c2_objects' own (node selectors, host ports, tolerations, BestEffort): the general form."""
import functools

import numpy as np

from ksim import abi, ingest, scheduler, synth

N, FAST, GENERAL = 1100, 40, 40
CAP = 3  # explain records kept per scenario


@functools.lru_cache(maxsize=None)
def cluster():
    nodes, c2 = synth.c2_objects(N, GENERAL, seed=2)
    cpus, mems = ["100m", "250m", "500m", "1", "2"], ["128Mi", "256Mi", "512Mi", "1Gi", "2Gi"]
    plain = [{"metadata": {"name": "plain-%d" % k, "namespace": "default"},
              "spec": {"containers": [{"resources": {"requests": {"cpu": cpus[k % 5], "memory": mems[(k // 5) % 5]}}}],
                       "tolerations": [{"operator": "Exists"}]}} for k in range(FAST)]
    cl = ingest.Cluster.from_objects(nodes, (), plain + c2)
    pods = cl.pods
    assert cl.n_nodes == N and len(pods) == FAST + GENERAL
    # pods 0-39: nothing but cpu / memory requests for the device to look at ...
    need = abi.POD_NEED_SELECTOR | abi.POD_NEED_TAINTS | abi.POD_NEED_SVC_AFFINITY
    head = pods[:FAST]
    assert not (head["flags"] & need).any() and not head["port_cnt"].any() and (head["host"] == -1).all()
    assert not head["scalar_cnt"].any() and not head["req_gpu"].any() and not head["req_eph"].any()
    # ... and one reduce class under the DefaultProvider's TaintToleration and NodeAffinity priorities
    preds, prios = scheduler.provider("DefaultProvider")
    tabs = scheduler.plan(cl, preds, prios).tables
    k = (np.asarray(tabs["n_tt"]) * np.asarray(tabs["n_na"]))[head["cls"]]
    assert (k == 1).all()
    # pods 40-79 cannot silently take the fast forms
    tail = pods[FAST:]
    assert (tail["port_cnt"] > 0).any() or (tail["flags"] & abi.POD_NEED_SELECTOR).any()
    return cl


def node_sets():
    rng = np.random.default_rng(20240611)
    return [[], [0], [N - 1], [31, 32], sorted(int(x) for x in rng.choice(N, N // 10, replace=False))]


def requeue():
    """A two-pod prefix per scenario: pairs from both ranges, one pod index shared by two scenarios."""
    return [[0, 41], [45, 7], [60, 61], [41, 79], [12, 13]]
