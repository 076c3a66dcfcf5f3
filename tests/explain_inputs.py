"""Inputs and CPU oracle of the explained scenario sweep (ksim_sweep_explain), shared by
tests/test_sweep_explain_host.py (their properties) and tests/test_gpu_sweep_explain.py (the GPU
cases).  The checker is cpu_ref.run on the reduced cluster: its histograms are over exactly the
nodes the scenario lists."""
import copy
import functools

import numpy as np

import cpu_ref
from ksim import abi, ingest, scheduler, synth

MAP_POLICIES = [[("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)],
                [("MostRequestedPriority", 2), ("BalancedResourceAllocation", 1)]]


def _reduced(cl, keep):
    """The cluster without the nodes outside `keep` (as tests/test_gpu_sweep_general.py reduces it); a
    queued pod's nodeName index becomes the rank in the reduced table, or -2 ("no such node", the
    value ingest uses) for a node left out."""
    sub = copy.copy(cl)
    sub.cols = {k: (np.ascontiguousarray(v[..., keep]) if isinstance(v, np.ndarray) else v) for k, v in cl.cols.items()}
    sub.names = [cl.names[i] for i in np.nonzero(keep)[0]]
    sub.index = {}
    rank = np.where(keep, np.cumsum(keep) - 1, -2).astype(np.int32)
    pods = np.ascontiguousarray(cl.pods).copy()
    host = pods["host"]
    pods["host"] = np.where(host >= 0, rank[np.maximum(host, 0)], host)
    sub.pods = pods
    return sub


def tight_objects(n, p, seed=2):
    """synth.c2_objects with every node's allocatable tightened so that the queue overflows the
    cluster on several resources at once: cpu // 8, memory Gi // 32, pods 2 + i % 3 for the i-th
    node of the returned list."""
    nodes, pods = synth.c2_objects(n, p, seed=seed)
    for i, node in enumerate(nodes):
        a = node["status"]["allocatable"]
        a["cpu"] = str(int(a["cpu"]) // 8)
        a["memory"] = "%dGi" % (int(a["memory"][:-2]) // 32)
        a["pods"] = str(2 + i % 3)
    return nodes, pods


@functools.lru_cache(maxsize=None)
def tight_cluster(n, p):
    nodes, pods = tight_objects(n, p)
    return ingest.Cluster.from_objects(nodes, (), pods)


@functools.lru_cache(maxsize=None)
def c3_cluster(n=1100, p=60000, seed=3):
    """The resource-only input: (cluster, predicates, priorities)."""
    return synth.config_c3(n, p, seed)


def oracle(cl, tables, na_add, cfg, absent, first=0, count=None, state=None, counter=0):
    """The reference run of pods [first, first + count) on the cluster without the absent nodes, from
    the node state `state` (default: as loaded) and lastNodeIndex `counter`: dict(out (placements as
    indices of the loaded table), counter, listed, count (failed pods), pod (their indices relative
    to first, queue order), hist ([count][NREASONS]))."""
    n = cl.n_nodes
    count = len(cl.pods) - first if count is None else count
    keep = np.ones(n, bool)
    keep[list(absent)] = False
    if not keep.any():  # ErrNoNodesAvailable for every pod: nothing evaluated
        return dict(out=np.full(count, -1, np.int32), counter=counter, listed=0, count=count,
                    pod=np.arange(count, dtype=np.int32), hist=np.zeros((count, abi.NREASONS), np.int32))
    sub = _reduced(cl, keep)
    if state is not None:  # an absent node takes the pods already on it along
        state = {k: np.ascontiguousarray(v[..., keep]) for k, v in state.items()}
    ref, reasons, _, ctr = cpu_ref.run(sub, cfg, first, count, threads=8, state=state, counter=counter, tables=tables,
                                       na_add=na_add)
    back = np.nonzero(keep)[0].astype(np.int32)
    failed = np.nonzero(ref < 0)[0].astype(np.int32)
    return dict(out=np.where(ref >= 0, back[np.maximum(ref, 0)], -1).astype(np.int32), counter=ctr,
                listed=int(keep.sum()), count=len(failed), pod=failed,
                hist=np.ascontiguousarray(reasons[failed]))


def general_sets(n):
    """(label, absent set) of the general-form cases."""
    rng = np.random.default_rng(20250114)
    sets_ = [("none", []), ("first", [0]), ("last", [n - 1]), ("word-edge", [31, 32])]
    if n > 1024:
        sets_.append(("1023-1024", [1023, 1024]))
    sets_.append(("random-10pct", sorted(int(x) for x in rng.choice(n, n // 10, replace=False))))
    # all but one node reaches at most five reason slots on this input (node 7: four), two nodes six
    sets_.append(("all-but-5-7", [i for i in range(n) if i not in (5, 7)]))
    sets_.append(("every-node", list(range(n))))
    return sets_


@functools.lru_cache(maxsize=None)
def general_refs(n, p):
    """(cluster, absent sets, oracle answers) of the tightened recipe under DefaultProvider, once."""
    cl = tight_cluster(n, p)
    preds, prios = scheduler.provider("DefaultProvider")
    tabs = scheduler.plan(cl, preds, prios)
    cfg = scheduler.make_config(preds, prios)
    sets_ = general_sets(n)
    return cl, sets_, [oracle(cl, tabs.tables, tabs.na_add, cfg, a) for _, a in sets_]


def resource_sets(n):
    rng = np.random.default_rng(20250115)
    return [("none", []), ("first", [0]), ("word-edge", [31, 32, n - 1]),
            ("random-10pct", sorted(int(x) for x in rng.choice(n, n // 10, replace=False))),
            ("every-node", list(range(n)))]


# The resource-only forms keep their quantities exact in float64 and refuse a range whose pods could
# push a node past 2^48: 60,000 pods of up to 8 GiB are one such range.  The cases therefore
# schedule() the first RES_FIRST pods, which all fit, and sweep the rest from that state.
RES_FIRST = 30000


@functools.lru_cache(maxsize=None)
def resource_prefix():
    """(placements, node state, lastNodeIndex) of the reference after pods [0, RES_FIRST) of the
    resource-only input under its own policy."""
    cl, preds, prios = c3_cluster()
    pre, _, state, ctr = cpu_ref.run(cl, scheduler.make_config(preds, prios), 0, RES_FIRST, threads=8)
    return pre, state, ctr


@functools.lru_cache(maxsize=None)
def resource_refs(weighted, count=None):
    """(cluster, scenarios, absent sets, oracle answers) of the resource-only input swept from pod
    RES_FIRST on: with absent sets under its own policy, or (weighted) two map policies and no node
    absent."""
    cl, preds, prios = c3_cluster()
    _, state, ctr = resource_prefix()
    if weighted:
        scen, sets_ = MAP_POLICIES, [("policy-0", []), ("policy-1", [])]
        cfgs = [scheduler.make_config(preds, pri) for pri in scen]
    else:
        scen, sets_ = None, resource_sets(cl.n_nodes)
        cfgs = [scheduler.make_config(preds, prios)] * len(sets_)
    count = len(cl.pods) - RES_FIRST if count is None else count
    return cl, scen, sets_, [oracle(cl, None, None, cfg, a, RES_FIRST, count, state=state, counter=ctr)
                             for cfg, (_, a) in zip(cfgs, sets_)]


NODENAME_POD = 100


@functools.lru_cache(maxsize=None)
def nodename_input():
    """The Ready, schedulable nodes of the tightened recipe at (130, 420) — every node reaches
    GeneralPredicates — with pod NODENAME_POD of the queue naming the node the reference binds it to
    anyway.  Returns (cluster, index of that node)."""
    nodes, pods = tight_objects(130, 420)
    nodes = [x for x in nodes if x["status"]["conditions"][0]["status"] == "True" and not x["spec"].get("unschedulable")]
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    preds, prios = scheduler.provider("DefaultProvider")
    pl = scheduler.plan(cl, preds, prios)
    name = cl.names[int(oracle(cl, pl.tables, pl.na_add, scheduler.make_config(preds, prios), [])["out"][NODENAME_POD])]
    pods[NODENAME_POD]["spec"]["nodeName"] = name
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    return cl, cl.index[name]


def binds_after_failures(out):
    """How often a bound pod follows a failed one in the queue."""
    return int(((out[1:] >= 0) & (out[:-1] < 0)).sum())
