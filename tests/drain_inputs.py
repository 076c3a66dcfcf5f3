"""Inputs and CPU oracle of the drain sweep (ksim_sweep_drain, include/ksim_drain.h), shared by
tests/test_sweep_drain_host.py (their properties) and tests/test_gpu_sweep_drain.py (the GPU cases).

Recipe: explain_inputs.tight_objects(n, p); the first R pods are scheduled by the C oracle under
DefaultProvider and bound (spec.nodeName) — the running pods, a pod that fits nowhere is dropped —,
the remaining pods are the queue, and the cluster is built from the nodes, the running pods and the
queue followed by the requeue_copy of every running pod: queue index Q + k is the copy of running
pod k.  The oracle of an absent set A is cpu_ref.run on the reduced cluster
(explain_inputs._reduced: the columns without A's nodes, so without the pods bound to them) over
the pod array [copies of the pods bound to A, in running order] + [queue]."""
import copy
import functools

import numpy as np

import cpu_ref
import explain_inputs as E
from ksim import abi, ingest, scheduler

SIZES = [(1100, 3600, 2600), (130, 420, 300), (65, 210, 150)]  # (n, p, R)


@functools.lru_cache(maxsize=None)
def objects(n, p, R):
    """(nodes, running pods, queue) of the recipe, as objects."""
    nodes, pods = E.tight_objects(n, p)
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    preds, prios = scheduler.provider("DefaultProvider")
    pl = scheduler.plan(cl, preds, prios)
    first = E.oracle(cl, pl.tables, pl.na_add, scheduler.make_config(preds, prios), [], 0, R)["out"]
    running = []
    for pod, w in zip(pods[:R], first):
        if w >= 0:
            pod = copy.deepcopy(pod)
            pod["spec"]["nodeName"] = cl.names[int(w)]
            running.append(pod)
    return nodes, running, pods[R:]


def resource_only(pod):
    """A copy of the pod without node selector, tolerations and host ports."""
    pod = copy.deepcopy(pod)
    pod["spec"].pop("nodeSelector", None)
    pod["spec"].pop("tolerations", None)
    for ctr in pod["spec"]["containers"]:
        ctr.pop("ports", None)
    return pod


@functools.lru_cache(maxsize=None)
def cluster(n, p, R, strip=None):
    """(cluster, Q = pods of the queue, host [len(running)] = node index of running pod k).
    strip="queue" / "prefix": the queued pods / the re-queued copies made resource_only."""
    nodes, running, queue = objects(n, p, R)
    copies = [scheduler.requeue_copy(x) for x in running]
    if strip == "queue":
        queue = [resource_only(x) for x in queue]
    if strip == "prefix":
        copies = [resource_only(x) for x in copies]
    cl = ingest.Cluster.from_objects(nodes, running, queue + copies)
    host = np.array([cl.index[x["spec"]["nodeName"]] for x in running], np.int64)
    return cl, len(queue), host


def requeue_of(n, p, R, absent, strip=None):
    """Loaded-queue indices of the copies of the running pods bound to an absent node, running order."""
    _, Q, host = cluster(n, p, R, strip)
    gone = np.zeros(n, bool)
    gone[list(absent)] = True
    return (Q + np.nonzero(gone[host])[0]).astype(np.int64)


def sets(n):
    """(label, absent set) of the cases: explain_inputs' sets, a random third and the tier outages."""
    rng = np.random.default_rng(20250114)
    out = [("first", [0]), ("none", []), ("last", [n - 1]), ("word-edge", [31, 32])]  # an empty prefix between two
    if n > 1024:
        out.append(("1023-1024", [1023, 1024]))
    out.append(("random-10pct", sorted(int(x) for x in rng.choice(n, n // 10, replace=False))))
    out.append(("random-third", sorted(int(x) for x in rng.choice(n, n // 3, replace=False))))
    return out


def all_sets(n, p, R):
    cl, _, _ = cluster(n, p, R)
    out = sets(n)
    out += [("tier-" + v, list(idx)) for v, idx in scheduler.outage_sets(cl, "tier")]
    out.append(("all-but-5-7", [i for i in range(n) if i not in (5, 7)]))
    out.append(("every-node", list(range(n))))
    return out


@functools.lru_cache(maxsize=None)
def _plan(n, p, R, strip=None):
    cl, _, _ = cluster(n, p, R, strip)
    preds, prios = scheduler.provider("DefaultProvider")
    return scheduler.plan(cl, preds, prios), scheduler.make_config(preds, prios)


def oracle_queue(cl, tables, na_add, cfg, absent, queue):
    """The reference run of the loaded pods `queue` (indices, in scheduling order) on the cluster
    without the absent nodes, from the reduced initial state and counter 0: dict(out (per queue
    position, indices of the loaded table), counter, listed, count (failed pods), pod (their queue
    positions), hist)."""
    n = cl.n_nodes
    queue = np.asarray(queue, np.int64)
    m = len(queue)
    keep = np.ones(n, bool)
    keep[list(absent)] = False
    if not keep.any() or m == 0:  # ErrNoNodesAvailable for every pod: nothing evaluated
        return dict(out=np.full(m, -1, np.int32), counter=0, listed=int(keep.sum()), count=m,
                    pod=np.arange(m, dtype=np.int32), hist=np.zeros((m, abi.NREASONS), np.int32))
    sub = E._reduced(cl, keep)
    sub.pods = np.ascontiguousarray(sub.pods[queue])
    ref, reasons, _, ctr = cpu_ref.run(sub, cfg, 0, m, threads=8, tables=tables, na_add=na_add)
    back = np.nonzero(keep)[0].astype(np.int32)
    failed = np.nonzero(ref < 0)[0].astype(np.int32)
    return dict(out=np.where(ref >= 0, back[np.maximum(ref, 0)], -1).astype(np.int32), counter=ctr,
                listed=int(keep.sum()), count=len(failed), pod=failed, hist=np.ascontiguousarray(reasons[failed]))


def oracle(n, p, R, absent, requeue=None, first=0, count=None, strip=None):
    """The drain oracle of one scenario: oracle_queue over requeue (default: the copies of the pods
    bound to the absent nodes) + [first, first + count) of the queue (default: all of it), split
    into pre (the prefix's placements), out (the range's), m = len(requeue)."""
    cl, Q, _ = cluster(n, p, R, strip)
    pl, cfg = _plan(n, p, R, strip)
    requeue = requeue_of(n, p, R, absent, strip) if requeue is None else np.asarray(requeue, np.int64)
    count = Q - first if count is None else count
    r = oracle_queue(cl, pl.tables, pl.na_add, cfg, absent, np.concatenate([requeue, np.arange(first, first + count)]))
    m = len(requeue)
    r.update(m=m, pre=r["out"][:m], out=r["out"][m:], requeue=requeue)
    return r


@functools.lru_cache(maxsize=None)
def refs(n, p, R):
    """(cluster, Q, sets, drain oracle answers, plain-outage answers of the queue alone), once."""
    cl, Q, _ = cluster(n, p, R)
    sets_ = all_sets(n, p, R)
    return cl, Q, sets_, [oracle(n, p, R, a) for _, a in sets_], [oracle(n, p, R, a, requeue=[]) for _, a in sets_]
