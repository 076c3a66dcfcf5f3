"""CPU-only tests of the scenario sweep's general form: the node cap mirrored in the binding, the
header's account of which pods ksim_sweep / ksim_sweep_nodes take, the unchanged C ABI, and the
properties of the input builders (tests/workloads.py) that tests/test_gpu_sweep_general_edges.py
relies on, under the C oracle."""
import os
import re

import numpy as np
import pytest

import cpu_ref
from ksim import abi
from workloads import sixteen_class_workload, uniform_selector_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ksim.h")
SWEEP_H = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc", "ksim_sweep.h")


def _comment_before(src, decl):
    """The block comment that ends right before the declaration."""
    end = src.index(decl)
    start = src.rindex("/*", 0, end)
    assert src[start:end].rstrip().endswith("*/")
    return " ".join(src[start:end].replace("*", " ").split())


def test_node_cap_is_mirrored():
    m = re.search(r"^#define\s+KSIM_SWEEP_GENERAL_MAX_NODES\s+(\d+)", open(SWEEP_H).read(), re.M)
    assert m and int(m.group(1)) == abi.SWEEP_GENERAL_MAX_NODES == 38400
    # one uint32 per node within 150 KiB of LDS
    assert abi.SWEEP_GENERAL_MAX_NODES * 4 == 150 * 1024
    text = _comment_before(open(HEADER).read(), "int ksim_sweep(")
    assert "38,400" in text and "KSIM_SWEEP_GENERAL_MAX_NODES" in text


def test_header_no_longer_requires_resource_only_pods():
    src = open(HEADER).read()
    for decl in ("int ksim_sweep(", "int ksim_sweep_nodes("):
        text = _comment_before(src, decl)
        assert "must be resource-only" not in text, decl
    sweep = _comment_before(src, "int ksim_sweep(")
    for word in ("host ports", "tolerations", "nodeName", "inter-pod affinity", "volume", "node-sharded",
                 "KSIM_MAX_RCLASS", "NodePreferAvoidPods"):
        assert word in sweep, word
    assert "general form" in _comment_before(src, "int ksim_sweep_nodes(")


def test_abi_is_unchanged():
    L = abi.lib()
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7
    assert "ksim_sweep" in abi.EXPORTS and "ksim_sweep_nodes" in abi.EXPORTS
    assert not any("general" in name for name in abi.EXPORTS)
    assert len(abi.EXPORTS) == len(set(abi.EXPORTS)) == 33
    for name in abi.EXPORTS:
        assert hasattr(L, name), name


# ---- the input builders of tests/test_gpu_sweep_general_edges.py, under the C oracle: the
# properties the GPU cases are chosen for, so an edit of a builder cannot hollow those cases out
def _default_run(nodes, pods, counter=0):
    """(cluster, plan, oracle placements, final counter) of the queue under DefaultProvider."""
    from ksim import ingest, scheduler
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    preds, prios = scheduler.provider("DefaultProvider")
    pl = scheduler.plan(cl, preds, prios)
    out, _, _, ctr = cpu_ref.run(cl, scheduler.make_config(preds, prios), 0, len(cl.pods), threads=4, counter=counter,
                                 tables=pl.tables, na_add=pl.na_add)
    return cl, pl, out, ctr


def _reduce_classes(cl, pl):
    """K of every queued pod: TaintToleration x NodeAffinity classes of its pod class."""
    return (np.asarray(pl.tables["n_tt"]) * np.asarray(pl.tables["n_na"]))[cl.pods["cls"]]


@pytest.mark.parametrize("n,counter", [(1027, 0), (2051, 0), (1027, 2**32 - 5)])
def test_uniform_selector_workload_ties_on_every_fit_node(n, counter):
    p = 2 * n + 7
    cl, pl, out, ctr = _default_run(*uniform_selector_workload(n, p), counter=counter)
    assert cl.names == ["u-%05d" % i for i in range(n)]  # index order = name order
    assert (cl.pods["flags"] & abi.POD_NEED_SELECTOR).all()  # not resource-only: the general form
    assert (_reduce_classes(cl, pl) == 1).all()
    decoys = [0, n // 2, n - 1]
    m = n - 3
    rest = np.setdiff1d(np.arange(n), decoys)
    # C starts at m and shrinks by one per pod: each round of m pods visits every fit node once
    assert np.array_equal(np.sort(out[:m]), rest)
    assert np.array_equal(np.sort(out[m:2 * m]), rest)
    assert (out >= 0).all() and not np.isin(out, decoys).any()
    assert ctr == counter + p  # more than one node fits every pod


def test_uniform_selector_workload_with_taints_has_two_classes_that_both_win():
    n, p = 1027, 4115
    cl, pl, out, ctr = _default_run(*uniform_selector_workload(n, p, taint_every=2, cpu="2", mem="4Gi"))
    assert (_reduce_classes(cl, pl) == 2).all()
    assert int((out >= 0).sum()) == 4096 and (out[-19:] == -1).all()  # four pods a node, 19 FitErrors
    bound = out[out >= 0]
    assert int((bound % 2 == 1).sum()) == 2048  # the odd nodes carry the taint
    assert np.count_nonzero(np.diff(bound % 2)) >= 1  # the winning class changes during the run
    assert not np.isin(out, [0, n // 2, n - 1]).any()


def test_sixteen_class_workload_reaches_the_class_cap():
    cl, pl, out, _ = _default_run(*sixteen_class_workload(203, 4))
    n = cl.n_nodes
    assert cl.names == ["k-%05d" % i for i in range(n)]
    assert len(cl.pods) == 4 * n + 7 == 819
    assert abi.MAX_RCLASS == 16 and (_reduce_classes(cl, pl) == 16).all()
    assert int((out >= 0).sum()) == 804
    pairs = {(int(i) % 4, (int(i) // 4) % 4) for i in out[out >= 0]}  # (taints, tier) of the nodes that received pods
    assert len(pairs) == 16
    # Several classes win together: replay the oracle's placements with the totals worked out by hand
    # (LeastRequested with the pod as the k + 1-th quarter of the node, BalancedResourceAllocation 10
    # or 0 on the node the pod fills, TaintToleration and NodeAffinity normalised over the fit nodes;
    # the other DefaultProvider priorities are one value on every node here) and count the pods whose
    # nodes at the best total belong to more than one class.
    idx = np.arange(n)
    tv, av = idx % 4, 10 * ((idx // 4) % 4)
    cnt = np.zeros(n, np.int64)
    together = most = 0
    for w in out:
        fit = (cnt < 4) & (idx != 0) & (idx != n - 1)
        if not fit.any():
            assert w == -1
            continue
        mt, ma = int(tv[fit].max()), int(av[fit].max())
        total = ((6 - 2 * cnt) * 10 // 8 + np.where(cnt == 3, 0, 10) + (10 - 10 * tv // mt if mt else 10) +
                 (10 * av // ma if ma else 0))
        tied = fit & (total == total[fit].max())
        assert tied[w]  # the oracle's choice is one of them
        classes = len({(int(a), int(b)) for a, b in zip(tv[tied], av[tied])})
        together += classes > 1
        most = max(most, classes)
        cnt[w] += 1
    assert together >= 100 and most >= 3  # (600 pods; up to six classes at once)
    from ksim import ingest, scheduler
    nodes5, pods5 = sixteen_class_workload(203, 5)
    cl5 = ingest.Cluster.from_objects(nodes5, (), pods5)
    pl5 = scheduler.plan(cl5, *scheduler.provider("DefaultProvider"))
    assert (_reduce_classes(cl5, pl5) == 20).all()
