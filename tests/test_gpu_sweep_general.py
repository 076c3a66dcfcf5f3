"""GPU parity of the scenario sweep's general form (ksim_sweep_general_kernel): queues with host
ports, node selectors, tolerations, nodeName, gpu / extended requests and several reduce classes,
swept with a node set per scenario.  Scenario s with absent set A_s must equal the CPU oracle run
on the snapshot from which the nodes of A_s were left out — placements (as indices of the loaded
table), final lastNodeIndex and pods bound."""
import copy
import functools

import numpy as np
import pytest

import cpu_ref
from ksim import abi, ingest, scheduler, synth

pytestmark = pytest.mark.gpu

PREDS = list(scheduler.DEFAULT_PREDICATES)
MAP_POLICIES = [[("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)],
                [("MostRequestedPriority", 2), ("BalancedResourceAllocation", 1)]]


def _reduced(cl, keep):
    """The cluster without the nodes outside `keep`; a queued pod's nodeName index becomes the rank
    in the reduced table, or -2 ("no such node", the value ingest uses) for a node left out."""
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


def _oracle(cl, g, cfg, absent, first, count, state=None, counter=0):
    """cpu_ref under the scheduler's own class tables and addends on the reduced cluster, its node
    indices mapped back to the loaded table.  Without any node left the reference returns
    ErrNoNodesAvailable for every pod: nothing bound, counter unchanged."""
    n = cl.n_nodes
    keep = np.ones(n, bool)
    keep[list(absent)] = False
    if not keep.any():
        return np.full(count, -1, np.int32), counter
    sub = _reduced(cl, keep)
    if state is not None:
        state = {k: np.ascontiguousarray(v[..., keep]) for k, v in state.items()}
    ref, _, _, ctr = cpu_ref.run(sub, cfg, first, count, threads=8, state=state, counter=counter, tables=g.tables,
                                 na_add=g.na_add)
    back = np.nonzero(keep)[0].astype(np.int32)
    return np.where(ref >= 0, back[np.maximum(ref, 0)], -1).astype(np.int32), ctr


def _node_sets(n, first_ten):
    """(label, absent set) of the what-ifs, as tests/test_gpu_sweep_nodes.py runs them."""
    rng = np.random.default_rng(20240611)
    sets_ = [("none", []), ("first", [0]), ("last", [n - 1]), ("word-edge", [31, 32])]
    if n > 1024:
        sets_.append(("1023-1024", [1023, 1024]))
    sets_.append(("random-10pct", sorted(int(x) for x in rng.choice(n, n // 10, replace=False))))
    sets_.append(("first-ten-pods", sorted(set(int(x) for x in first_ten if x >= 0))))
    sets_.append(("all-but-7", [i for i in range(n) if i != 7]))
    sets_.append(("every-node", list(range(n))))
    return sets_


def _check(sets_, refs, out, ctr, bound):
    for k, ((label, a), (ref, ref_ctr)) in enumerate(zip(sets_, refs)):
        assert np.array_equal(out[k], ref), label
        assert int(ctr[k]) == ref_ctr, label
        assert not np.isin(out[k][out[k] >= 0], a).any(), label  # no absent node is ever chosen
        assert int(bound[k]) == int((ref >= 0).sum()), label


@functools.lru_cache(maxsize=None)
def _c2_cluster(n, p, seed):
    nodes, pods = synth.c2_objects(n, p, seed=seed)
    return ingest.Cluster.from_objects(nodes, (), pods)


@functools.lru_cache(maxsize=None)
def _input1():
    """c2_objects(1500, 1200, seed=2) under DefaultProvider: host-port pods, selectors, tolerations,
    two TaintToleration classes; n = 1500 gives two-row select segments and a ragged last mask
    word.  The absent sets and the oracle's answers, once."""
    cl = _c2_cluster(1500, 1200, 2)
    preds, prios = scheduler.provider("DefaultProvider")
    tabs = scheduler.plan(cl, preds, prios)  # the class tables and addends a scheduler loads
    cfg = scheduler.make_config(preds, prios)
    plain, _ = _oracle(cl, tabs, cfg, [], 0, len(cl.pods))
    sets_ = _node_sets(cl.n_nodes, plain[:10])
    refs = [_oracle(cl, tabs, cfg, a, 0, len(cl.pods)) for _, a in sets_]
    return cl, sets_, refs


def test_c2_queue_matches_oracle_on_the_reduced_cluster():
    cl, sets_, refs = _input1()
    assert int((cl.pods["port_cnt"] > 0).sum()) > 100  # the queue is not resource-only
    n, p = cl.n_nodes, len(cl.pods)
    preds, prios = scheduler.provider("DefaultProvider")
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    before = g.node_state()
    out, ctr, st = g.sweep(None, 0, p, absent=[a for _, a in sets_])
    assert st.mode == abi.MODE_PERSISTENT
    assert st.kernel_launches == 1 and st.blocks == len(sets_)
    assert st.node_evals == len(sets_) * p * n
    _check(sets_, refs, out, ctr, g.last_scheduled)
    for k, (label, a) in enumerate(sets_):
        if label not in ("none", "every-node"):  # every node set changes the outcome
            assert not np.array_equal(out[k], refs[0][0]), label
        if label == "every-node":
            assert (out[k] == -1).all() and int(ctr[k]) == 0 and int(g.last_scheduled[k]) == 0
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    g.close()


def test_c2_queue_runs_in_scenario_chunks(monkeypatch):
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "5")
    cl, sets_, refs = _input1()
    preds, prios = scheduler.provider("DefaultProvider")
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    out, ctr, st = g.sweep(None, 0, len(cl.pods), absent=[a for _, a in sets_])
    assert st.mode == abi.MODE_PERSISTENT
    assert st.kernel_launches == (len(sets_) + 4) // 5 and st.blocks == 5
    _check(sets_, refs, out, ctr, g.last_scheduled)
    g.close()


def test_overflowing_queue_swept_from_mid_queue():
    """c2_objects(64, 3000, seed=7) overflows the cluster (and single-fit pods keep the counter below
    the bound count).  Swept from pod 500 after a regular schedule() of the prefix: absent nodes take
    their prefix pods with them."""
    cl = _c2_cluster(64, 3000, 7)
    n, p = cl.n_nodes, len(cl.pods)
    preds, prios = scheduler.provider("DefaultProvider")
    cfg = scheduler.make_config(preds, prios)
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    pre, _, state0, ctr0 = cpu_ref.run(cl, cfg, 0, 500, threads=4, tables=g.tables, na_add=g.na_add)
    sets_ = _node_sets(n, pre[:10])
    held = dict(sets_)["first-ten-pods"]
    assert len(held) > 0 and (np.bincount(pre[pre >= 0], minlength=n)[held] > 0).all()
    got_pre, _, _ = g.schedule(0, 500)
    assert np.array_equal(got_pre, pre)
    out, ctr, st = g.sweep(None, 500, p - 500, absent=[a for _, a in sets_])
    assert st.mode == abi.MODE_PERSISTENT
    refs = [_oracle(cl, g, cfg, a, 500, p - 500, state={k: v.copy() for k, v in state0.items()}, counter=ctr0)
            for _, a in sets_]
    _check(sets_, refs, out, ctr, g.last_scheduled)
    assert (out < 0).any(axis=1).all()  # the cluster fills up in every scenario
    assert g.last_node_index == ctr0
    st1 = g.node_state()
    for key in state0:
        assert np.array_equal(st1[key], state0[key]), key
    g.close()


def test_nodename_extended_requests_and_twelve_reduce_classes():
    """rnd_workload(5, 200 nodes, 600 pods, 40 running): nodeName pods, extended and gpu requests,
    up to 12 reduce classes (3 TaintToleration x 4 NodeAffinity), running pods; one scenario leaves
    out the node a nodeName pod names."""
    from workloads import rnd_workload
    nodes, running, pods = rnd_workload(5, n_nodes=200, n_pods=600, n_running=40)
    cl = ingest.Cluster.from_objects(nodes, running, pods)
    n, p = cl.n_nodes, len(cl.pods)
    named = sorted(set(int(x) for x in cl.pods["host"] if x >= 0))
    assert named and int((cl.pods["scalar_cnt"] > 0).sum()) > 0 and int((cl.pods["req_gpu"] > 0).sum()) > 0
    preds, prios = scheduler.provider("DefaultProvider")
    cfg = scheduler.make_config(preds, prios)
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    k_max = int((np.asarray(g.tables["n_tt"]) * np.asarray(g.tables["n_na"]))[cl.pods["cls"]].max())
    assert 1 < k_max <= abi.MAX_RCLASS
    plain, _ = _oracle(cl, g, cfg, [], 0, p)
    # a nodeName pod the full cluster places, and its node
    kept = [int(k) for k in np.nonzero(cl.pods["host"] >= 0)[0] if plain[k] >= 0]
    assert kept and int(plain[kept[0]]) == int(cl.pods["host"][kept[0]])
    its_node = int(cl.pods["host"][kept[0]])
    sets_ = [("none", []), ("first", [0]), ("last", [n - 1]), ("word-edge", [31, 32]), ("nodename", [its_node]),
             ("every-nodename", named), ("first-ten-pods", sorted(set(int(x) for x in plain[:10] if x >= 0))),
             ("every-second", list(range(0, n, 2)))]
    before = g.node_state()
    out, ctr, st = g.sweep(None, 0, p, absent=[a for _, a in sets_])
    assert st.mode == abi.MODE_PERSISTENT
    refs = [_oracle(cl, g, cfg, a, 0, p) for _, a in sets_]
    _check(sets_, refs, out, ctr, g.last_scheduled)
    k = [label for label, _ in sets_].index("nodename")
    assert out[0][kept[0]] == its_node and out[k][kept[0]] == -1  # its nodeName names a node the scenario does not list
    assert not np.array_equal(out[k], out[0])
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    g.close()


def test_explicit_map_weights_per_scenario():
    """A scheduler configured with map priorities only: two scenarios with different weights over
    the c2 queue, each against the oracle under its own config."""
    cl = _c2_cluster(1500, 1200, 2)
    p = len(cl.pods)
    g = scheduler.GenericScheduler(cl, PREDS, MAP_POLICIES[0], collect_reasons=False)
    sets_ = [("word-edge", [31, 32]), ("last", [cl.n_nodes - 1])]
    out, ctr, st = g.sweep(MAP_POLICIES, 0, p, absent=[a for _, a in sets_])
    assert st.mode == abi.MODE_PERSISTENT
    refs = [_oracle(cl, g, scheduler.make_config(PREDS, pri), a, 0, p) for (_, a), pri in zip(sets_, MAP_POLICIES)]
    _check(sets_, refs, out, ctr, g.last_scheduled)
    # without node sets (ksim_sweep): the same weights, every node listed
    o2, c2, st2 = g.sweep(MAP_POLICIES, 0, p)
    assert st2.mode == abi.MODE_PERSISTENT
    for k, pri in enumerate(MAP_POLICIES):
        ref, ref_ctr = _oracle(cl, g, scheduler.make_config(PREDS, pri), [], 0, p)
        assert np.array_equal(o2[k], ref) and int(c2[k]) == ref_ctr
    assert not np.array_equal(o2[0], o2[1])
    g.close()


def test_cluster_capacity_what_if_on_objects_with_selectors_taints_and_ports():
    """ClusterCapacity.what_if under DefaultProvider on c2 objects against ksim_ref.simulate on the
    object lists with the outage's node removed."""
    import ksim_ref as R
    nodes, pods = synth.c2_objects(48, 150)
    preds, prios = scheduler.provider("DefaultProvider")
    cc = scheduler.ClusterCapacity(nodes, [], pods, provider_name="DefaultProvider", collect_reasons=False)
    outages = scheduler.outage_sets(cc.cluster, "node")[:4]
    recs = cc.what_if(outages)
    assert [r["name"] for r in recs] == [nm for nm, _ in outages]
    for r, (name, idx) in zip(recs, outages):
        assert idx == [cc.cluster.index[name]] and r["absent"] == 1
        left = [x for x in nodes if x["metadata"]["name"] != name]
        want, _ = R.simulate(left, [], pods, set(preds), prios)
        assert r["placements"] == [(pn, host) for pn, host, _ in want], name
        assert r["scheduled"] == sum(1 for _, host, _ in want if host is not None)
        assert all(host != name for _, host in r["placements"])


def test_affinity_and_volume_queues_are_refused():
    from workloads import rnd_affinity_workload, rnd_volume_workload
    preds, prios = scheduler.provider("DefaultProvider")
    nodes, running, pods = rnd_affinity_workload(1, n_nodes=20, n_pods=40)
    cl = ingest.Cluster.from_objects(nodes, running, pods)
    assert int((cl.pods["aff_class"] > 0).sum()) > 0
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="affinity"):
        g.sweep(None, 0, len(cl.pods), absent=[[0], []])
    g.close()
    nodes, running, pods, pvs, pvcs = rnd_volume_workload(0, resolvable_only=True)
    cl =ingest.Cluster.from_objects(nodes, running, pods, pvs=pvs, pvcs=pvcs)
    assert int((cl.pods["vol_class"] > 0).sum()) > 0
    vol_preds = ["GeneralPredicates", "NoDiskConflict", "MaxEBSVolumeCount", "MaxGCEPDVolumeCount"]
    g = scheduler.GenericScheduler(cl, vol_preds, MAP_POLICIES[0], collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="volumes"):
        g.sweep(None, 0, len(cl.pods), absent=[[0], []])
    g.close()


def test_explicit_weights_under_a_reduce_policy_are_refused():
    """Scenario weights over a general queue on a DefaultProvider scheduler would drop its
    TaintToleration / NodeAffinity / NodePreferAvoidPods part: refused; scenarios=None sweeps it."""
    cl = _c2_cluster(64, 3000, 7)
    preds, prios = scheduler.provider("DefaultProvider")
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="weights = NULL"):
        g.sweep([MAP_POLICIES[0]], 0, 100, absent=[[0]])
    with pytest.raises(abi.KsimUnsupported):
        g.sweep([MAP_POLICIES[0]], 0, 100)
    g.close()


def test_resource_only_queues_keep_their_forms(monkeypatch):
    n, p = 300, 200
    cpu, mem = synth.c3_nodes(n, 11)
    pcpu, pmem = synth.c3_pods(p, 11)
    cl = synth.resource_cluster(["s-%05d" % i for i in range(n)], cpu, mem, np.full(n, 30, np.int32), pcpu, pmem)
    g = scheduler.GenericScheduler(cl, PREDS, MAP_POLICIES[0], collect_reasons=False)
    _, _, st = g.sweep(MAP_POLICIES, 0, p, absent=[[0], [1]])
    assert st.mode == abi.MODE_TREE
    monkeypatch.setenv("KSIM_SWEEP_SCAN", "1")
    _, _, st = g.sweep(MAP_POLICIES, 0, p, absent=[[0], [1]])
    assert st.mode == abi.MODE_PERSISTENT
    g.close()
