"""GPU parity of the scenario sweep over SelectorSpread queues (the SPR instantiations of
ksim_sweep_general_kernel): every scenario — the snapshot without its absent nodes and the running
pods bound to them, the listers unchanged — must equal, bit for bit, the reference's run on the
reduced objects (tests/spread_sweep_inputs.py; the inputs' properties are pinned on the CPU in
tests/test_sweep_spread_host.py).  Before the SPR instantiations every case here ended in
KsimUnsupported: "a pod in the range carries inter-pod affinity or spread state"."""
import copy

import numpy as np
import pytest

import ksim_ref as R
import spread_sweep_inputs as X
from ksim import abi, ingest, scheduler, spread

pytestmark = pytest.mark.gpu


def _sched(cl, policy="default", **kw):
    preds, prios = X.POLICIES[policy]
    return scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False, **kw)


def _check(sets_, refs, out, ctr, g):
    for k, ((label, _), r) in enumerate(zip(sets_, refs)):
        assert np.array_equal(out[k], r["out"]), label
        assert int(ctr[k]) == r["counter"], label
        assert int(g.last_scheduled[k]) == int((r["out"] >= 0).sum()), label


def _check_records(sets_, refs, f, cap):
    for k, ((label, _), r) in enumerate(zip(sets_, refs)):
        assert int(f["count"][k]) == r["count"] and int(f["listed"][k]) == r["listed"], label
        kept = min(r["count"], cap)
        assert np.array_equal(f["pod"][k, :kept], r["pod"][:kept]), label
        assert np.array_equal(f["hist"][k, :kept], r["hist"][:kept]), label
        assert (f["pod"][k, kept:] == -1).all() and (f["hist"][k, kept:] == -1).all(), label


# ---- 1. the random workloads: placements, counter, pods bound
@pytest.mark.parametrize("policy", sorted(X.POLICIES))
@pytest.mark.parametrize("zones", [True, False], ids=["zones", "no-zones"])
@pytest.mark.parametrize("n_nodes", [n for n, _ in X.RND_SIZES])
def test_random_workloads_match_the_reference(n_nodes, zones, policy):
    inp, sets_, refs = X.rnd_refs(n_nodes, zones, policy)
    cl = inp.cluster()
    assert cl.spread_active
    g = _sched(cl, policy)
    out, ctr, st = g.sweep(None, 0, len(inp.queue), absent=[a for _, a in sets_])
    assert st.mode == abi.MODE_PERSISTENT and st.kernel_launches == 1 and st.blocks == len(sets_)
    assert st.pods == len(sets_) * len(inp.queue) and st.node_evals == st.pods * n_nodes
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 2. segment geometry
@pytest.mark.parametrize("n", [1025, 2049])
def test_ragged_segments_under_wide_ties(n):
    inp, sets_, refs = X.uniform_refs(n)
    g = _sched(inp.cluster())
    out, ctr, _ = g.sweep(None, 0, len(inp.queue), absent=[a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 3. several reduce classes together with spread
def test_several_reduce_classes_with_spread():
    inp, sets_, refs = X.classes_refs()
    g = _sched(inp.cluster())
    out, ctr, _ = g.sweep(None, 0, len(inp.queue), absent=[a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 4. fit nodes only; 5. first pod of a service, a pod no selector matches
@pytest.mark.parametrize("which", ["overflow", "first-pod"])
def test_fit_nodes_only_and_first_pods(which):
    inp = X.overflow_input() if which == "overflow" else X.first_pod_input()
    sets_ = X.sets_of(inp.cluster())
    refs = [X.oracle_ref(inp, "default", a) for _, a in sets_]
    g = _sched(inp.cluster())
    out, ctr, _ = g.sweep(None, 0, len(inp.queue), absent=[a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 6. a sweep from mid-queue after schedule() of a prefix; the handle stays untouched
def test_sweep_after_a_scheduled_prefix_and_untouched_handle():
    inp, sets_, refs = X.rnd_refs(70, True, "default")
    cl = inp.cluster()
    Q, K = len(inp.queue), 35
    g = _sched(cl)
    fresh = _sched(cl)
    # untouched: a whole sweep first, then the handle schedules as a fresh one does
    before = g.node_state()
    out, ctr, _ = g.sweep(None, 0, Q, absent=[a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    head, _, _ = g.schedule(0, K)
    want, _, _ = fresh.schedule(0, K)
    none = refs[[label for label, _ in sets_].index("none")]
    assert np.array_equal(head, want) and np.array_equal(head, none["out"][:K])  # the sweep wrote no count of the handle
    lni = g.last_node_index
    assert lni == fresh.last_node_index
    # from mid-queue: the scenarios carry the prefix's commits (counts included) unless their node is absent
    bound = [(pod, int(w)) for pod, w in zip(inp.queue[:K], head) if w >= 0]
    tail = [X.oracle_ref(inp, "default", a, queue=inp.queue[K:], bound=bound, counter=lni) for _, a in sets_]
    out, ctr, _ = g.sweep(None, K, Q - K, absent=[a for _, a in sets_])
    _check(sets_, tail, out, ctr, g)
    assert np.array_equal(out[0], none["out"][K:]) and int(ctr[0]) == none["counter"]
    rest, _, _ = g.schedule(K, Q - K)
    assert np.array_equal(rest, none["out"][K:]) and g.last_node_index == none["counter"]
    g.close()
    fresh.close()


# ---- 7. chunks
def test_scenario_chunks(monkeypatch):
    inp, sets_, refs = X.rnd_refs(130, True, "spread_heavy")
    g = _sched(inp.cluster(), "spread_heavy")
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "3")
    out, ctr, st = g.sweep(None, 0, len(inp.queue), absent=[a for _, a in sets_])
    assert st.kernel_launches == (len(sets_) + 2) // 3 and st.blocks == 3
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 8. explained records
@pytest.mark.parametrize("cap", [True, 3])
def test_explained_records_equal_the_oracles_histograms(cap):
    inp = X.overflow_input()
    sets_ = X.sets_of(inp.cluster())
    refs = [X.oracle_cpu(inp, "default", a) for _, a in sets_]
    assert min(r["count"] for r in refs) > 3  # the cap falls inside every scenario's failures
    g = _sched(inp.cluster())
    Q = len(inp.queue)
    o0, c0, _ = g.sweep(None, 0, Q, absent=[a for _, a in sets_])
    out, ctr, _ = g.sweep(None, 0, Q, absent=[a for _, a in sets_], explain=cap)
    assert np.array_equal(out, o0) and np.array_equal(ctr, c0)
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, Q if cap is True else cap)
    g.close()


# ---- 9. object level: what_if and drain_what_if
def _zone_outages(cc):
    return [("zone-" + v, idx) for v, idx in scheduler.outage_sets(cc.cluster, X.ZONE)]


def test_cluster_capacity_what_if_with_listers():
    inp = X.overflow_input()
    preds, prios = X.POLICIES["default"]
    sim_pods = list(reversed(inp.queue))  # the simulator pops its list from the end
    cc = scheduler.ClusterCapacity(inp.nodes, inp.running, sim_pods, provider_name="DefaultProvider", collect_reasons=False,
                                   spread=inp.listers())
    outages = _zone_outages(cc)
    assert len(outages) == 3
    failed = 0
    for r, (name, idx) in zip(cc.what_if(outages, explain=True), outages):
        gone = {cc.cluster.names[i] for i in idx}
        left = [x for x in inp.nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in inp.running if x["spec"]["nodeName"] not in gone]
        want, _ = R.simulate(left, stay, sim_pods, set(preds), list(prios), spread=R.SpreadListers(**inp.objs))
        assert r["placements"] == [(pn, host) for pn, host, _ in want], name
        assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
        assert r["listed"] == len(left)
        failed += r["failed"]
    assert failed > 0


def test_cluster_capacity_drain_what_if_with_listers():
    inp = X.overflow_input()
    preds, prios = X.POLICIES["default"]
    running = copy.deepcopy(inp.running)
    for x in running:  # controller-owned: kubectl drain evicts them
        x["metadata"]["ownerReferences"] = [{"kind": "ReplicaSet", "name": "rs", "controller": True}]
    sim_pods = list(reversed(inp.queue))
    cc = scheduler.ClusterCapacity(inp.nodes, running, sim_pods, provider_name="DefaultProvider", collect_reasons=False,
                                   spread=inp.listers())
    outages = _zone_outages(cc)
    rehosted = 0
    for r, (name, idx) in zip(cc.drain_what_if(outages, explain=True), outages):
        gone = {cc.cluster.names[i] for i in idx}
        left = [x for x in inp.nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in running if x["spec"]["nodeName"] not in gone]
        evicted = [x for x in running if x["spec"]["nodeName"] in gone and scheduler.default_evictable(x)]
        m = len(evicted)
        assert r["evicted"] == m and all(x["metadata"]["labels"] == {"app": "a"} for x in evicted)  # service members
        order = [scheduler.requeue_copy(x) for x in evicted] + inp.queue
        want, _ = R.simulate(left, stay, list(reversed(order)), set(preds), list(prios), spread=R.SpreadListers(**inp.objs))
        assert r["requeued"] == [(pn, host) for pn, host, _ in want[:m]], name
        assert r["placements"] == [(pn, host) for pn, host, _ in want[m:]], name
        assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
        rehosted += r["rehosted"]
    assert rehosted > 0


# ---- 10. the caps
def test_node_and_zone_caps():
    """38,400 nodes in KSIM_SWEEP_SPREAD_MAX_ZONES zones: the evaluations, the zone words and the
    reduction words together are the largest LDS request the kernel makes."""
    inp = X.caps_input()
    cl = inp.cluster()
    n = cl.n_nodes
    zone0 = dict(scheduler.outage_sets(cl, X.ZONE))["z0000"]
    sets_ = [("none", []), ("zone-z0000", list(zone0)), ("last-1000", list(range(n - 1000, n)))]
    refs = [X.oracle_cpu(inp, "default", a) for _, a in sets_]
    g = _sched(cl)
    out, ctr, _ = g.sweep(None, 0, len(inp.queue), absent=[a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 11. refusals
def test_one_zone_above_the_cap_is_refused():
    inp = X.caps_input(n=abi.SWEEP_SPREAD_MAX_ZONES + 1, zones=abi.SWEEP_SPREAD_MAX_ZONES + 1, p=6)
    g = _sched(inp.cluster())
    with pytest.raises(abi.KsimUnsupported, match=r"inter-pod affinity or spread state \(%d zones exceed the %d zones"
                       % (abi.SWEEP_SPREAD_MAX_ZONES + 1, abi.SWEEP_SPREAD_MAX_ZONES)):
        g.sweep(None, 0, 6, absent=[[0]])
    assert len(g.schedule(0, 6)[0]) == 6  # the handle stays usable
    g.close()


def test_spread_weight_counts_toward_the_score_bits():
    inp = X.rnd_input(18, True)
    lim = (1 << 27) // 10
    preds = ["GeneralPredicates"]
    g = scheduler.GenericScheduler(inp.cluster(), preds, [("SelectorSpreadPriority", lim - 1), ("LeastRequestedPriority", 1)],
                                   collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="map scores exceed 27 bits"):
        g.sweep(None, 0, 10, absent=[[0]])
    g.close()
    g = scheduler.GenericScheduler(inp.cluster(), preds, [("SelectorSpreadPriority", lim - 2), ("LeastRequestedPriority", 1)],
                                   collect_reasons=False)
    out, _, _ = g.sweep(None, 0, 10, absent=[[0]])
    want, _, _ = g.schedule(0, 10)
    assert out.shape == (1, 10) and (out[0] != 0).all() and (want >= 0).all()
    g.close()


def test_scenario_weights_over_a_spread_range_are_refused():
    """A policy without reduce priorities, so that the spread weight alone is what the scenario would drop."""
    inp = X.for_policy(X.rnd_input(18, True), "service_spreading")
    g = _sched(inp.cluster(), "service_spreading")
    with pytest.raises(abi.KsimUnsupported, match="scenario weights over a SelectorSpread queue would drop"):
        g.sweep([[("LeastRequestedPriority", 1)]], 0, 10)
    with pytest.raises(abi.KsimUnsupported, match="scenario weights over a SelectorSpread queue would drop"):
        g.sweep([[("LeastRequestedPriority", 1)]], 0, 10, absent=[[0]])
    out, _, _ = g.sweep(None, 0, 10, absent=[[0]])  # the handle stays usable
    assert out.shape == (1, 10)
    g.close()


def test_an_inter_pod_affinity_pod_among_spread_pods_is_refused():
    inp = X.rnd_input(18, True)
    queue = copy.deepcopy(inp.queue[:12])
    queue[5]["spec"]["affinity"] = {"podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [
        {"labelSelector": {"matchLabels": {"app": "a"}}, "topologyKey": "kubernetes.io/hostname"}]}}
    cl = ingest.Cluster.from_objects(inp.nodes, inp.running, queue, spread=inp.listers())
    g = _sched(cl)
    with pytest.raises(abi.KsimUnsupported, match="inter-pod affinity or spread state"):
        g.sweep(None, 0, 12, absent=[[0]])
    with pytest.raises(abi.KsimUnsupported, match="re-queued pod 5 carries inter-pod affinity"):
        g.sweep_drain([[0]], [[5]], 0, 0)
    g.close()


def test_auxiliary_tables_are_refused():
    inp = X.rnd_input(18, True)
    preds = ["GeneralPredicates"]
    prios = [("SelectorSpreadPriority", 1), ("ServiceSpreadingPriority", 1), ("LeastRequestedPriority", 1)]
    cc = scheduler.ClusterCapacity(inp.nodes, inp.running, list(reversed(inp.queue)), predicates=preds, priorities=prios,
                                   collect_reasons=False, spread=inp.listers())
    with pytest.raises(abi.KsimUnsupported, match=r"ksim_sweep_nodes: a pod in the range carries inter-pod affinity or spread "
                       r"state \(auxiliary spreading priority or lender tables are loaded\)"):
        cc.what_if([("first", [0])])
    with pytest.raises(abi.KsimUnsupported, match=r"ksim_sweep_drain: a pod in the range carries inter-pod affinity or spread "
                       r"state \(auxiliary"):
        cc.drain_what_if([("first", [0])])
