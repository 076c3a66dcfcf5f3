"""GPU parity of the scenario sweep over inter-pod affinity queues (ksim_sweep_affinity, the IPA
instantiations of ksim_sweep_general_kernel): every scenario — the snapshot without its absent nodes
and the running pods bound to them — must equal, bit for bit, the reference's run on the reduced
objects (tests/affinity_sweep_inputs.py; the inputs' properties are pinned on the CPU in
tests/test_sweep_affinity_host.py).  Every comparison is against the oracles, never against another
GPU form.  Without the entry every case here fails (no ksim_sweep_affinity); without the correction
of the scenarios' counts the outage cases fail."""
import copy
import ctypes as C

import numpy as np
import pytest

import affinity_sweep_inputs as A
import ksim_ref as R
import spread_sweep_inputs as X
from ksim import abi, ingest, scheduler

pytestmark = pytest.mark.gpu


def _sched(cl, policy=A.DEFAULT, **kw):
    return scheduler.GenericScheduler(cl, policy[0], policy[1], collect_reasons=False, **kw)


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


# ---- 1. the hand cases and an outage of nothing: placements, counters, FitError histograms
@pytest.mark.parametrize("case", sorted(A.HAND))
def test_hand_cases(case):
    inp = A.hand_input(case)
    cl = inp.cluster()
    sets_ = A.hand_sets(case)
    refs = [A.oracle_cpu(inp, a) for _, a in sets_]
    texts = [A.oracle_ref(inp, a) for _, a in sets_]
    want = A.HAND[case][3]
    assert refs[1]["out"][0] == (cl.index[want] if want else -1)
    g = _sched(cl)
    out, ctr, st = g.sweep_affinity([a for _, a in sets_], explain=True)
    assert st.mode == abi.MODE_PERSISTENT and st.kernel_launches == 1 and st.blocks == 2
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, 1)
    f = g.last_failures
    for k, t in enumerate(texts):
        got = [(inp.queue[int(f["pod"][k, j])]["metadata"]["name"],
                scheduler.fit_error_message(int(f["listed"][k]), f["hist"][k, j], cl.scalar_names.items))
               for j in range(int(f["count"][k]))]
        assert got == t["msgs"], sets_[k][0]
    g.close()


# ---- 2. the random workloads under DefaultProvider, records with and without a cap
@pytest.mark.parametrize("cap", [None, True, 2])
@pytest.mark.parametrize("n_nodes", [n for n, _, _ in A.RND_SIZES])
def test_random_workloads_match_the_reference(n_nodes, cap):
    inp, sets_, refs = A.rnd_refs(n_nodes)
    cl = inp.cluster()
    Q = len(inp.queue)
    g = _sched(cl)
    assert g.has_affinity_terms()
    out, ctr, st = g.sweep_affinity([a for _, a in sets_], None, 0, Q, explain=cap)
    assert st.mode == abi.MODE_PERSISTENT and st.kernel_launches == 1 and st.blocks == len(sets_)
    assert st.pods == len(sets_) * Q and st.node_evals == st.pods * n_nodes
    _check(sets_, refs, out, ctr, g)
    if cap is not None:
        assert min(r["count"] for r in refs) >= 2
        _check_records(sets_, refs, g.last_failures, Q if cap is True else cap)
    g.close()


# ---- 3. two rows per thread
def test_more_than_1024_nodes():
    inp, sets_, refs = A.wide_refs()
    assert inp.cluster().n_nodes == 1100 and len(sets_) == 4
    g = _sched(inp.cluster())
    out, ctr, _ = g.sweep_affinity([a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 4. the node cap
def test_node_cap():
    inp = A.caps_input()
    cl = inp.cluster()
    n = cl.n_nodes
    assert n == abi.SWEEP_GENERAL_MAX_NODES
    zone0 = dict(scheduler.outage_sets(cl, A.ZONE))["z000"]
    sets_ = [("none", []), ("zone-z000", list(zone0)), ("last-1000", list(range(n - 1000, n)))]
    refs = [A.oracle_cpu(inp, a) for _, a in sets_]
    assert A.lost_affinity_pods(inp, zone0) + A.lost_affinity_pods(inp, sets_[2][1]) > 0
    g = _sched(cl)
    out, ctr, _ = g.sweep_affinity([a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 5. prefix queues: the evictable running pods of the outage's nodes first
@pytest.mark.parametrize("which", ["hand", "rnd-70"])
def test_prefix_queues(which):
    inp = A.hand_input("own-anti-affinity") if which == "hand" else A.rnd_input(70)
    sets_ = A.hand_sets("own-anti-affinity") if which == "hand" else A.sets_of(inp.cluster())
    copies, requeue, queues = A.drain_plan(inp, sets_)
    assert sum(len(r) for r in requeue) > 0
    dcl = inp.cluster(extra=copies)
    Q = len(inp.queue)
    for count in (Q, 0):
        refs = [A.oracle_cpu(inp, a, queue=q + inp.queue[:count]) if q or count else None
                for (_, a), q in zip(sets_, queues)]
        g = _sched(dcl)
        out, pre, ctr, st = g.sweep_affinity([a for _, a in sets_], requeue, 0, count, explain=True)
        for k, ((label, _), r, rq) in enumerate(zip(sets_, refs, requeue)):
            m = len(rq)
            if r is None:  # neither prefix nor range: nothing is scheduled
                assert len(pre[k]) == 0 and out.shape[1] == 0 and int(ctr[k]) == 0, label
                continue
            assert np.array_equal(pre[k], r["out"][:m]) and np.array_equal(out[k], r["out"][m:]), label
            assert int(ctr[k]) == r["counter"], label
            assert int(g.last_rehosted[k]) == int((r["out"][:m] >= 0).sum()), label
            assert int(g.last_scheduled[k]) == int((r["out"][m:] >= 0).sum()), label
            f = g.last_failures
            assert int(f["count"][k]) == r["count"] and int(f["listed"][k]) == r["listed"], label
            assert np.array_equal(f["pod"][k, :r["count"]], r["pod"]), label
            assert np.array_equal(f["hist"][k, :r["count"]], r["hist"]), label
        assert st.pods == sum(len(r) for r in requeue) + len(sets_) * count
        g.close()


# ---- 6. affinity and SelectorSpread together: step 1b adds both terms
def test_affinity_with_selector_spread():
    inp = A.spread_input()
    cl = inp.cluster()
    assert cl.spread_active
    sets_ = A.sets_of(cl, X.ZONE)
    refs = [A.oracle_cpu(inp, a) for _, a in sets_]
    g = _sched(cl)
    assert g.has_affinity_terms()
    out, ctr, _ = g.sweep_affinity([a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 7. several reduce classes together with affinity
def test_several_reduce_classes_with_affinity():
    inp = A.classes_input()
    cl = inp.cluster()
    assert X.max_reduce_classes(cl) > 1
    sets_ = [s for s in A.sets_of(cl) if s[0] in ("none", "first", "zone-z2")]
    refs = [A.oracle_cpu(inp, a) for _, a in sets_]
    g = _sched(cl)
    out, ctr, _ = g.sweep_affinity([a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 8. bound=: the placements of a scheduled prefix as residents
def test_bound_pods_of_a_scheduled_prefix():
    inp, sets_, _ = A.rnd_refs(70)
    cl = inp.cluster()
    K, Q = 10, len(inp.queue)
    g = _sched(cl)
    head, _, _ = g.schedule(0, K)
    lni = g.last_node_index
    bound = [(q, int(w)) for q, w in enumerate(head) if w >= 0]
    assert bound
    objs = [(inp.queue[q], w) for q, w in bound]
    tail = [A.oracle_ref(inp, a, queue=inp.queue[K:], bound=objs, counter=lni) for _, a in sets_]
    out, ctr, _ = g.sweep_affinity([a for _, a in sets_], None, K, Q - K, bound=bound)
    _check(sets_, tail, out, ctr, g)
    g.close()


# ---- 9. a pod with neither identity nor class, in a queue whose tables hold affinity terms
def test_pods_without_affinity_state():
    inp = A.rnd_input(18)
    lone = [A._pod("lone-%d" % k, "x", cpu="100m") for k in range(3)]
    for x in lone:
        x["metadata"]["labels"] = {}
        x["metadata"]["namespace"] = "elsewhere"
    mixed = A.Input(inp.nodes, inp.running, lone[:1] + inp.queue[:20] + lone[1:])
    cl = mixed.cluster()
    pods = np.asarray(cl.pods)
    idx = [0, 21, 22]
    assert (pods["aff_ident"][idx] == 0).all() and (pods["aff_class"][idx] == 0).all()
    sets_ = A.sets_of(cl)
    refs = [A.oracle_cpu(mixed, a) for _, a in sets_]
    g = _sched(cl)
    out, ctr, _ = g.sweep_affinity([a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 10. refusals, by message
def test_refusals():
    plain = X.rnd_input(18, True)
    g = scheduler.GenericScheduler(ingest.Cluster.from_objects(plain.nodes, [], plain.queue[:6]), *A.DEFAULT,
                                   collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: no affinity tables are loaded"):
        g.sweep_affinity([[0]])
    g.close()
    # auxiliary tables
    prios = [("SelectorSpreadPriority", 1), ("ServiceSpreadingPriority", 1), ("LeastRequestedPriority", 1)]
    cc = scheduler.ClusterCapacity(plain.nodes, plain.running, list(reversed(plain.queue)), predicates=["GeneralPredicates"],
                                   priorities=prios, collect_reasons=False, spread=plain.listers())
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: an auxiliary spreading priority or "
                       "CheckServiceAffinity's lender table is loaded"):
        cc.scheduler.sweep_affinity([[0]])
    # the packed score
    inp = A.rnd_input(18)
    lim = (1 << 27) // 10
    g = scheduler.GenericScheduler(inp.cluster(), ["GeneralPredicates", "MatchInterPodAffinity"],
                                   [("InterPodAffinityPriority", lim - 1), ("LeastRequestedPriority", 1)], collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="map, spread and inter-pod scores exceed 27 bits"):
        g.sweep_affinity([[0]])
    g.close()
    # the existing entries keep refusing these tables, with their messages
    g = _sched(inp.cluster())
    with pytest.raises(abi.KsimUnsupported, match=r"ksim_sweep_nodes: a pod in the range carries inter-pod affinity or spread "
                       r"state \(the tables hold inter-pod affinity terms"):
        g.sweep(None, 0, 10, absent=[[0]])
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_drain: re-queued pod"):
        g.sweep_drain([[0]], [[int(np.nonzero(np.asarray(inp.cluster().pods)["aff_class"] > 0)[0][0])]], 0, 0)
    g.close()


def _with_host_anti(pods, k):
    """The pods, pod k labelled app=a and repelling app=a per hostname: the cluster gets affinity tables."""
    pods = copy.deepcopy(list(pods))
    pods[k]["metadata"].setdefault("labels", {})["app"] = "a"
    pods[k]["spec"]["affinity"] = dict(pods[k]["spec"].get("affinity") or {}, **A.HOST_ANTI)  # node affinity kept
    return pods


def test_lender_tables_are_refused():
    from test_oracle_c_features import SVC_PREDS, SVC_PRIOS
    from ksim import spread
    from workloads import rnd_svc_affinity_workload
    nodes, running, pods, services = rnd_svc_affinity_workload(0, n_pods=80, full_labels=True)
    cl = ingest.Cluster.from_objects(nodes, running, list(reversed(pods)), spread=spread.SpreadListers(services=services),
                                     service_affinity=["region", "rack"])
    assert cl.svc_active
    g = scheduler.GenericScheduler(cl, SVC_PREDS, SVC_PRIOS, collect_reasons=False, service_affinity=["region", "rack"])
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: an auxiliary spreading priority or "
                       "CheckServiceAffinity's lender table is loaded"):
        g.sweep_affinity([[0]], None, 0, 10)
    g.close()


def test_volume_pods_are_refused_in_the_range_and_in_a_prefix():
    from workloads import rnd_volume_workload
    nodes, running, pods, pvs, pvcs = rnd_volume_workload(0, resolvable_only=True)
    plain = next(k for k, p in enumerate(pods) if not p["spec"].get("volumes"))
    cl = ingest.Cluster.from_objects(nodes, running, _with_host_anti(pods, plain), pvs=pvs, pvcs=pvcs)
    k = int(np.nonzero(cl.pods["vol_class"] > 0)[0][0])
    preds = ["GeneralPredicates", "NoDiskConflict", "MaxEBSVolumeCount", "MaxGCEPDVolumeCount", "MatchInterPodAffinity"]
    g = scheduler.GenericScheduler(cl, preds, [("LeastRequestedPriority", 1)], collect_reasons=False)
    assert g.affinity is not None and g.volumes is not None
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: pod %d mounts volumes" % k):
        g.sweep_affinity([[0]], None, k, 1)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: re-queued pod %d mounts volumes" % k):
        g.sweep_affinity([[0]], [[k]], plain, 1)
    assert len(g.schedule(0, 5)[0]) == 5  # the handle stays usable
    g.close()


def test_more_than_sixteen_reduce_classes_are_refused():
    from workloads import sixteen_class_workload
    nodes, pods = sixteen_class_workload(203, 5)
    cl = ingest.Cluster.from_objects(nodes, (), _with_host_anti(pods, 0))
    g = _sched(cl)
    assert ((np.asarray(g.tables["n_tt"]) * np.asarray(g.tables["n_na"]))[cl.pods["cls"]] > abi.MAX_RCLASS).all()
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: a pod class in the range has more than %d reduce "
                       "classes" % abi.MAX_RCLASS):
        g.sweep_affinity([[0]], None, 0, 4)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: the class of re-queued pod 3 has more than"):
        g.sweep_affinity([[0]], [[3]], 0, 0)
    g.close()


def test_one_zone_above_the_cap_is_refused_with_a_spread_pair():
    ci = X.caps_input(n=abi.SWEEP_SPREAD_MAX_ZONES + 1, zones=abi.SWEEP_SPREAD_MAX_ZONES + 1, p=6)
    cl = ingest.Cluster.from_objects(ci.nodes, ci.running, _with_host_anti(ci.queue, 2), spread=ci.listers())
    assert (cl.affinity["spread_pair"] >= 0).any() and cl.affinity["n_terms"] > 0
    g = _sched(cl)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: %d zones exceed the %d zones of a swept SelectorSpread "
                       "queue" % (abi.SWEEP_SPREAD_MAX_ZONES + 1, abi.SWEEP_SPREAD_MAX_ZONES)):
        g.sweep_affinity([[0]])
    assert len(g.schedule(0, 6)[0]) == 6
    g.close()


def test_more_zones_than_the_cap_are_swept_without_a_spread_pair():
    """No class has a spread pair: the zone words stay unused, the zone-keyed terms read the counts."""
    inp = A.many_zones_input()
    cl = inp.cluster()
    t = cl.affinity
    assert t["n_dom"][t["zone_key"]] > abi.SWEEP_SPREAD_MAX_ZONES and not (t["spread_pair"] >= 0).any()
    zone0 = dict(scheduler.outage_sets(cl, X.ZONE))["z0000"]
    sets_ = [("none", []), ("first", [0]), ("zone-z0000", list(zone0)), ("every-third", list(range(0, cl.n_nodes, 3)))]
    assert A.lost_affinity_pods(inp, sets_[3][1]) > 5
    refs = [A.oracle_cpu(inp, a) for _, a in sets_]
    assert (refs[0]["out"] != A.oracle_cpu(A.without_priority(inp), [])["out"]).any()
    g = _sched(cl)
    out, ctr, _ = g.sweep_affinity([a for _, a in sets_], explain=True)
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    g.close()


def test_node_sharded_handle_is_refused():
    """One rank of a two-rank node-sharded scheduler (not connected: the refusal precedes any launch);
    hostname-keyed terms alone, which a shard may load."""
    from ksim import synth
    nodes, pods = synth.c2_objects(64, 50, seed=7)
    nodes = copy.deepcopy(nodes)
    for x in nodes:
        x["metadata"]["labels"]["kubernetes.io/hostname"] = x["metadata"]["name"]
    cl = ingest.Cluster.from_objects(nodes, (), _with_host_anti(pods, 0))
    s = scheduler.ShardedScheduler(cl, *A.DEFAULT, 0, 2)
    assert s.affinity is not None
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: a node-sharded handle"):
        s.sweep_affinity([[0]], None, 0, 10)
    s.close()


def test_one_node_above_the_cap_is_refused():
    cl = A.caps_input(n=abi.SWEEP_GENERAL_MAX_NODES + 1, p=4).cluster()
    g = _sched(cl)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: %d nodes exceed the %d-node scenario layout"
                       % (abi.SWEEP_GENERAL_MAX_NODES + 1, abi.SWEEP_GENERAL_MAX_NODES)):
        g.sweep_affinity([[0]])
    g.close()


def test_stale_tables_after_a_node_event_are_refused():
    """Where ksim_schedule refuses them (E_STATE), the sweep refuses under its own name."""
    g = _sched(A.rnd_input(18).cluster())
    g.h.call("ksim_node_remove", 0)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: the affinity tables predate a node event"):
        g.sweep_affinity([[1]], None, 0, 10)
    with pytest.raises(abi.KsimError, match="predate a node event") as e:
        g.schedule()
    assert e.value.code == abi.E_STATE
    g.close()
    from workloads import rnd_volume_workload
    nodes, running, pods, pvs, pvcs = rnd_volume_workload(0, resolvable_only=True)
    cl = ingest.Cluster.from_objects(nodes, running, pods, pvs=pvs, pvcs=pvcs)
    g = scheduler.GenericScheduler(cl, ["GeneralPredicates", "NoDiskConflict"], [("LeastRequestedPriority", 1)],
                                   collect_reasons=False)
    g.h.call("ksim_node_remove", 0)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: the volume tables predate a node event"):
        g.sweep_affinity([[1]], None, 0, 10)
    g.close()


def test_residents_out_of_range_are_invalid():
    inp = A.rnd_input(18)
    cl = inp.cluster()
    g = _sched(cl)
    n_ident, n_aclass = cl.affinity["n_ident"], cl.affinity["n_aclass"]
    for row, what in (([cl.n_nodes, 0, 1], "node"), ([-1, 0, 1], "node"), ([0, n_ident + 1, 0], "identity"),
                      ([0, 0, n_aclass + 1], "identity .* or class")):
        cols = [np.array([v], np.int32) for v in row]
        rs = abi.SweepResidents(1, *(abi.ptr(c, C.c_int32) for c in cols))
        out = np.zeros(4, np.int32)
        mask = scheduler.absent_mask(cl.n_nodes, [[0]])
        with pytest.raises(abi.KsimError, match="ksim_sweep_affinity: resident 0: " + what) as e:
            g.h.call("ksim_sweep_affinity", abi.vptr(mask), 1, C.byref(rs), None, 0, 4, abi.vptr(out), None, None, None,
                     None, None)
        assert e.value.code == abi.E_INVAL
    g.close()


# ---- 11. a residents list with one pod too many: E_INVAL naming the scenario, the handle untouched
def test_one_resident_too_many():
    inp, _, refs = A.rnd_refs(18)
    cl = inp.cluster()
    t = cl.affinity
    res = cl.residents

    def counted(row):  # the resident adds to a counted pair at its node
        w, ident = int(row[0]), int(row[1])
        return ident > 0 and any((int(t["ident_sel"][ident - 1, s >> 6]) >> (s & 63)) & 1 and t["dom"][k, w] >= 0
                                 for s, k in zip(t["pair_sel"].tolist(), t["pair_key"].tolist()))

    extra = next(row for row in res if counted(row))
    twice = copy.copy(cl)
    twice.residents = np.concatenate([res, extra[None, :]])
    g = _sched(twice)
    sets_ = [[], [int(extra[0])]]  # the second scenario takes the pod's pairs out twice
    with pytest.raises(abi.KsimError, match="ksim_sweep_affinity: scenario 1: a counted pair is negative") as e:
        g.sweep_affinity(sets_)
    assert e.value.code == abi.E_INVAL and not isinstance(e.value, abi.KsimUnsupported)
    head, _, _ = g.schedule()
    assert np.array_equal(head, refs[0]["out"]) and g.last_node_index == refs[0]["counter"]
    g.close()


# ---- 12. object level
def _outages(cc):
    return [("first", [0])] + [("zone-" + v, idx) for v, idx in scheduler.outage_sets(cc.cluster, A.ZONE)]


def test_cluster_capacity_what_if():
    inp = A.rnd_input(18)
    preds, prios = A.DEFAULT
    sim_pods = list(reversed(inp.queue))
    cc = scheduler.ClusterCapacity(inp.nodes, inp.running, sim_pods, provider_name="DefaultProvider", collect_reasons=False)
    failed = 0
    outages = _outages(cc)
    for r, (name, idx) in zip(cc.what_if(outages, explain=True), outages):
        gone = {cc.cluster.names[i] for i in idx}
        left = [x for x in inp.nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in inp.running if x["spec"]["nodeName"] not in gone]
        want, _ = R.simulate(left, stay, sim_pods, set(preds), list(prios))
        assert r["placements"] == [(pn, host) for pn, host, _ in want], name
        assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
        assert r["listed"] == len(left)
        failed += r["failed"]
    assert failed > 0


def test_cluster_capacity_drain_what_if():
    inp = A.rnd_input(18)
    preds, prios = A.DEFAULT
    sim_pods = list(reversed(inp.queue))
    cc = scheduler.ClusterCapacity(inp.nodes, inp.running, sim_pods, provider_name="DefaultProvider", collect_reasons=False)
    outages = _outages(cc)
    evicted_all = 0
    for r, (name, idx) in zip(cc.drain_what_if(outages, explain=True), outages):
        gone = {cc.cluster.names[i] for i in idx}
        left = [x for x in inp.nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in inp.running if x["spec"]["nodeName"] not in gone]
        evicted = [x for x in inp.running if x["spec"]["nodeName"] in gone and scheduler.default_evictable(x)]
        m = len(evicted)
        assert r["evicted"] == m
        order = [scheduler.requeue_copy(x) for x in evicted] + inp.queue
        want, _ = R.simulate(left, stay, list(reversed(order)), set(preds), list(prios))
        assert r["requeued"] == [(pn, host) for pn, host, _ in want[:m]], name
        assert r["placements"] == [(pn, host) for pn, host, _ in want[m:]], name
        assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
        evicted_all += m
    assert evicted_all > 0


# ---- 13. more scenarios than one chunk holds
def test_scenario_chunks(monkeypatch):
    inp, sets_, refs = A.rnd_refs(130)
    g = _sched(inp.cluster())
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "3")
    out, ctr, st = g.sweep_affinity([a for _, a in sets_], explain=True)
    assert st.kernel_launches == (len(sets_) + 2) // 3 and st.blocks == 3
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    g.close()
