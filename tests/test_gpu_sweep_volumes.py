"""GPU parity of the scenario sweep over volume queues (ksim_sweep_volumes, the VOL instantiations of
ksim_sweep_general_kernel): every scenario — the snapshot without its absent nodes and the running pods
bound to them, every commit adding its mounts to the scenario's own copy — must equal, bit for bit,
the reference's run on the reduced objects (tests/volume_sweep_inputs.py; the inputs' properties are
pinned on the CPU in tests/test_sweep_volume_host.py).  Every comparison is against the oracles, never
against another GPU form.  Without the entry every case here fails (no ksim_sweep_volumes)."""
import copy
import ctypes as C

import numpy as np
import pytest

import ksim_ref as R
import spread_sweep_inputs as X
import volume_sweep_inputs as V
from ksim import abi, ingest, scheduler

pytestmark = pytest.mark.gpu


def _check(sets_, refs, out, ctr, g):
    for k, ((label, _), r) in enumerate(zip(sets_, refs)):
        assert np.array_equal(out[k], r["out"]), label
        assert int(ctr[k]) == r["counter"], label
        assert int(g.last_scheduled[k]) == int((r["out"] >= 0).sum()), label


def _check_records(sets_, refs, f, cap):
    for k, ((label, _), r) in enumerate(zip(sets_, refs)):
        assert int(f["count"][k]) == r["count"] and int(f["listed"][k]) == r["listed"], label
        kept = min(r["count"], cap)
        if r["listed"]:  # (no node listed: every pod fails before any predicate; the histograms are not compared)
            assert np.array_equal(f["pod"][k, :kept], r["pod"][:kept]), label
            assert np.array_equal(f["hist"][k, :kept], r["hist"][:kept]), label
        assert (f["pod"][k, kept:] == -1).all() and (f["hist"][k, kept:] == -1).all(), label


def _texts(inp, cl, f, k, names):
    return [(names[int(f["pod"][k, j])], scheduler.fit_error_message(int(f["listed"][k]), f["hist"][k, j], cl.scalar_names.items))
            for j in range(int(f["count"][k]))]


def _state(g):
    slots, cnt = g.volume_state()
    return slots.copy(), cnt.copy(), {k: np.asarray(v).copy() for k, v in g.node_state().items()}, g.last_node_index


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3] and \
        all(np.array_equal(a[2][k], b[2][k]) for k in a[2])


# ---- 1. the hand cases and an outage of nothing: placements, counters, histograms, message texts
@pytest.mark.parametrize("case", V.HAND)
def test_hand_cases(case):
    inp = V.hand_input(case)
    cl = inp.cluster()
    sets_ = V.hand_sets(case)
    refs = [V.oracle_cpu(inp, a) for _, a in sets_]
    texts = [V.oracle_ref(inp, a) for _, a in sets_]
    g = V.scheduler_of(inp)
    before = _state(g)
    out, ctr, st = g.sweep_volumes([a for _, a in sets_], explain=True)
    assert st.mode == abi.MODE_PERSISTENT and st.kernel_launches == 1 and st.blocks == len(sets_)
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    names = [x["metadata"]["name"] for x in inp.queue]
    for k, (t, want) in enumerate(zip(texts, V.HAND_WANT[case])):
        assert np.array_equal(out[k], t["out"]), sets_[k][0]
        assert _texts(inp, cl, g.last_failures, k, names) == t["msgs"], sets_[k][0]
        assert [(nm, cl.names[w] if w >= 0 else None) for nm, w in zip(names, out[k])] == \
            [(nm, w if isinstance(w, str) else None) for nm, w in want]
    assert _same_state(before, _state(g))
    g.close()


def test_zone_outage_message():
    inp = V.hand_input("pv-zone")
    g = V.scheduler_of(inp)
    g.sweep_volumes([a for _, a in V.hand_sets("pv-zone")], explain=True)
    got = _texts(inp, inp.cluster(), g.last_failures, 1, [x["metadata"]["name"] for x in inp.queue])
    assert got == [("q", "0/2 nodes are available: 2 node(s) had no available volume zone.")]
    g.close()


# ---- 1b. drain: the evicted pod carries its disk; an evicted pod no survivor can take
@pytest.mark.parametrize("case", V.DRAIN)
def test_drain_hand_cases(case):
    inp = V.drain_input(case)
    cl = inp.cluster()
    sets_ = [("none", [])] + [(nm, [cl.index[nm]]) for nm in cl.names]
    copies, requeue, queues = V.drain_plan(inp, sets_)
    dcl = inp.cluster(extra=copies)
    g = V.scheduler_of(inp, dcl)
    out, pre, ctr, _ = g.sweep_volumes([a for _, a in sets_], requeue, 0, len(inp.queue), explain=True)
    for k, ((label, a), q) in enumerate(zip(sets_, queues)):
        r = V.oracle_ref(inp, a, queue=q + inp.queue)
        m = len(q)
        assert np.array_equal(pre[k], r["out"][:m]) and np.array_equal(out[k], r["out"][m:]), label
        assert int(ctr[k]) == r["counter"], label
        assert int(g.last_rehosted[k]) == int((r["out"][:m] >= 0).sum()), label
        assert _texts(inp, dcl, g.last_failures, k, r["names"]) == r["msgs"], label
    k = 1  # the outage of n1
    if case == "rehost-keeps-off":
        assert pre[k][0] >= 0 and out[k][0] >= 0 and out[k][0] != pre[k][0] and out[0][0] == pre[k][0]
    else:
        assert pre[k][0] == -1 and int(g.last_rehosted[k]) == 0  # stranded
    g.close()


# ---- 2. the random workloads, records with and without a cap
@pytest.mark.parametrize("cap", [None, True, 2])
@pytest.mark.parametrize("zones", [False, True])
@pytest.mark.parametrize("n_nodes", sorted(V.RND))
def test_random_workloads_match_the_reference(n_nodes, zones, cap):
    inp, sets_, refs = V.rnd_refs(n_nodes, zones)
    cl = inp.cluster()
    Q = len(inp.queue)
    g = V.scheduler_of(inp)
    assert g.volumes is not None
    before = _state(g)
    out, ctr, st = g.sweep_volumes([a for _, a in sets_], None, 0, Q, explain=cap)
    assert st.mode == abi.MODE_PERSISTENT and st.kernel_launches == 1 and st.blocks == len(sets_)
    assert st.pods == len(sets_) * Q and st.node_evals == st.pods * n_nodes
    _check(sets_, refs, out, ctr, g)
    if cap is not None:
        _check_records(sets_, refs, g.last_failures, Q if cap is True else cap)
    assert _same_state(before, _state(g))
    g.close()


# ---- 3. geometry: one node, the wave's edges, two rows per thread and a ragged last round
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_geometry(n):
    inp = V.geometry_input(n)
    sets_ = V.geometry_sets(n)
    refs = [V.oracle_cpu(inp, a) for _, a in sets_]
    g = V.scheduler_of(inp)
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_], explain=True)
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    g.close()


def test_node_with_more_mounted_keys_than_the_register_form():
    inp = V.many_mounts_input()
    cl = inp.cluster()
    busy = cl.index["busy"]
    assert int(cl.volumes["slot_count"][busy]) > 16
    sets_ = [("none", []), ("small", [cl.index["small"]])]
    refs = [V.oracle_cpu(inp, a) for _, a in sets_]
    assert refs[0]["out"].tolist() == [busy, cl.index["small"], busy, cl.index["small"]]  # evaluated there and committed to it
    g = V.scheduler_of(inp)
    before = _state(g)
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_], explain=True)
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    assert _same_state(before, _state(g))
    g.close()


def test_node_cap():
    inp = V.caps_input()
    cl = inp.cluster()
    n = cl.n_nodes
    assert n == abi.SWEEP_GENERAL_MAX_NODES
    sets_ = [("none", []), ("last-1000", list(range(n - 1000, n)))]
    refs = [V.oracle_cpu(inp, a) for _, a in sets_]
    g = V.scheduler_of(inp)
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


# ---- 4. combinations
def test_volumes_with_selector_spread():
    inp = V.spread_input()
    cl = inp.cluster()
    sets_ = V.sets_of(cl, X.ZONE)
    refs = [V.oracle_cpu(inp, a) for _, a in sets_]
    g = V.scheduler_of(inp)
    assert g.affinity is not None and not g.has_affinity_terms() and g.volumes is not None
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_], explain=True)
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    g.close()


def test_volumes_with_inter_pod_affinity():
    """A C2x-shaped queue on the IPA + VOL kernels; the zone outages lose running pods with affinity
    state, which the residents take out of the scenarios' counts."""
    inp = V.affinity_input()
    cl = inp.cluster()
    sets_ = V.sets_of(cl, V.AFF_ZONE)
    assert sum(x.startswith("zone-") for x, _ in sets_) >= 2 and len(cl.residents) > 0
    refs = [V.oracle_cpu(inp, a) for _, a in sets_]
    g = V.scheduler_of(inp)
    assert g.has_affinity_terms() and g.volumes is not None
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_], explain=True)
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    g.close()


def test_several_reduce_classes_with_volume_pods():
    inp = V.classes_input()
    cl = inp.cluster()
    assert X.max_reduce_classes(cl) > 1
    sets_ = [s for s in V.sets_of(cl) if s[0] in ("none", "first", "tenth")]
    refs = [V.oracle_cpu(inp, a) for _, a in sets_]
    g = V.scheduler_of(inp)
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_])
    _check(sets_, refs, out, ctr, g)
    g.close()


@pytest.mark.parametrize("which", ["volumes", "affinity"])
def test_prefix_queues(which):
    """The evictable running pods of every outage first, then the range; and count == 0."""
    inp = V.rnd_input(16, True) if which == "volumes" else V.affinity_input()
    sets_ = [s for s in V.sets_of(inp.cluster(), V.ZONE if which == "volumes" else V.AFF_ZONE) if s[0] != "all"]
    copies, requeue, queues = V.drain_plan(inp, sets_)
    assert sum(len(r) for r in requeue) > 0 and any(x["spec"].get("volumes") for x in copies)
    dcl = inp.cluster(extra=copies)
    Q = 40
    for count in (Q, 0):
        refs = [V.oracle_cpu(inp, a, queue=q + inp.queue[:count]) if q or count else None for (_, a), q in zip(sets_, queues)]
        g = V.scheduler_of(inp, dcl)
        out, pre, ctr, st = g.sweep_volumes([a for _, a in sets_], requeue, 0, count, explain=True)
        for k, ((label, _), r, rq) in enumerate(zip(sets_, refs, requeue)):
            m = len(rq)
            if r is None:
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


def test_prefix_and_range_of_different_kinds():
    """Volume pods in the prefixes alone, then a range without any; and the other way round."""
    inp = V.rnd_input(16)
    cl = inp.cluster()
    vol = np.nonzero(np.asarray(cl.pods)["vol_class"] > 0)[0].tolist()
    none = np.nonzero(np.asarray(cl.pods)["vol_class"] == 0)[0].tolist()
    first = next(k for k in range(len(inp.queue) - 3) if all(j in none for j in range(k, k + 3)))  # three plain pods in a row
    sets_ = [s for s in V.sets_of(cl) if s[0] in ("none", "first", "tenth")]
    g = V.scheduler_of(inp)
    for prefix, (lo, cnt) in ((vol[:5], (first, 3)), (none[:4], (vol[0], 1))):
        queue = [inp.queue[q] for q in prefix] + inp.queue[lo:lo + cnt]
        out, pre, ctr, _ = g.sweep_volumes([a for _, a in sets_], [prefix] * len(sets_), lo, cnt)
        for k, (label, a) in enumerate(sets_):
            r = V.oracle_cpu(inp, a, queue=queue)
            assert np.array_equal(pre[k], r["out"][:len(prefix)]) and np.array_equal(out[k], r["out"][len(prefix):]), label
            assert int(ctr[k]) == r["counter"], label
    g.close()


def test_range_without_a_volume_pod_on_a_handle_with_volume_tables():
    inp = V.rnd_input(16)
    cl = inp.cluster()
    none = set(np.nonzero(np.asarray(cl.pods)["vol_class"] == 0)[0].tolist())
    first = next(k for k in range(len(inp.queue) - 2) if k in none and k + 1 in none)
    sets_ = [s for s in V.sets_of(cl) if s[0] in ("none", "last")]
    g = V.scheduler_of(inp)
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_], None, first, 2)
    for k, (label, a) in enumerate(sets_):
        r = V.oracle_cpu(inp, a, queue=inp.queue[first:first + 2])
        assert np.array_equal(out[k], r["out"]) and int(ctr[k]) == r["counter"], label
    g.close()


# ---- 5. state
@pytest.mark.parametrize("which", ["volumes", "affinity"])
def test_sweep_from_mid_queue_carries_the_scheduled_mounts(which):
    inp = V.rnd_input(16) if which == "volumes" else V.affinity_input()
    cl = inp.cluster()
    sets_ = [s for s in V.sets_of(cl, V.ZONE if which == "volumes" else V.AFF_ZONE) if s[0] != "all"]
    K, Q = 10, 60
    g = V.scheduler_of(inp)
    head, _, _ = g.schedule(0, K)
    lni = g.last_node_index
    bound = [(q, int(w)) for q, w in enumerate(head) if w >= 0]
    assert any(inp.queue[q]["spec"].get("volumes") for q, _ in bound)
    objs = [(inp.queue[q], w) for q, w in bound]
    before = _state(g)
    tail = [V.oracle_ref(inp, a, queue=inp.queue[K:Q], bound=objs, counter=lni) for _, a in sets_]
    out, ctr, _ = g.sweep_volumes([a for _, a in sets_], None, K, Q - K, bound=bound)
    _check(sets_, tail, out, ctr, g)
    assert _same_state(before, _state(g))
    # the handle goes on from where schedule() left it
    rest, _, _ = g.schedule(K, Q - K)
    assert np.array_equal(rest, tail[0]["out"]) and g.last_node_index == tail[0]["counter"]
    g.close()


def test_scenario_chunks(monkeypatch):
    inp, sets_, refs = V.rnd_refs(70, True)
    g = V.scheduler_of(inp)
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "3")
    out, ctr, st = g.sweep_volumes([a for _, a in sets_], explain=True)
    assert st.kernel_launches == (len(sets_) + 2) // 3 and st.blocks == 3
    _check(sets_, refs, out, ctr, g)
    _check_records(sets_, refs, g.last_failures, len(inp.queue))
    g.close()


def test_handle_is_untouched_and_schedules_as_the_oracle():
    inp, sets_, refs = V.rnd_refs(16, True)
    g = V.scheduler_of(inp)
    before = _state(g)
    g.sweep_volumes([a for _, a in sets_])
    assert _same_state(before, _state(g))
    out, _, _ = g.schedule()
    assert np.array_equal(out, refs[0]["out"]) and g.last_node_index == refs[0]["counter"]
    g.close()


def test_one_volume_slot_too_few_overflows():
    """MostRequested packs n1, where r mounts one disk; four queue pods bring four more: five slots."""
    nodes = [V._node("n1"), V._node("n2")]
    running = [V._pod("r", [V.gce("g-r", True)], cpu="2", node="n1")]
    queue = [V._pod("q%d" % k, [V.gce("g-%d" % k, True)], cpu="500m") for k in range(4)]
    inp = V.Input(nodes, running, queue, max_vols=40, policy="volumes_only")
    need = inp.cluster().volumes["vol_slots"]
    assert need == 5
    ref = V.oracle_cpu(inp, [])
    assert (ref["out"] == inp.cluster().index["n1"]).all()
    cl = inp.ingest(nodes, running, queue, vol_slots=need - 1)
    g = V.scheduler_of(inp, cl)
    before = _state(g)
    with pytest.raises(abi.KsimError, match="ksim_sweep_volumes: a node's volume slots or host-port slots overflowed") as e:
        g.sweep_volumes([[], [1]])
    assert e.value.code == abi.E_OVERFLOW
    assert _same_state(before, _state(g))
    out, ctr, _ = g.sweep_volumes([[], [1]], None, 0, 3)  # the same layout, from a cleared word: three pods fit
    assert np.array_equal(out[0], ref["out"][:3]) and np.array_equal(out[1], ref["out"][:3])
    assert _same_state(before, _state(g))
    g.close()


# ---- 6. refusals, by message
def test_refusals():
    plain = X.rnd_input(18, True)
    g = scheduler.GenericScheduler(ingest.Cluster.from_objects(plain.nodes, [], plain.queue[:6]), *V.POLICIES["volumes_lr_bra"],
                                   collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: no volume tables are loaded .ksim_sweep_nodes, "
                       "ksim_sweep_drain and ksim_sweep_affinity sweep such a queue"):
        g.sweep_volumes([[0]])
    g.close()
    # the packed score
    inp = V.rnd_input(16)
    lim = (1 << 27) // 10
    g = scheduler.GenericScheduler(inp.cluster(), V.POLICIES["volumes_lr_bra"][0], [("LeastRequestedPriority", lim)],
                                   collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: scenario 0: weight out of range"):
        g.sweep_volumes([[0]])
    g.close()
    g = scheduler.GenericScheduler(inp.cluster(), V.POLICIES["volumes_lr_bra"][0],
                                   [("LeastRequestedPriority", lim - 1), ("MostRequestedPriority", 1)], collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: scenario 0: map scores exceed 27 bits"):
        g.sweep_volumes([[0]])
    g.close()


def test_auxiliary_and_lender_tables_are_refused():
    sp = V.spread_input()
    preds = V.POLICIES["default_zone"][0]
    prios = [("SelectorSpreadPriority", 1), ("ServiceSpreadingPriority", 1), ("LeastRequestedPriority", 1)]
    cc = scheduler.ClusterCapacity(sp.nodes, sp.running, list(reversed(sp.queue)), predicates=preds, priorities=prios,
                                   collect_reasons=False, spread=sp.listers(), pvs=sp.pvs, pvcs=sp.pvcs)
    assert cc.scheduler.volumes is not None
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: a(n auxiliary spreading priority or "
                       "CheckServiceAffinity's lender table is loaded| pod in the range carries inter-pod affinity or spread "
                       r"state \(auxiliary spreading priority or lender tables are loaded\))"):
        cc.scheduler.sweep_volumes([[0]])


def test_more_than_sixteen_reduce_classes_are_refused():
    from workloads import sixteen_class_workload
    nodes, pods = sixteen_class_workload(203, 5)
    pods = copy.deepcopy(pods)
    for x in pods:
        x["spec"]["volumes"] = [V.ebs("e-1")]
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    preds, prios = V.POLICIES["default_zone"]
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    assert g.volumes is not None
    assert ((np.asarray(g.tables["n_tt"]) * np.asarray(g.tables["n_na"]))[cl.pods["cls"]] > abi.MAX_RCLASS).all()
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: a pod class in the range has more than %d reduce "
                       "classes" % abi.MAX_RCLASS):
        g.sweep_volumes([[0]], None, 0, 4)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: the class of re-queued pod 3 has more than"):
        g.sweep_volumes([[0]], [[3]], 0, 0)
    g.close()


def _with_volume(pods, k):
    pods = copy.deepcopy(list(pods))
    pods[k]["spec"]["volumes"] = [V.ebs("e-1")]
    return pods


def test_one_zone_above_the_cap_is_refused_with_a_spread_pair():
    from test_gpu_sweep_affinity import _with_host_anti
    ci = X.caps_input(n=abi.SWEEP_SPREAD_MAX_ZONES + 1, zones=abi.SWEEP_SPREAD_MAX_ZONES + 1, p=6)
    cl = ingest.Cluster.from_objects(ci.nodes, ci.running, _with_volume(_with_host_anti(ci.queue, 2), 1), spread=ci.listers())
    assert (cl.affinity["spread_pair"] >= 0).any() and cl.affinity["n_terms"] > 0 and cl.volumes is not None
    preds, prios = V.POLICIES["default_zone"]
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: %d zones exceed the %d zones of a swept SelectorSpread "
                       "queue" % (abi.SWEEP_SPREAD_MAX_ZONES + 1, abi.SWEEP_SPREAD_MAX_ZONES)):
        g.sweep_volumes([[0]])
    assert len(g.schedule(0, 6)[0]) == 6
    g.close()


def test_node_sharded_handle_is_refused():
    from ksim import synth
    nodes, pods = synth.c2_objects(64, 50, seed=7)
    cl = ingest.Cluster.from_objects(nodes, (), _with_volume(pods, 0))
    preds, prios = V.POLICIES["volumes_lr_bra"]
    s = scheduler.ShardedScheduler(cl, preds, prios, 0, 2)
    assert s.volumes is not None
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: a node-sharded handle"):
        s.sweep_volumes([[0]], None, 0, 10)
    s.close()


def test_one_node_above_the_cap_is_refused():
    inp = V.caps_input(n=abi.SWEEP_GENERAL_MAX_NODES + 1, p=4)
    g = V.scheduler_of(inp)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: %d nodes exceed the %d-node scenario layout"
                       % (abi.SWEEP_GENERAL_MAX_NODES + 1, abi.SWEEP_GENERAL_MAX_NODES)):
        g.sweep_volumes([[0]])
    g.close()


def test_stale_tables_after_a_node_event_are_refused():
    g = V.scheduler_of(V.rnd_input(16))
    g.h.call("ksim_node_remove", 0)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: the volume tables predate a node event"):
        g.sweep_volumes([[1]], None, 0, 10)
    g.close()
    g = V.scheduler_of(V.affinity_input())
    g.h.call("ksim_node_remove", 0)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_volumes: the affinity tables predate a node event"):
        g.sweep_volumes([[1]], None, 0, 10)
    g.close()


def test_residents_out_of_range_are_invalid():
    inp = V.affinity_input()
    cl = inp.cluster()
    g = V.scheduler_of(inp)
    n_ident, n_aclass = cl.affinity["n_ident"], cl.affinity["n_aclass"]
    mask = scheduler.absent_mask(cl.n_nodes, [[0]])
    out = np.zeros(4, np.int32)
    for row, what in (([cl.n_nodes, 0, 1], "node"), ([-1, 0, 1], "node"), ([0, n_ident + 1, 0], "identity"),
                      ([0, 0, n_aclass + 1], "identity .* or class")):
        cols = [np.array([v], np.int32) for v in row]
        rs = abi.SweepResidents(1, *(abi.ptr(c, C.c_int32) for c in cols))
        with pytest.raises(abi.KsimError, match="ksim_sweep_volumes: resident 0: " + what) as e:
            g.h.call("ksim_sweep_volumes", abi.vptr(mask), 1, C.byref(rs), None, 0, 4, abi.vptr(out), None, None, None,
                     None, None)
        assert e.value.code == abi.E_INVAL
    for rs, what in ((abi.SweepResidents(-1, None, None, None), "a negative number of residents"),
                     (abi.SweepResidents(2, None, None, None), "residents without a node, aff_ident or aff_class array")):
        with pytest.raises(abi.KsimError, match="ksim_sweep_volumes: " + what) as e:
            g.h.call("ksim_sweep_volumes", abi.vptr(mask), 1, C.byref(rs), None, 0, 4, abi.vptr(out), None, None, None,
                     None, None)
        assert e.value.code == abi.E_INVAL
    g.close()


def test_the_old_entries_still_refuse_volume_queues():
    inp = V.affinity_input()
    cl = inp.cluster()
    k = int(np.nonzero(np.asarray(cl.pods)["vol_class"] > 0)[0][0])
    g = V.scheduler_of(inp)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: pod %d mounts volumes" % k):
        g.sweep_affinity([[0]], None, k, 1)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_affinity: re-queued pod %d mounts volumes" % k):
        g.sweep_affinity([[0]], [[k]], 0, 0)
    g.close()
    inp = V.rnd_input(16)
    cl = inp.cluster()
    k = int(np.nonzero(np.asarray(cl.pods)["vol_class"] > 0)[0][0])
    g = V.scheduler_of(inp)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_nodes: pod %d mounts volumes" % k):
        g.sweep(None, k, 1, absent=[[0]])
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_drain: re-queued pod %d mounts volumes" % k):
        g.sweep_drain([[0]], [[k]], 0, 0)
    g.close()


# ---- 7. object level
def _outages(cc):
    return [("none", []), ("first", [0])] + [("zone-" + v, idx) for v, idx in scheduler.outage_sets(cc.cluster, V.ZONE)]


def _custom(inp, preds):
    return {k: v for k, v in R.volume_predicates(R.VolumeListers(inp.pvs, inp.pvcs), None).items() if k in preds}


def test_cluster_capacity_what_if():
    inp = V.rnd_input(16, True)
    preds, prios = inp.keys()
    sim_pods = list(reversed(inp.queue))
    cc = scheduler.ClusterCapacity(inp.nodes, inp.running, sim_pods, predicates=preds, priorities=prios, collect_reasons=False,
                                   pvs=inp.pvs, pvcs=inp.pvcs)
    assert cc.scheduler.volumes is not None
    failed = 0
    outages = _outages(cc)
    for r, (name, idx) in zip(cc.what_if(outages, explain=True), outages):
        gone = {cc.cluster.names[i] for i in idx}
        left = [x for x in inp.nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in inp.running if x["spec"]["nodeName"] not in gone]
        want, _ = R.simulate(left, stay, sim_pods, set(preds), list(prios), custom_predicates=_custom(inp, preds))
        assert r["placements"] == [(pn, host) for pn, host, _ in want], name
        assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
        assert r["listed"] == len(left)
        failed += r["failed"]
    assert failed > 0


def test_cluster_capacity_drain_what_if():
    inp = V.rnd_input(16, True)
    preds, prios = inp.keys()
    sim_pods = list(reversed(inp.queue))
    cc = scheduler.ClusterCapacity(inp.nodes, inp.running, sim_pods, predicates=preds, priorities=prios, collect_reasons=False,
                                   pvs=inp.pvs, pvcs=inp.pvcs)
    outages = _outages(cc)
    evicted_all = stranded_all = 0
    for r, (name, idx) in zip(cc.drain_what_if(outages, explain=True), outages):
        gone = {cc.cluster.names[i] for i in idx}
        left = [x for x in inp.nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in inp.running if x["spec"]["nodeName"] not in gone]
        evicted = [x for x in inp.running if x["spec"]["nodeName"] in gone and scheduler.default_evictable(x)]
        m = len(evicted)
        order = [scheduler.requeue_copy(x) for x in evicted] + inp.queue
        want, _ = R.simulate(left, stay, list(reversed(order)), set(preds), list(prios), custom_predicates=_custom(inp, preds))
        back = sum(1 for _, host, _ in want[:m] if host is not None)
        assert (r["evicted"], r["rehosted"], r["stranded"]) == (m, back, m - back), name
        assert r["requeued"] == [(pn, host) for pn, host, _ in want[:m]], name
        assert r["placements"] == [(pn, host) for pn, host, _ in want[m:]], name
        assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
        evicted_all += m
        stranded_all += r["stranded"]
    assert evicted_all > 0
