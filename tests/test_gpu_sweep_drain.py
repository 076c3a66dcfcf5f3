"""GPU parity of the drain sweep (ksim_sweep_drain, include/ksim_drain.h): every scenario — the
snapshot without its absent nodes, the pods that ran on them re-queued in front of the queue — must
equal, bit for bit, the CPU oracle's run on the reduced cluster over that scenario's own queue
(tests/drain_inputs.py; the inputs' properties are pinned on the CPU in
tests/test_sweep_drain_host.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

import drain_inputs as D
from ksim import abi, ingest, scheduler

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SMALL = (130, 420, 300)


def _default(cl):
    preds, prios = scheduler.provider("DefaultProvider")
    return scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)


def _check_run(sets_, refs, out, pre, ctr, g):
    for k, ((label, _), r) in enumerate(zip(sets_, refs)):
        assert np.array_equal(pre[k], r["pre"]), label
        assert np.array_equal(out[k], r["out"]), label
        assert int(ctr[k]) == r["counter"], label
        assert int(g.last_scheduled[k]) == int((r["out"] >= 0).sum()), label
        assert int(g.last_rehosted[k]) == int((r["pre"] >= 0).sum()), label


def _check_records(sets_, refs, f, cap, past=-1):
    for k, ((label, _), r) in enumerate(zip(sets_, refs)):
        assert int(f["count"][k]) == r["count"], label
        assert int(f["listed"][k]) == r["listed"], label
        kept = min(r["count"], cap)
        assert np.array_equal(f["pod"][k, :kept], r["pod"][:kept]), label
        assert np.array_equal(f["hist"][k, :kept], r["hist"][:kept]), label
        assert (f["pod"][k, kept:] == past).all() and (f["hist"][k, kept:] == past).all(), label


# ---- 1. parity
@pytest.mark.parametrize("n,p,R", D.SIZES)
def test_drain_matches_oracle(n, p, R):
    """n = 1100: two-row ragged segments and a ragged last mask word; 130 and 65: waves without rows."""
    cl, Q, sets_, refs, plain = D.refs(n, p, R)
    g = _default(cl)
    before = g.node_state()
    out, pre, ctr, st = g.sweep_drain([a for _, a in sets_], [r["requeue"] for r in refs], 0, Q)
    assert st.mode == abi.MODE_PERSISTENT and st.kernel_launches == 1 and st.blocks == len(sets_)
    total = sum(r["m"] for r in refs) + len(sets_) * Q
    assert st.pods == total and st.node_evals == total * n
    assert out.shape == (len(sets_), Q) and [len(x) for x in pre] == [r["m"] for r in refs]
    _check_run(sets_, refs, out, pre, ctr, g)
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    got, _, _ = g.schedule(0, Q)
    none = plain[[label for label, _ in sets_].index("none")]
    assert np.array_equal(got, none["out"]) and g.last_node_index == none["counter"]
    g.close()


# ---- 2. empty prefixes
def test_empty_prefixes_are_the_plain_sweep():
    cl, Q, sets_, _, plain = D.refs(*SMALL)
    absent = [a for _, a in sets_]
    g = _default(cl)
    o0, c0, st0 = g.sweep(None, 0, Q, absent=absent)
    b0 = g.last_scheduled.copy()
    out, pre, ctr, st = g.sweep_drain(absent, [[] for _ in absent], 0, Q)
    assert np.array_equal(out, o0) and np.array_equal(ctr, c0) and np.array_equal(g.last_scheduled, b0)
    assert all(len(x) == 0 for x in pre) and not g.last_rehosted.any()
    assert (st.kernel_launches, st.mode, st.blocks, st.node_evals) == (st0.kernel_launches, st0.mode, st0.blocks,
                                                                       st0.node_evals)
    for k, r in enumerate(plain):
        assert np.array_equal(out[k], r["out"]) and int(ctr[k]) == r["counter"]
    # absent = NULL: no node absent in any scenario
    out, _, ctr, _ = g.sweep_drain(None, [[], []], 0, Q)
    none = plain[[label for label, _ in sets_].index("none")]
    assert all(np.array_equal(o, none["out"]) for o in out) and [int(x) for x in ctr] == [none["counter"]] * 2
    g.close()


# ---- 3. count == 0
@pytest.mark.parametrize("n,p,R", D.SIZES[1:])
def test_only_rehosting(n, p, R):
    """count == 0: the prefix part alone, the oracle re-run with an empty range; out_node NULL."""
    cl, Q, sets_, full, _ = D.refs(n, p, R)
    refs = [D.oracle(n, p, R, a, count=0) for _, a in sets_]
    for r, r1 in zip(refs, full):  # the prefix is scheduled first: the range cannot change it
        assert np.array_equal(r["pre"], r1["pre"])
    g = _default(cl)
    out, pre, ctr, st = g.sweep_drain([a for _, a in sets_], [r["requeue"] for r in refs], 0, 0)
    assert out.shape == (len(sets_), 0) and st.pods == sum(r["m"] for r in refs)
    _check_run(sets_, refs, out, pre, ctr, g)
    # called raw with out_node = NULL, and with the range elsewhere in the queue
    S = len(sets_)
    off = np.zeros(S + 1, np.int64)
    off[1:] = np.cumsum([r["m"] for r in refs])
    pod = np.concatenate([r["requeue"] for r in refs])
    ans = np.full(len(pod), SENTINEL, np.int32)
    rq = abi.SweepRequeue(abi.ptr(off, C.c_int64), abi.ptr(pod, C.c_int64), abi.ptr(ans, C.c_int32))
    mask = scheduler.absent_mask(n, [a for _, a in sets_])
    back = np.zeros(S, np.int32)
    g.h.call("ksim_sweep_drain", abi.vptr(mask), S, C.byref(rq), 7, 0, None, None, None, abi.vptr(back), None, None)
    assert np.array_equal(ans, np.concatenate([r["pre"] for r in refs]))
    assert back.tolist() == [int((r["pre"] >= 0).sum()) for r in refs]
    with pytest.raises(abi.KsimError, match="ksim_sweep_drain: neither re-queued pods nor a pod range"):
        g.sweep_drain([[0]], [[]], 0, 0)
    g.close()


# ---- 4. prefix and range of different kinds
@pytest.mark.parametrize("strip", ["queue", "prefix"])
def test_prefix_and_range_of_different_kinds(strip):
    """A resource-only range behind prefix pods with selectors, ports and tolerations, and the
    reverse: always the general form."""
    n, p, R = SMALL
    cl, Q, _ = D.cluster(n, p, R, strip)
    part = cl.pods[:Q] if strip == "queue" else cl.pods[Q:]
    other = cl.pods[Q:] if strip == "queue" else cl.pods[:Q]
    assert not part["port_cnt"].any() and not (part["flags"] & abi.POD_NEED_SELECTOR).any()
    assert other["port_cnt"].any() and (other["flags"] & abi.POD_NEED_SELECTOR).any()
    sets_ = [s for s in D.all_sets(n, p, R) if s[0] in ("first", "none", "random-third", "tier-a", "tier-b", "every-node")]
    refs = [D.oracle(n, p, R, a, strip=strip) for _, a in sets_]
    assert any(0 < int((r["pre"] >= 0).sum()) < r["m"] for r in refs)
    g = _default(cl)
    out, pre, ctr, st = g.sweep_drain([a for _, a in sets_], [r["requeue"] for r in refs], 0, Q)
    assert st.mode == abi.MODE_PERSISTENT
    _check_run(sets_, refs, out, pre, ctr, g)
    g.close()


# ---- 5. chunks
def test_scenario_chunks(monkeypatch):
    """Launches of three scenarios: the kernel indexes the prefix lists by the sweep's scenario."""
    cl, Q, sets_, refs, _ = D.refs(*SMALL)
    assert len(sets_) >= 8
    absent, requeue = [a for _, a in sets_], [r["requeue"] for r in refs]
    g = _default(cl)
    o1, p1, c1, st1 = g.sweep_drain(absent, requeue, 0, Q, explain=40)
    f1 = g.last_failures
    assert st1.kernel_launches == 1
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "3")
    out, pre, ctr, st = g.sweep_drain(absent, requeue, 0, Q, explain=40)
    assert st.kernel_launches == (len(sets_) + 2) // 3 and st.blocks == 3
    assert np.array_equal(out, o1) and np.array_equal(ctr, c1)
    assert all(np.array_equal(x, y) for x, y in zip(pre, p1))
    for key in f1:
        assert np.array_equal(g.last_failures[key], f1[key]), key
    _check_run(sets_, refs, out, pre, ctr, g)
    _check_records(sets_, refs, g.last_failures, 40)
    g.close()


# ---- 6. explain
def _raw(g, n, sets_, refs, Q, cap):
    """ksim_sweep_drain called directly on record arrays holding a sentinel."""
    S = len(sets_)
    off = np.zeros(S + 1, np.int64)
    off[1:] = np.cumsum([r["m"] for r in refs])
    pod = np.concatenate([r["requeue"] for r in refs])
    ans = np.zeros(len(pod), np.int32)
    rq = abi.SweepRequeue(abi.ptr(off, C.c_int64), abi.ptr(pod, C.c_int64), abi.ptr(ans, C.c_int32))
    mask = scheduler.absent_mask(n, [a for _, a in sets_])
    out, ctr = np.zeros((S, Q), np.int32), np.zeros(S, np.uint64)
    f = dict(count=np.full(S, SENTINEL, np.int32), listed=np.full(S, SENTINEL, np.int32),
             pod=np.full((S, cap), SENTINEL, np.int32), hist=np.full((S, cap, abi.NREASONS), SENTINEL, np.int32))
    s = abi.SweepFailures(cap, abi.ptr(f["count"], C.c_int32), abi.ptr(f["listed"], C.c_int32),
                          abi.ptr(f["pod"], C.c_int32), abi.ptr(f["hist"], C.c_int32))
    st = abi.Stats()
    g.h.call("ksim_sweep_drain", abi.vptr(mask), S, C.byref(rq), 0, Q, abi.vptr(out), abi.vptr(ctr), None, None,
             C.byref(s), C.byref(st))
    return out, [ans[off[k]:off[k + 1]] for k in range(S)], ctr, f, st


@pytest.mark.parametrize("n,p,R", D.SIZES[:2])
def test_explained_drain_matches_oracle(n, p, R):
    """Every record: queue positions (prefix first), histograms, count, listed; and no placement moves."""
    cl, Q, sets_, refs, _ = D.refs(n, p, R)
    absent, requeue = [a for _, a in sets_], [r["requeue"] for r in refs]
    g = _default(cl)
    o0, p0, c0, _ = g.sweep_drain(absent, requeue, 0, Q)
    out, pre, ctr, st = g.sweep_drain(absent, requeue, 0, Q, explain=True)
    f = g.last_failures
    longest = max(r["m"] for r in refs) + Q
    assert f["pod"].shape == (len(sets_), longest) and st.kernel_launches == 1
    assert np.array_equal(out, o0) and np.array_equal(ctr, c0) and all(np.array_equal(x, y) for x, y in zip(pre, p0))
    _check_run(sets_, refs, out, pre, ctr, g)
    _check_records(sets_, refs, f, longest)
    k = [label for label, _ in sets_].index("every-node")
    assert int(f["listed"][k]) == 0 and int(f["count"][k]) == refs[k]["m"] + Q and not f["hist"][k, :refs[k]["m"] + Q].any()
    assert np.array_equal(f["pod"][k, :refs[k]["m"] + Q], np.arange(refs[k]["m"] + Q))
    g.close()


def test_caps_count_over_the_scenario_queue():
    """cap = 1 and a cap inside tier-a's prefix: the stride is the caller's cap, the words past the
    kept records keep the sentinel."""
    n, p, R = SMALL
    cl, Q, sets_, refs, _ = D.refs(n, p, R)
    a = refs[[label for label, _ in sets_].index("tier-a")]
    inside = 10
    assert int(a["pod"][inside - 1]) < a["m"] - 1 and int((a["pod"] < a["m"]).sum()) > inside  # falls inside the prefix
    g = _default(cl)
    for cap in (1, inside, max(r["m"] for r in refs) + Q + 1):
        out, pre, ctr, f, st = _raw(g, n, sets_, refs, Q, cap)
        for k, ((label, _), r) in enumerate(zip(sets_, refs)):
            assert np.array_equal(pre[k], r["pre"]) and np.array_equal(out[k], r["out"]) and int(ctr[k]) == r["counter"], label
        _check_records(sets_, refs, f, cap, past=SENTINEL)
    g.close()


# ---- 7. refusals
def test_refusals_leave_the_handle_usable():
    n, p, R = SMALL
    cl, Q, sets_, refs, _ = D.refs(n, p, R)
    g = _default(cl)
    with pytest.raises(abi.KsimError, match="ksim_sweep_drain: re-queued pod index %d outside" % len(cl.pods)) as e:
        g.sweep_drain([[0], [1]], [[Q], [Q + 1, len(cl.pods)]], 0, Q)
    assert e.value.code == abi.E_INVAL
    with pytest.raises(abi.KsimError, match="ksim_sweep_drain: re-queued pod index -1 outside"):
        g.sweep_drain([[0]], [[-1]], 0, Q)
    k = [label for label, _ in sets_].index("tier-b")
    out, pre, ctr, _ = g.sweep_drain([sets_[k][1]], [refs[k]["requeue"]], 0, Q)
    _check_run(sets_[k:k + 1], refs[k:k + 1], out, pre, ctr, g)
    g.close()


def test_affinity_and_volume_pods_in_a_prefix_are_refused():
    from workloads import rnd_affinity_workload, rnd_volume_workload
    preds, prios = scheduler.provider("DefaultProvider")
    nodes, running, pods = rnd_affinity_workload(1, n_nodes=20, n_pods=40)
    cl = ingest.Cluster.from_objects(nodes, running, pods)
    k = int(np.nonzero(cl.pods["aff_class"] > 0)[0][0])
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_drain: re-queued pod %d carries inter-pod affinity" % k):
        g.sweep_drain([[0], []], [[], [k]], 0, 0)
    assert len(g.schedule(0, 5)[0]) == 5
    g.close()
    nodes, running, pods, pvs, pvcs = rnd_volume_workload(0, resolvable_only=True)
    cl = ingest.Cluster.from_objects(nodes, running, pods, pvs=pvs, pvcs=pvcs)
    k = int(np.nonzero(cl.pods["vol_class"] > 0)[0][0])
    vol_preds = ["GeneralPredicates", "NoDiskConflict", "MaxEBSVolumeCount", "MaxGCEPDVolumeCount"]
    g = scheduler.GenericScheduler(cl, vol_preds, [("LeastRequestedPriority", 1)], collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_drain: re-queued pod %d mounts volumes" % k):
        g.sweep_drain([[0], []], [[k], []], 0, 0)
    assert len(g.schedule(0, 5)[0]) == 5
    g.close()


def test_node_sharded_handle_is_refused():
    """One rank of a two-rank node-sharded scheduler (not connected: the refusal precedes any launch)."""
    cl, Q, _ = D.cluster(*SMALL)
    preds, prios = scheduler.provider("DefaultProvider")
    s = scheduler.ShardedScheduler(cl, preds, prios, 0, 2)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_drain: a node-sharded handle"):
        s.sweep_drain([[0]], [[Q]], 0, Q)
    s.close()


# ---- 8. object level
def test_cluster_capacity_drain_what_if_on_objects():
    """drain_what_if on 40 nodes against ksim_ref.simulate on the reduced object lists, the simulator
    fed the reversed evicted copies + queue (it pops LIFO): pod -> node names and FitError texts."""
    import ksim_ref as R
    from ksim.report import ERR_NO_NODES
    nodes, running, queue = D.objects(40, 130, 90)
    running = copy.deepcopy(running)
    preds, prios = scheduler.provider("DefaultProvider")
    cl0 = ingest.Cluster.from_objects(nodes, running, queue)
    tier_a = dict(scheduler.outage_sets(cl0, "tier"))["a"]
    lost = cl0.names[tier_a[0]]  # absent in all three outages
    extra = [{"metadata": {"name": "ds-pod", "namespace": "default", "ownerReferences": [{"kind": "DaemonSet", "name": "d"}]},
              "spec": {"nodeName": lost, "containers": [{"resources": {"requests": {"cpu": "100m"}}}]}},
             {"metadata": {"name": "done-pod", "namespace": "default"},
              "spec": {"nodeName": lost, "containers": [{"resources": {"requests": {"cpu": "100m"}}}]},
              "status": {"phase": "Succeeded"}}]
    running = running[:10] + extra + running[10:]
    sim_pods = list(reversed(queue))  # PodQueue.Pop takes the last element: the queue in scheduling order
    cc = scheduler.ClusterCapacity(nodes, running, sim_pods, provider_name="DefaultProvider", collect_reasons=False)
    outages = [("node", [lost]), ("tier-a", tier_a), ("everything", list(range(cc.cluster.n_nodes)))]
    plain = cc.drain_what_if(outages)
    recs = cc.drain_what_if(outages, explain=True)
    capped = cc.drain_what_if(outages, explain=2)
    stranded = 0
    for r, r0, r2, (name, idx) in zip(recs, plain, capped, outages):
        assert {k: r[k] for k in r0} == r0  # explaining changes no record
        assert set(r) - set(r0) == {"listed", "fit_errors", "explained"}
        gone = {i if isinstance(i, str) else cc.cluster.names[i] for i in idx}  # an outage names nodes or indexes them
        left = [x for x in nodes if x["metadata"]["name"] not in gone]
        stay = [x for x in running if x["spec"]["nodeName"] not in gone]
        evicted = [x for x in running if x["spec"]["nodeName"] in gone and scheduler.default_evictable(x)]
        assert "ds-pod" not in [x["metadata"]["name"] for x in evicted] and len(evicted) < len(running) - len(stay)
        m = len(evicted)
        assert (r["absent"], r["evicted"], r["listed"]) == (len(idx), m, len(left))
        assert [pn for pn, _ in r["requeued"]] == [x["metadata"]["name"] for x in evicted]
        assert r["rehosted"] + r["stranded"] == m and r["scheduled"] + r["failed"] == len(queue)
        assert r["explained"] == r["stranded"] + r["failed"] == len(r["fit_errors"])
        if not left:
            assert r["rehosted"] == 0 and r["scheduled"] == 0
            assert r["fit_errors"] == [(pn, ERR_NO_NODES) for pn, _ in r["requeued"] + r["placements"]]
        else:
            sched_order = [scheduler.requeue_copy(x) for x in evicted] + queue
            want, _ = R.simulate(left, stay, list(reversed(sched_order)), set(preds), prios)
            assert r["requeued"] == [(pn, host) for pn, host, _ in want[:m]], name
            assert r["placements"] == [(pn, host) for pn, host, _ in want[m:]], name
            assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
            stranded += r["stranded"]
        assert r2["explained"] == min(2, r["explained"]) and r2["fit_errors"] == r["fit_errors"][:2]
    assert stranded > 0 and recs[1]["rehosted"] > 0
    assert cc.drain_what_if(outages[:1], count=0)[0]["requeued"] == recs[0]["requeued"]
