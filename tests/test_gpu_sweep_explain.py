"""GPU parity of the explained scenario sweep (ksim_sweep_explain, include/ksim_whatif.h) in its three
forms — general, tree, scan.  Every scenario's failed pods, their FitError histograms, the failure
count and the listed-node count must equal, bit for bit, the CPU oracle's run on the snapshot from
which the scenario's absent nodes were left out (tests/explain_inputs.py; the inputs' properties
are pinned on the CPU in tests/test_sweep_explain_host.py), and the placements and counters both the
oracle's and those of the same sweep without explain."""
import ctypes as C

import numpy as np
import pytest

import explain_inputs as E
from ksim import abi, ingest, scheduler

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


def _check_records(sets_, refs, f, cap, past=-1):
    """last_failures-shaped arrays against the oracle; words past the kept records hold `past`."""
    for k, ((label, _), r) in enumerate(zip(sets_, refs)):
        assert int(f["count"][k]) == r["count"], label
        assert int(f["listed"][k]) == r["listed"], label
        kept = min(r["count"], cap)
        assert np.array_equal(f["pod"][k, :kept], r["pod"][:kept]), label
        assert np.array_equal(f["hist"][k, :kept], r["hist"][:kept]), label
        assert (f["pod"][k, kept:] == past).all() and (f["hist"][k, kept:] == past).all(), label


def _check_run(sets_, refs, out, ctr, bound):
    for k, ((label, a), r) in enumerate(zip(sets_, refs)):
        assert np.array_equal(out[k], r["out"]), label
        assert int(ctr[k]) == r["counter"], label
        assert int(bound[k]) == len(r["out"]) - r["count"], label


def _explained_equals_plain(g, scen, absent, explain, **kw):
    """sweep with explain, then without: identical placements, counters, pods bound and launches."""
    out, ctr, st = g.sweep(scen, absent=absent, explain=explain, **kw)
    bound, fails = g.last_scheduled.copy(), g.last_failures
    launches, mode = st.kernel_launches, st.mode
    o2, c2, st2 = g.sweep(scen, absent=absent, **kw)
    assert np.array_equal(out, o2) and np.array_equal(ctr, c2)
    assert st2.kernel_launches == launches and st2.mode == mode
    if absent is not None:
        assert np.array_equal(bound, g.last_scheduled)
    return out, ctr, bound, fails


def _default(cl):
    preds, prios = scheduler.provider("DefaultProvider")
    return scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)


@pytest.mark.parametrize("n,p", [(1100, 3600), (130, 420), (65, 210)])
def test_general_form_matches_oracle(n, p):
    """n = 1100: two-row ragged segments and a ragged last mask word; 130 and 65: waves without rows."""
    cl, sets_, refs = E.general_refs(n, p)
    g = _default(cl)
    before = g.node_state()
    out, ctr, bound, f = _explained_equals_plain(g, None, [a for _, a in sets_], True)
    assert g.last_stats.mode == abi.MODE_PERSISTENT and g.last_stats.kernel_launches == 1
    _check_run(sets_, refs, out, ctr, bound)
    assert f["pod"].shape == (len(sets_), p) and f["hist"].shape == (len(sets_), p, abi.NREASONS)
    _check_records(sets_, refs, f, p)
    k = [label for label, _ in sets_].index("every-node")
    assert int(f["listed"][k]) == 0 and int(f["count"][k]) == p and not f["hist"][k].any()
    assert np.array_equal(f["pod"][k], np.arange(p))
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    g.close()


def _raw(g, mask, count, cap, fill=True):
    """ksim_sweep_explain called directly on arrays holding a sentinel."""
    S = len(mask)
    out, ctr, bound = np.zeros((S, count), np.int32), np.zeros(S, np.uint64), np.zeros(S, np.int32)
    f = dict(count=np.full(S, SENTINEL, np.int32), listed=np.full(S, SENTINEL, np.int32),
             pod=np.full((S, cap), SENTINEL, np.int32), hist=np.full((S, cap, abi.NREASONS), SENTINEL, np.int32))
    s = abi.SweepFailures(cap, abi.ptr(f["count"], C.c_int32), abi.ptr(f["listed"], C.c_int32),
                          abi.ptr(f["pod"], C.c_int32) if cap else None, abi.ptr(f["hist"], C.c_int32) if cap else None)
    st = abi.Stats()
    g.h.call("ksim_sweep_explain", None, abi.vptr(mask), S, 0, count, abi.vptr(out), abi.vptr(ctr), abi.vptr(bound),
             C.byref(s) if fill else None, C.byref(st))
    return out, ctr, bound, f, st


def test_caps_keep_the_first_records_and_leave_the_rest_unwritten():
    """cap = 1, the smallest scenario's failure count, and above the largest (more than the queue
    holds): the records' stride is the caller's cap, words past the kept ones keep the sentinel."""
    cl, sets_, refs = E.general_refs(1100, 3600)
    p = len(cl.pods)
    smallest, largest = min(r["count"] for r in refs), max(r["count"] for r in refs)
    assert (smallest, largest) == (408, p)
    g = _default(cl)
    mask = scheduler.absent_mask(cl.n_nodes, [a for _, a in sets_])
    for cap in (1, smallest, largest + 1):
        out, ctr, bound, f, st = _raw(g, mask, p, cap)
        assert st.kernel_launches == 1
        _check_run(sets_, refs, out, ctr, bound)
        _check_records(sets_, refs, f, cap, past=SENTINEL)
    g.close()


def test_no_explanation_asked_is_the_plain_sweep():
    """fail = NULL and cap = 0 launch what ksim_sweep_nodes launches; cap = 0 still fills count and
    listed; explain=None is the call without the keyword."""
    cl, sets_, refs = E.general_refs(130, 420)
    p = len(cl.pods)
    absent = [a for _, a in sets_]
    g = _default(cl)
    o0, c0, st0 = g.sweep(None, absent=absent)
    b0 = g.last_scheduled.copy()
    g.last_failures = "untouched"
    o1, c1, st1 = g.sweep(None, absent=absent, explain=None)
    assert g.last_failures == "untouched"
    assert np.array_equal(o0, o1) and np.array_equal(c0, c1) and st1.kernel_launches == st0.kernel_launches == 1
    mask = scheduler.absent_mask(cl.n_nodes, absent)
    for fill in (False, True):
        out, ctr, bound, f, st = _raw(g, mask, p, 0, fill=fill)
        assert np.array_equal(out, o0) and np.array_equal(ctr, c0) and np.array_equal(bound, b0)
        assert (st.kernel_launches, st.mode, st.blocks, st.node_evals) == (st0.kernel_launches, st0.mode, st0.blocks,
                                                                           st0.node_evals)
        if fill:
            assert f["count"].tolist() == [r["count"] for r in refs]
            assert f["listed"].tolist() == [r["listed"] for r in refs]
        else:
            assert (f["count"] == SENTINEL).all() and (f["listed"] == SENTINEL).all()
    # an int 0 through the scheduler: counts without records
    g.sweep(None, absent=absent, explain=0)
    assert g.last_failures["count"].tolist() == [r["count"] for r in refs] and g.last_failures["pod"].shape == (len(refs), 0)
    with pytest.raises(abi.KsimError, match="ksim_sweep_explain: a negative record cap"):
        g.sweep(None, absent=absent, explain=-1)
    g.close()


def test_general_form_in_scenario_chunks(monkeypatch):
    """Launches of three scenarios: the records land at their scenarios' offsets."""
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "3")
    cl, sets_, refs = E.general_refs(130, 420)
    g = _default(cl)
    out, ctr, bound, f = _explained_equals_plain(g, None, [a for _, a in sets_], 50)
    assert g.last_stats.kernel_launches == (len(sets_) + 2) // 3 and g.last_stats.blocks == 3
    _check_run(sets_, refs, out, ctr, bound)
    _check_records(sets_, refs, f, 50)
    g.close()


def test_general_form_under_scenario_weights():
    """A scheduler of map priorities only over the tightened queue: two policies, without node sets
    (absent = NULL) and with one each."""
    cl = E.tight_cluster(130, 420)
    p = len(cl.pods)
    preds = list(scheduler.DEFAULT_PREDICATES)
    g = scheduler.GenericScheduler(cl, preds, E.MAP_POLICIES[0], collect_reasons=False)
    for absent in (None, [[31, 32], [cl.n_nodes - 1]]):
        sets_ = [("policy-%d" % k, a) for k, a in enumerate(absent or [[], []])]
        refs = [E.oracle(cl, g.tables, g.na_add, scheduler.make_config(preds, pri), a)
                for pri, (_, a) in zip(E.MAP_POLICIES, sets_)]
        assert all(0 < r["count"] < p for r in refs) and not np.array_equal(refs[0]["out"], refs[1]["out"])
        out, ctr, bound, f = _explained_equals_plain(g, E.MAP_POLICIES, absent, True)
        assert g.last_stats.mode == abi.MODE_PERSISTENT
        _check_run(sets_, refs, out, ctr, bound)
        _check_records(sets_, refs, f, p)
    g.close()


def _resource_scheduler(cl):
    """The resource-only input with its first RES_FIRST pods scheduled (explain_inputs.RES_FIRST)."""
    _, preds, prios = E.c3_cluster()
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    pre, _, ctr = E.resource_prefix()
    got, _, _ = g.schedule(0, E.RES_FIRST)
    assert np.array_equal(got, pre) and (pre >= 0).all() and g.last_node_index == ctr
    return g


@pytest.mark.parametrize("form", ["tree", "scan", "tree-chunked"])
@pytest.mark.parametrize("weighted", [False, True], ids=["absent-sets", "scenario-weights"])
def test_resource_only_forms_match_oracle(monkeypatch, form, weighted):
    """config_c3(1100, 60000), swept from pod 30,000 on: 26,893 failures in long runs.  cap = 1000
    truncates every scenario; in the tree form a class's histogram is copied from its last record
    until the next commit, up to and not beyond the cap."""
    if form == "scan":
        monkeypatch.setenv("KSIM_SWEEP_SCAN", "1")
    if form == "tree-chunked":
        monkeypatch.setenv("KSIM_SWEEP_CHUNK", "3")
    cl, scen, sets_, refs = E.resource_refs(weighted)
    g = _resource_scheduler(cl)
    absent = None if weighted else [a for _, a in sets_]
    out, ctr, bound, f = _explained_equals_plain(g, scen, absent, 1000, first=E.RES_FIRST)
    assert g.last_stats.mode == (abi.MODE_PERSISTENT if form == "scan" else abi.MODE_TREE)
    if form == "tree-chunked" and not weighted:
        assert g.last_stats.kernel_launches == 2 and g.last_stats.blocks == 3
    _check_run(sets_, refs, out, ctr, bound)
    _check_records(sets_, refs, f, 1000)
    g.close()


@pytest.mark.parametrize("form", ["tree", "scan"])
def test_resource_only_forms_keep_every_record(monkeypatch, form):
    """explain=True on 6,000 pods: 3,000 and more failures per scenario, every one kept."""
    if form == "scan":
        monkeypatch.setenv("KSIM_SWEEP_SCAN", "1")
    count = 6000
    cl, _, sets_, refs = E.resource_refs(False, count)
    assert all(r["count"] > 3000 for r in refs)
    g = _resource_scheduler(cl)
    out, ctr, bound, f = _explained_equals_plain(g, None, [a for _, a in sets_], True, first=E.RES_FIRST, count=count)
    _check_run(sets_, refs, out, ctr, bound)
    _check_records(sets_, refs, f, count)
    g.close()


def test_nodename_pod_whose_node_is_absent():
    """Every listed node fails PodFitsHost for it: slot R_HOSTNAME equals listed."""
    cl, its_node = E.nodename_input()
    p, pod = len(cl.pods), E.NODENAME_POD
    g = _default(cl)
    cfg = scheduler.make_config(*scheduler.provider("DefaultProvider"))
    sets_ = [("none", []), ("nodename", [its_node]), ("every-second", list(range(0, cl.n_nodes, 2)))]
    refs = [E.oracle(cl, g.tables, g.na_add, cfg, a) for _, a in sets_]
    out, ctr, bound, f = _explained_equals_plain(g, None, [a for _, a in sets_], True)
    _check_run(sets_, refs, out, ctr, bound)
    _check_records(sets_, refs, f, p)
    assert out[0][pod] == its_node and out[1][pod] == -1
    k = int(np.nonzero(f["pod"][1, :int(f["count"][1])] == pod)[0][0])
    assert int(f["hist"][1, k, abi.R_HOSTNAME]) == int(f["listed"][1]) == cl.n_nodes - 1
    g.close()


def test_cluster_capacity_what_if_explains_on_objects():
    """what_if(explain=True) on the tightened recipe at 48 nodes against ksim_ref.simulate on the object
    lists without the outage's nodes: the FitError messages string-equal; an outage of every node
    gives ERR_NO_NODES; an int cap keeps that many."""
    import ksim_ref as R
    from ksim.report import ERR_NO_NODES
    nodes, pods = E.tight_objects(48, 150)
    preds, prios = scheduler.provider("DefaultProvider")
    cc = scheduler.ClusterCapacity(nodes, [], pods, provider_name="DefaultProvider", collect_reasons=False)
    per_node = scheduler.outage_sets(cc.cluster, "node")
    outages = per_node[:3] + [("tier-a", dict(scheduler.outage_sets(cc.cluster, "tier"))["a"]),
                              ("everything", list(range(cc.cluster.n_nodes)))]
    plain = cc.what_if(outages)
    recs = cc.what_if(outages, explain=True)
    capped = cc.what_if(outages, explain=2)
    failed_somewhere = 0
    for r, r0, r2, (name, idx) in zip(recs, plain, capped, outages):
        assert {k: r[k] for k in r0} == r0  # explaining changes no record of today's
        assert set(r) - set(r0) == {"listed", "fit_errors", "explained"}
        gone = {cc.cluster.names[i] for i in idx}
        left = [x for x in nodes if x["metadata"]["name"] not in gone]
        assert r["listed"] == len(left) and r["explained"] == r["failed"] == len(r["fit_errors"])
        if not left:
            with pytest.raises(RuntimeError, match=ERR_NO_NODES):
                R.simulate(left, [], pods, set(preds), prios)
            assert r["fit_errors"] == [(pn, ERR_NO_NODES) for pn, _ in r["placements"]]
        else:
            want, _ = R.simulate(left, [], pods, set(preds), prios)
            assert r["placements"] == [(pn, host) for pn, host, _ in want], name
            assert r["fit_errors"] == [(pn, msg) for pn, host, msg in want if host is None], name
            failed_somewhere += r["failed"]
        assert r2["explained"] == min(2, r["failed"]) and r2["fit_errors"] == r["fit_errors"][:2]
    assert failed_somewhere > 20
