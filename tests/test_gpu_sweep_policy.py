"""GPU parity of the policy sweep (ksim_sweep_policy, include/ksim_polsweep.h): every scenario — a
prioritizer list that may rescale or drop TaintToleration, NodeAffinity, SelectorSpread and InterPodAffinity
beside the map priorities — must equal, bit for bit, the reference's run on the reduced objects under
that list (tests/policy_sweep_inputs.py; the inputs' properties are pinned on the CPU in
tests/test_sweep_policy_host.py), and its outcome record the host recount from the oracle's placements.
Every comparison is against the oracles, never against another GPU form.  Without the entry every case
that calls sweep_policy fails (no ksim_sweep_policy)."""
import numpy as np
import pytest

import policy_sweep_inputs as PI
import volume_sweep_inputs as V
from ksim import abi, scheduler, synth
from ksim.ingest import Unsupported

pytestmark = pytest.mark.gpu
SIZES = [n for n, _ in PI.RND_SIZES]


def _check(refs, out, ctr, g):
    for k, r in enumerate(refs):
        assert np.array_equal(out[k], r["out"]), k
        assert int(ctr[k]) == r["counter"], k
        assert int(g.last_scheduled[k]) == int((r["out"] >= 0).sum()), k


def _check_records(refs, f, cap):
    for k, r in enumerate(refs):
        assert int(f["count"][k]) == r["count"] and int(f["listed"][k]) == r["listed"], k
        kept = min(r["count"], cap)
        if r["listed"]:
            assert np.array_equal(f["pod"][k, :kept], r["pod"][:kept]), k
            assert np.array_equal(f["hist"][k, :kept], r["hist"][:kept]), k
        assert (f["pod"][k, kept:] == -1).all() and (f["hist"][k, kept:] == -1).all(), k


def _check_outcome(got, want):
    """got: last_outcome; want: one host recount per scenario."""
    for k, rec in enumerate(want):
        assert int(got["listed"][k]) == rec["listed"] and int(got["used"][k]) == rec["used"], k
        assert [int(v) for v in got["free_cpu"][k]] == rec["free_cpu"], k
        assert [int(v) for v in got["free_mem"][k]] == rec["free_mem"], k


def _texts(cl, f, k, names):
    return [(names[int(f["pod"][k, j])], scheduler.fit_error_message(int(f["listed"][k]), f["hist"][k, j], cl.scalar_names.items))
            for j in range(int(f["count"][k]))]


def _state(g):
    vol = g.volume_state() if g.volumes is not None else (np.zeros(0), np.zeros(0))
    return vol[0].copy(), vol[1].copy(), {k: np.asarray(v).copy() for k, v in g.node_state().items()}, g.last_node_index


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3] and \
        all(np.array_equal(a[2][k], b[2][k]) for k in a[2])


# ---- 1. the full workload under the default provider: placements, counters, last_scheduled, records
#         and outcome records per scenario; the handle untouched (its counts too: the schedule() that
#         follows reads them and equals the provider's own scenario)
@pytest.mark.parametrize("n", SIZES)
def test_full_workload_matches_the_reference_per_scenario(n):
    inp, scen, refs = PI.full_refs(n)
    cl = inp.cluster()
    Q = len(inp.queue)
    g = V.scheduler_of(inp)
    assert g.affinity is not None and g.has_affinity_terms()
    before = _state(g)
    out, ctr, st = g.sweep_policy(scen, explain=True, outcome=True)
    assert st.mode == abi.MODE_PERSISTENT and st.kernel_launches == 1 and st.blocks == len(scen)
    assert st.pods == len(scen) * Q and st.node_evals == st.pods * n
    _check(refs, out, ctr, g)
    _check_records(refs, g.last_failures, Q)
    _check_outcome(g.last_outcome, [PI.outcome_of_answer(cl, (), r["out"]) for r in refs])
    assert _same_state(before, _state(g))
    got, _, _ = g.schedule()
    assert np.array_equal(got, refs[0]["out"]) and g.last_node_index == refs[0]["counter"]
    g.close()


def test_message_texts_match_the_reference():
    inp, scen, refs = PI.full_refs(18)
    cl = inp.cluster()
    names = [x["metadata"]["name"] for x in inp.queue]
    pick = [0, 1, 5, 7, 10]
    g = V.scheduler_of(inp)
    out, _, _ = g.sweep_policy([scen[k] for k in pick], explain=True)
    for j, k in enumerate(pick):
        t = PI.oracle_messages(inp, scen[k])
        assert np.array_equal(out[j], t["out"]), k
        assert _texts(cl, g.last_failures, j, names) == t["msgs"] and t["msgs"], k
    g.close()


# ---- 2. scenario counts at the context kernel's block edge: a short list, repeated
@pytest.mark.parametrize("S", [1, 64, 65])
def test_scenario_counts_at_the_context_block_edge(S):
    inp, scen, refs = PI.full_refs(18)
    cl = inp.cluster()
    pick = [0, 1, 5, 7, 10]
    idx = [pick[k % len(pick)] for k in range(S)]
    g = V.scheduler_of(inp)
    out, ctr, st = g.sweep_policy([scen[k] for k in idx], outcome=True)
    assert st.blocks == S and out.shape == (S, len(inp.queue))
    _check([refs[k] for k in idx], out, ctr, g)
    _check_outcome(g.last_outcome, [PI.outcome_of_answer(cl, (), refs[k]["out"]) for k in idx])
    g.close()


# ---- 3. chunks of two scenarios: the same outputs and outcome records as one launch and as the oracle
def test_chunked_sweep_equals_the_unchunked_one_and_the_reference(monkeypatch):
    inp, scen, refs = PI.full_refs(70)
    cl = inp.cluster()
    g = V.scheduler_of(inp)
    monkeypatch.delenv("KSIM_SWEEP_CHUNK", raising=False)
    whole = g.sweep_policy(scen, explain=3, outcome=True)
    whole_f = {k: v.copy() for k, v in g.last_failures.items()}
    whole_o = {k: v.copy() for k, v in g.last_outcome.items()}
    assert whole[2].kernel_launches == 1
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "2")  # (the runtime reads it in every call)
    out, ctr, st = g.sweep_policy(scen, explain=3, outcome=True)
    assert st.kernel_launches == (len(scen) + 1) // 2 and st.blocks == 2
    assert np.array_equal(out, whole[0]) and np.array_equal(ctr, whole[1])
    for k in whole_f:
        assert np.array_equal(g.last_failures[k], whole_f[k]), k
    for k in whole_o:
        assert np.array_equal(g.last_outcome[k], whole_o[k]), k
    _check(refs, out, ctr, g)
    _check_records(refs, g.last_failures, 3)
    _check_outcome(g.last_outcome, [PI.outcome_of_answer(cl, (), r["out"]) for r in refs])
    g.close()


# ---- 4. each instantiation once
def _sweep_and_check(inp, scen, absent=None, **kw):
    cl = inp.cluster()
    sets_ = absent if absent is not None else [[]] * len(scen)
    refs = [PI.oracle(inp, pri, a) for pri, a in zip(scen, sets_)]
    g = V.scheduler_of(inp)
    before = _state(g)
    out, ctr, st = g.sweep_policy(scen, absent=absent, outcome=True, **kw)
    assert st.mode == abi.MODE_PERSISTENT
    _check(refs, out, ctr, g)
    _check_outcome(g.last_outcome, [PI.outcome_of_answer(cl, a, r["out"]) for r, a in zip(refs, sets_)])
    assert _same_state(before, _state(g))
    return g, refs, out


def test_plain_instantiation_with_several_reduce_classes():
    inp = PI.plain_input()
    g, refs, out = _sweep_and_check(inp, PI.scenarios_of())
    assert g.affinity is None and g.volumes is None and len({o.tobytes() for o in out}) >= 3
    g.close()


def test_spread_instantiation_over_a_queue_with_services():
    inp = PI.spread_input()
    g, refs, out = _sweep_and_check(inp, PI.scenarios_of())
    assert g.affinity is not None and not g.has_affinity_terms()
    assert not np.array_equal(out[0], out[5])  # SelectorSpread dropped
    g.close()


def test_affinity_instantiation_of_anti_affinity_replicas_with_residents():
    inp = PI.anti_input()
    cl = inp.cluster()
    zones = [list(idx) for _, idx in scheduler.outage_sets(cl, PI.A.ZONE)]
    base = list(PI.DEFAULT_PRIORITIES)
    scen = [base, PI.vary(base, InterPodAffinity=0), PI.vary(base, InterPodAffinity=5), base, PI.vary(base, InterPodAffinity=0)]
    absent = [[], [], [], zones[0], zones[1]]
    g, refs, out = _sweep_and_check(inp, scen, absent=absent)
    assert g.has_affinity_terms() and len(cl.residents) > 0
    assert not np.array_equal(out[0], out[1])
    g.close()


def test_volume_instantiation():
    inp = PI.volume_input()
    preds, prios = inp.keys()
    scen = PI.scenarios_of(prios)
    g, refs, out = _sweep_and_check(inp, scen, explain=True)
    assert g.volumes is not None
    _check_records(refs, g.last_failures, len(inp.queue))
    assert any(r["hist"][:, list(V.VOLUME_REASONS)].any() for r in refs)
    g.close()


def test_outage_times_policy():
    inp, scen, _ = PI.full_refs(70)
    cl = inp.cluster()
    n = cl.n_nodes
    sets_ = [[], [0], [n - 1]] + [list(idx) for _, idx in scheduler.outage_sets(cl, PI.X.ZONE)][:2] + [list(range(n))]
    pick = [0, 1, 5, 7]
    pairs = [(scen[p], a) for a in sets_ for p in pick]
    g, refs, out = _sweep_and_check(inp, [p for p, _ in pairs], absent=[a for _, a in pairs], explain=True)
    _check_records(refs, g.last_failures, len(inp.queue))
    # the scenario that lists no node: every pod fails, listed 0, all-zero histograms
    last = len(pairs) - 1
    assert (out[last] == -1).all() and int(g.last_outcome["listed"][last]) == 0 and int(g.last_outcome["used"][last]) == 0
    assert not g.last_outcome["free_cpu"][last].any() and not g.last_outcome["free_mem"][last].any()
    assert int(g.last_failures["listed"][last]) == 0
    g.close()


def test_drain_prefix_under_policies():
    inp, scen, _ = PI.full_refs(70)
    cl = inp.cluster()
    sets_ = [("first", [0]), ("zone", list(scheduler.outage_sets(cl, PI.X.ZONE)[0][1])), ("none", [])]
    copies, requeue, queues = V.drain_plan(inp, sets_)
    dcl = inp.cluster(extra=copies)
    assert sum(len(r) for r in requeue) > 0
    pick = [0, 5, 7, 10]
    cases = [(scen[p], a, rq, q) for (_, a), rq, q in zip(sets_, requeue, queues) for p in pick]
    g = V.scheduler_of(inp, dcl)
    Q = len(inp.queue)
    out, pre, ctr, st = g.sweep_policy([c[0] for c in cases], absent=[c[1] for c in cases], requeue=[c[2] for c in cases],
                                       first=0, count=Q, explain=True, outcome=True)
    want = []
    for k, (pri, a, rq, q) in enumerate(cases):
        r = PI.oracle(inp, pri, a, queue=q + inp.queue)
        m = len(q)
        assert np.array_equal(pre[k], r["out"][:m]) and np.array_equal(out[k], r["out"][m:]), k
        assert int(ctr[k]) == r["counter"], k
        assert int(g.last_rehosted[k]) == int((r["out"][:m] >= 0).sum()), k
        assert int(g.last_scheduled[k]) == int((r["out"][m:] >= 0).sum()), k
        assert int(g.last_failures["count"][k]) == r["count"], k
        assert np.array_equal(g.last_failures["pod"][k, :r["count"]], r["pod"]), k
        assert np.array_equal(g.last_failures["hist"][k, :r["count"]], r["hist"]), k
        want.append(PI.outcome_of_answer(dcl, a, r["out"][m:], 0, rq, r["out"][:m]))
    _check_outcome(g.last_outcome, want)
    g.close()


# ---- 5. outcome records at the geometry's edges
@pytest.mark.parametrize("n", [1, 65])
def test_outcome_records_on_small_clusters(n):
    inp = V.geometry_input(n)
    preds, prios = inp.keys()
    scen = PI.map_scenarios(prios)
    absent = [[], [], [0], list(range(n))]
    g, refs, out = _sweep_and_check(inp, scen, absent=absent)
    assert int(g.last_outcome["listed"][3]) == 0 and not g.last_outcome["free_cpu"][3].any()
    assert int(g.last_outcome["listed"][0]) == n
    g.close()


# ---- 6. refusals
def test_a_weight_the_handle_lacks_is_refused():
    inp = PI.full_input(18)
    preds, prios = inp.keys()
    lean = [(nm, w) for nm, w in prios if nm not in ("SelectorSpreadPriority", "TaintTolerationPriority")]
    g = scheduler.GenericScheduler(inp.cluster(), preds, lean, collect_reasons=False)
    ok = [lean, PI.vary(lean, NodeAffinity=0)]
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_policy: scenario 1: SelectorSpreadPriority"):
        g.sweep_policy([lean, PI.vary(lean, SelectorSpread=1)])
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_policy: scenario 2: TaintTolerationPriority"):
        g.sweep_policy(ok + [PI.vary(lean, TaintToleration=2)])
    refs = [PI.oracle(inp, pri) for pri in ok]
    out, ctr, _ = g.sweep_policy(ok)  # the handle is as usable as before
    _check(refs, out, ctr, g)
    g.close()


def test_a_scenario_beyond_the_score_bits_is_refused():
    inp = PI.plain_input()
    g = V.scheduler_of(inp)
    wmax = (1 << abi.SWEEP_GENERAL_SCORE_BITS) // 10 - 1
    base = list(PI.DEFAULT_PRIORITIES)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep_policy: scenario 1: .*exceed 27 bits"):
        g.sweep_policy([base, PI.vary(base, LeastRequested=wmax)])
    with pytest.raises(Unsupported, match="scenario 0 is empty"):
        g.sweep_policy([[]])
    g.close()


def test_old_entries_still_refuse_what_they_refused():
    nodes, pods = synth.c2_objects(300, 40, seed=7)
    from ksim.ingest import Cluster
    cl = Cluster.from_objects(nodes, [], list(reversed(pods)))
    preds, prios = scheduler.provider("DefaultProvider")
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    for pri in ([("TaintTolerationPriority", 1), ("LeastRequestedPriority", 1)], [("LeastRequestedPriority", 1)]):
        with pytest.raises(abi.KsimUnsupported, match="ksim_sweep: .*would drop the handle's reduce priorities"):
            g.sweep([pri])
    g.close()
    g = scheduler.GenericScheduler(cl, preds, [("LeastRequestedPriority", 1)], collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="ksim_sweep: scenario 0: reduce priorities are not swept"):
        g.sweep([[("TaintTolerationPriority", 1), ("LeastRequestedPriority", 1)]])
    g.close()
    inp = PI.spread_input()
    lean = [("SelectorSpreadPriority", 1), ("LeastRequestedPriority", 1)]
    g = scheduler.GenericScheduler(inp.cluster(), ["GeneralPredicates"], lean, collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="would drop the handle's spread priority"):
        g.sweep([[("LeastRequestedPriority", 1)]], absent=[[0]])
    g.close()


# ---- 7. the simulator's level: ClusterCapacity.policy_what_if and the command line
def _snapshot():
    """workloads.rnd_workload (taints, preferred node affinity, selectors, ports): a snapshot as the
    simulator takes it, its pods in the order of the podspec list."""
    from workloads import rnd_workload
    return rnd_workload(11, n_nodes=40, n_pods=90)


def test_policy_what_if_matches_the_object_level_oracle():
    import ksim_ref as R
    nodes, running, pods = _snapshot()
    preds, prios = scheduler.provider("DefaultProvider")
    policies = [("default", list(prios)), ("no-taints", PI.vary(prios, TaintToleration=0)),
                ("affinity-x4", PI.vary(prios, NodeAffinity=4)), ("packing", PI.vary(prios, LeastRequested=0, MostRequested=2))]
    cc = scheduler.ClusterCapacity(nodes, running, pods, provider_name="DefaultProvider", collect_reasons=False)
    recs = cc.policy_what_if(policies, explain=True)
    assert [(r["policy"], r["name"], r["absent"]) for r in recs] == [(nm, None, 0) for nm, _ in policies]
    answers = set()
    for r, (_, pri) in zip(recs, policies):
        want, _ = R.simulate(nodes, running, pods, set(preds), pri)
        assert r["placements"] == [(pn, host) for pn, host, _ in want], r["policy"]
        assert r["fit_errors"] == [(pn, m) for pn, host, m in want if host is None] and r["explained"] == r["failed"]
        assert r["scheduled"] == sum(1 for _, host, _ in want if host is not None)
        placed = [(k, cc.cluster.index[host]) for k, (_, host, _) in enumerate(want) if host is not None]
        rec = PI.outcome_of(cc.cluster, (), placed)
        assert {k: r[k] for k in rec} == rec, r["policy"]
        answers.add(tuple(r["placements"]))
    assert len(answers) >= 3
    # outage x policy in one sweep, policy-major
    outages = scheduler.outage_sets(cc.cluster, "node")[:2]
    both = cc.policy_what_if(policies[:2], outages)
    assert [(r["policy"], r["name"]) for r in both] == [(p, o) for p, _ in policies[:2] for o, _ in outages]
    for r in both:
        pri = dict(policies)[r["policy"]]
        left = [x for x in nodes if x["metadata"]["name"] != r["name"]]
        stay = [x for x in running if x["spec"]["nodeName"] != r["name"]]
        want, _ = R.simulate(left, stay, pods, set(preds), pri)
        assert r["placements"] == [(pn, host) for pn, host, _ in want] and r["listed"] == len(nodes) - 1
    assert cc.policy_what_if([]) == [] and cc.policy_what_if(policies, []) == []


def test_cli_prints_one_line_per_policy_after_the_unchanged_report(tmp_path, capsys):
    import json

    import ksim_ref as R
    from ksim import cli
    nodes, _ = synth.c1_objects(6, 0, 0)
    spec = [{"name": "A", "num": 14, "pod": {"spec": {"containers": [  # a quarter of a node each
        {"name": "a", "resources": {"requests": {"cpu": "8", "memory": "32Gi"}}}]}}}]
    preds, prios = scheduler.provider("DefaultProvider")
    doc = [{"name": "default", "priorities": [{"name": nm, "weight": w} for nm, w in prios]},
           {"name": "packing", "priorities": [{"name": nm, "weight": w} for nm, w in PI.vary(prios, LeastRequested=0, MostRequested=1)]}]
    (tmp_path / "nodes.json").write_text(json.dumps(nodes))
    (tmp_path / "pod.json").write_text(json.dumps(spec))
    (tmp_path / "policies.json").write_text(json.dumps(doc))
    base = ["--podspec", str(tmp_path / "pod.json"), "--nodes", str(tmp_path / "nodes.json")]
    assert cli.main(base) == 0
    plain = capsys.readouterr().out
    assert cli.main(base + ["--what-if-policy", str(tmp_path / "policies.json")]) == 0
    got = capsys.readouterr().out
    assert got.startswith(plain) and "what-if" not in plain
    lines = got[len(plain):].splitlines()
    assert len(lines) == 2 and lines[0].startswith("what-if policy default: ") and lines[1].startswith("what-if policy packing: ")
    assert cli.main(base + ["--what-if-policy", str(tmp_path / "policies.json"), "--what-if-json"]) == 0
    recs = json.loads(capsys.readouterr().out[len(plain):])
    pods = scheduler.expand_simulation_pods(spec)
    for r, ent, line in zip(recs, doc, lines):
        pri = [(p["name"], p["weight"]) for p in ent["priorities"]]
        want, _ = R.simulate(nodes, [], pods, set(preds), pri)
        assert [tuple(x) for x in r["placements"]] == [(pn, host) for pn, host, _ in want]
        ok = sum(1 for _, host, _ in want if host is not None)
        assert line == "what-if policy %s: scheduled %d, failed %d, nodes used %d of %d, cpu nearly full %d, nearly empty %d" % (
            ent["name"], ok, len(want) - ok, r["used"], 6, sum(r["free_cpu"][:2]), sum(r["free_cpu"][9:]))
    assert recs[0]["used"] > recs[1]["used"]  # packing leaves nodes empty that spreading fills
    (tmp_path / "bad.json").write_text(json.dumps({"name": "x"}))
    assert cli.main(base + ["--what-if-policy", str(tmp_path / "bad.json")]) == 1
