"""GPU parity of the node-outage what-if (ksim_sweep_nodes, GenericScheduler.sweep(absent=...),
ClusterCapacity.what_if): scenario s with absent set A_s must equal the CPU oracle run on the
snapshot from which the nodes of A_s were left out — placements (as indices of the loaded table),
final lastNodeIndex and pods bound — in all three sweep forms."""
import copy
import functools

import numpy as np
import pytest

import cpu_ref
from ksim import abi, scheduler, synth

pytestmark = pytest.mark.gpu

SWEEP_FORMS = ["tree", "tree-chunked", "scan"]
POLICIES = [[("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)],
            [("MostRequestedPriority", 2), ("BalancedResourceAllocation", 1)]]
PREDS = list(scheduler.DEFAULT_PREDICATES)
STATE_KEYS = ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pod_count")


def _sweep_form(form, monkeypatch):
    """tree: one tree-mode wave per scenario (ksim_tree.hip); scan: the per-scenario scan kernel
    (ksim_sweep.hip); tree-chunked: scenarios in launches of 5."""
    if form == "scan":
        monkeypatch.setenv("KSIM_SWEEP_SCAN", "1")
    if form == "tree-chunked":
        monkeypatch.setenv("KSIM_SWEEP_CHUNK", "5")
    return abi.MODE_PERSISTENT if form == "scan" else abi.MODE_TREE


def _cluster(n, p):
    cpu, mem = synth.c3_nodes(n, 11)
    pcpu, pmem = synth.c3_pods(p, 11)
    return synth.resource_cluster(["s-%05d" % i for i in range(n)], cpu, mem, np.full(n, 30, np.int32), pcpu, pmem)


def _reduced(cl, keep):
    """The cluster without the nodes outside `keep` (sliced the way Cluster.shard slices)."""
    sub = copy.copy(cl)
    sub.cols = {k: (np.ascontiguousarray(v[..., keep]) if isinstance(v, np.ndarray) else v) for k, v in cl.cols.items()}
    sub.names = [cl.names[i] for i in np.nonzero(keep)[0]]
    sub.index = {}
    return sub


def _oracle(cl, cfg, absent, first, count, state=None, counter=0):
    """cpu_ref on the reduced cluster, its node indices mapped back to the loaded table.  Without
    any node left the reference returns ErrNoNodesAvailable for every pod: nothing bound, counter
    unchanged."""
    n = cl.n_nodes
    keep = np.ones(n, bool)
    keep[list(absent)] = False
    if not keep.any():
        return np.full(count, -1, np.int32), counter
    sub = _reduced(cl, keep)
    if state is not None:
        state = {k: np.ascontiguousarray(v[..., keep]) for k, v in state.items()}
    ref, _, _, ctr = cpu_ref.run(sub, cfg, first, count, threads=8, state=state, counter=counter)
    back = np.nonzero(keep)[0].astype(np.int32)
    return np.where(ref >= 0, back[np.maximum(ref, 0)], -1).astype(np.int32), ctr


def _node_sets(n, first_ten):
    """(label, absent set) of the what-ifs every parity case runs."""
    rng = np.random.default_rng(20240611)
    sets_ = [("none", []), ("first", [0]), ("last", [n - 1]), ("word-edge", [31, 32])]
    if n > 1024:
        sets_.append(("1023-1024", [1023, 1024]))
    sets_.append(("random-10pct", sorted(int(x) for x in rng.choice(n, n // 10, replace=False))))
    sets_.append(("first-ten-pods", sorted(set(int(x) for x in first_ten if x >= 0))))
    sets_.append(("all-but-7", [i for i in range(n) if i != 7]))
    if n > 900:
        sets_.append(("all-but-7-900", [i for i in range(n) if i not in (7, 900)]))
    sets_.append(("every-node", list(range(n))))
    return sets_


@functools.lru_cache(maxsize=None)
def _parity_case():
    """n = 1500 (1500 % 32 = 28: a ragged last word; two-row segments in the scan form's select
    phase; a two-level tree), 1200 pods: the scenario list and the oracle's answers, once."""
    n, p = 1500, 1200
    cl = _cluster(n, p)
    plain, _, _, _ = cpu_ref.run(cl, scheduler.make_config(PREDS, POLICIES[0]), 0, p, threads=8)
    scen = [(label, a, pri) for label, a in _node_sets(n, plain[:10]) for pri in POLICIES]
    refs = [_oracle(cl, scheduler.make_config(PREDS, pri), a, 0, p) for _, a, pri in scen]
    return cl, scen, refs, plain


def _check(scen, refs, out, ctr, bound, n):
    for k, ((label, a, pri), (ref, ref_ctr)) in enumerate(zip(scen, refs)):
        assert np.array_equal(out[k], ref), (label, pri)
        assert int(ctr[k]) == ref_ctr, (label, pri)
        assert not np.isin(out[k][out[k] >= 0], a).any(), (label, pri)
        assert int(bound[k]) == int((ref >= 0).sum()), (label, pri)


@pytest.mark.parametrize("form", SWEEP_FORMS)
def test_absent_sets_match_oracle_on_the_reduced_cluster(form, monkeypatch):
    mode = _sweep_form(form, monkeypatch)
    cl, scen, refs, plain = _parity_case()
    n, p = cl.n_nodes, len(cl.pods)
    g = scheduler.GenericScheduler(cl, PREDS, POLICIES[0], collect_reasons=False)
    before = g.node_state()
    out, ctr, st = g.sweep([pri for _, _, pri in scen], 0, p, absent=[a for _, a, _ in scen])
    assert st.mode == mode
    assert st.node_evals == len(scen) * p * n
    _check(scen, refs, out, ctr, g.last_scheduled, n)
    for k, (label, a, pri) in enumerate(scen):
        if label == "none" and pri == POLICIES[0]:
            assert np.array_equal(out[k], plain)
        elif label != "none":  # every node set changes the outcome
            assert not np.array_equal(out[k], refs[0 if pri == POLICIES[0] else 1][0]), (label, pri)
        if label == "all-but-7":  # one listed node: never more than one fit, lastNodeIndex stays
            assert int(ctr[k]) == 0 and set(out[k].tolist()) <= {7, -1} and (out[k] == 7).any()
        if label == "every-node":
            assert (out[k] == -1).all() and int(ctr[k]) == 0 and int(g.last_scheduled[k]) == 0
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    g.close()


@pytest.mark.parametrize("form", SWEEP_FORMS)
def test_absent_sets_overflow_and_mid_queue_start(form, monkeypatch):
    """A queue that overflows a 64-node cluster, swept from pod 500 after a regular schedule() of the
    prefix: absent nodes that already hold prefix pods take those pods with them."""
    _sweep_form(form, monkeypatch)
    n, p = 64, 3000
    cl = _cluster(n, p)
    base = POLICIES[0]
    pre, _, state0, ctr0 = cpu_ref.run(cl, scheduler.make_config(PREDS, base), 0, 500, threads=4)
    sets_ = _node_sets(n, pre[:10])
    held = dict(sets_)["first-ten-pods"]
    # absent nodes that hold prefix pods
    assert len(held) > 0 and (np.bincount(pre[pre >= 0], minlength=n)[held] > 0).all()
    scen = [(label, a, pri) for label, a in sets_ for pri in POLICIES]
    g = scheduler.GenericScheduler(cl, PREDS, base, collect_reasons=False)
    got_pre, _, _ = g.schedule(0, 500)
    assert np.array_equal(got_pre, pre)
    out, ctr, _ = g.sweep([pri for _, _, pri in scen], 500, 2500, absent=[a for _, a, _ in scen])
    refs = [_oracle(cl, scheduler.make_config(PREDS, pri), a, 500, 2500,
                    state={k: v.copy() for k, v in state0.items()}, counter=ctr0) for _, a, pri in scen]
    _check(scen, refs, out, ctr, g.last_scheduled, n)
    assert (out < 0).any(axis=1).all()  # the cluster fills up in every scenario
    assert g.last_node_index == ctr0
    st = g.node_state()
    for key in STATE_KEYS:
        assert np.array_equal(st[key], state0[key]), key
    g.close()


@functools.lru_cache(maxsize=None)
def _ragged_case(n, p):
    cl = _cluster(n, p)
    scen = [("none", [], POLICIES[0]), ("last", [n - 1], POLICIES[0]), ("every-third", list(range(0, n, 3)), POLICIES[0])]
    refs = [_oracle(cl, scheduler.make_config(PREDS, pri), a, 0, p) for _, a, pri in scen]
    return cl, scen, refs


@pytest.mark.parametrize("form", SWEEP_FORMS)
@pytest.mark.parametrize("n,p", [(2051, 600), (20_000, 300)])
def test_absent_sets_ragged_tail_and_deeper_tree(n, p, form, monkeypatch):
    """n = 2051 = 64 * 32 + 3 (three bits in the last word); n = 20 000: a three-level tree."""
    mode = _sweep_form(form, monkeypatch)
    cl, scen, refs = _ragged_case(n, p)
    g = scheduler.GenericScheduler(cl, PREDS, POLICIES[0], collect_reasons=False)
    out, ctr, st = g.sweep([pri for _, _, pri in scen], 0, p, absent=[a for _, a, _ in scen])
    assert st.mode == mode
    _check(scen, refs, out, ctr, g.last_scheduled, n)
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[0], out[2])
    g.close()


SCAN_MAX_NODES = 76_800  # KSIM_SWEEP_MAX_NODES: one uint16 evaluation per node in 150 KiB of dynamic LDS


def test_scan_form_at_its_node_cap(monkeypatch):
    """76,800 nodes: 150 KiB of dynamic LDS per workgroup, 75-row select segments."""
    assert SCAN_MAX_NODES * 2 == 150 * 1024
    monkeypatch.setenv("KSIM_SWEEP_SCAN", "1")
    cl, scen, refs = _ragged_case(SCAN_MAX_NODES, 300)
    g = scheduler.GenericScheduler(cl, PREDS, POLICIES[0], collect_reasons=False)
    before = g.node_state()
    out, ctr, st = g.sweep([pri for _, _, pri in scen], 0, len(cl.pods), absent=[a for _, a, _ in scen])
    assert st.mode == abi.MODE_PERSISTENT
    assert st.kernel_launches == 1 and st.blocks == len(scen) == 3
    _check(scen, refs, out, ctr, g.last_scheduled, cl.n_nodes)
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[0], out[2])
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    g.close()


@pytest.mark.parametrize("form", ["tree", "scan"])
def test_one_node_beyond_the_cap_is_refused(form, monkeypatch):
    _sweep_form(form, monkeypatch)
    cl = _cluster(SCAN_MAX_NODES + 1, 20)
    g = scheduler.GenericScheduler(cl, PREDS, POLICIES[0], collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported, match="76800"):
        g.sweep(POLICIES, 0, 20, absent=[[], [0]])
    with pytest.raises(abi.KsimUnsupported, match="76800"):
        g.sweep(POLICIES, 0, 20)
    assert g.last_node_index == 0
    g.close()


@pytest.mark.parametrize("form", SWEEP_FORMS)
def test_empty_sets_equal_the_plain_sweep(form, monkeypatch):
    _sweep_form(form, monkeypatch)
    cl, _, _, _ = _parity_case()
    pick = POLICIES + [[("LeastRequestedPriority", 3)]]
    g = scheduler.GenericScheduler(cl, PREDS, POLICIES[0], collect_reasons=False)
    o1, c1, _ = g.sweep(pick, 0, 400)
    o2, c2, _ = g.sweep(pick, 0, 400, absent=[[]] * len(pick))
    o3, c3, _ = g.sweep(pick, 0, 400, absent=[np.zeros(cl.n_nodes, bool)] * len(pick))
    assert np.array_equal(o1, o2) and np.array_equal(c1, c2)
    assert np.array_equal(o1, o3) and np.array_equal(c1, c3)
    assert g.last_scheduled.tolist() == (o1 >= 0).sum(axis=1).tolist()
    g.close()


@pytest.mark.parametrize("form", SWEEP_FORMS)
def test_own_policy_of_a_default_provider_scheduler(form, monkeypatch):
    """scenarios=None runs every scenario under the scheduler's own configured weights (weights =
    NULL).  DefaultProvider carries reduce priorities, which the plain sweep refuses as scenario
    weights; for resource-only pods they are one value on every node, so the result is the
    oracle's under the whole provider, and the same as sweeping the provider's map priorities."""
    _sweep_form(form, monkeypatch)
    n, p = 300, 500
    cl = _cluster(n, p)
    preds, prios = scheduler.provider("DefaultProvider")
    g = scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False)
    with pytest.raises(abi.KsimUnsupported):
        g.sweep([prios], 0, p)
    sets_ = [[], [0], list(range(0, n, 2)), [31, 32, 299]]
    out, ctr, _ = g.sweep(None, 0, p, absent=sets_)
    cfg = scheduler.make_config(preds, prios)
    for k, a in enumerate(sets_):
        ref, ref_ctr = _oracle(cl, cfg, a, 0, p)
        assert np.array_equal(out[k], ref), a
        assert int(ctr[k]) == ref_ctr, a
    maps = [(nm, w) for nm, w in prios if nm in ("LeastRequestedPriority", "MostRequestedPriority",
                                                 "BalancedResourceAllocation")]
    o2, c2, _ = g.sweep([maps] * len(sets_), 0, p, absent=sets_)
    assert np.array_equal(out, o2) and np.array_equal(ctr, c2)
    g.close()


def test_scan_form_runs_in_scenario_chunks(monkeypatch):
    monkeypatch.setenv("KSIM_SWEEP_SCAN", "1")
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "5")
    cl, scen, refs, _ = _parity_case()
    scen, refs = scen[2:14], refs[2:14]  # twelve scenarios with a node set: launches of 5, 5 and 2
    g = scheduler.GenericScheduler(cl, PREDS, POLICIES[0], collect_reasons=False)
    out, ctr, st = g.sweep([pri for _, _, pri in scen], 0, len(cl.pods), absent=[a for _, a, _ in scen])
    assert st.mode == abi.MODE_PERSISTENT
    assert st.kernel_launches == 3
    _check(scen, refs, out, ctr, g.last_scheduled, cl.n_nodes)
    g.close()


def test_cluster_capacity_what_if_matches_the_object_level_oracle():
    """ClusterCapacity.what_if under DefaultProvider against ksim_ref.simulate on the object lists
    with the outage's node removed."""
    import ksim_ref as R
    nodes, pods = synth.c1_objects(64, 200, 5)
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
        assert r["failed"] == sum(1 for _, host, _ in want if host is None)
        assert all(host != name for _, host in r["placements"])
    # node names work as well as indices
    again = cc.what_if([(nm, [nm]) for nm, _ in outages[:1]])
    assert again[0]["placements"] == recs[0]["placements"]


def test_cli_prints_the_what_ifs_after_the_unchanged_report(tmp_path, capsys):
    """--what-if-outage: the normal report byte for byte, then one line per outage (or the records
    as JSON); the lines agree with the object-level oracle on the snapshot without that zone."""
    import json

    import ksim_ref as R
    from ksim import cli
    zone = "failure-domain.beta.kubernetes.io/zone"
    nodes, _ = synth.c1_objects(6, 0, 0)
    for i, x in enumerate(nodes):
        x["metadata"]["labels"] = {zone: "z%d" % (i % 3)}
    spec = [{"name": "A", "num": 150, "pod": {"spec": {"containers": [
        {"name": "a", "resources": {"requests": {"cpu": "1", "memory": "1Gi"}}}]}}}]
    (tmp_path / "nodes.json").write_text(json.dumps(nodes))
    (tmp_path / "pod.json").write_text(json.dumps(spec))
    base = ["--podspec", str(tmp_path / "pod.json"), "--nodes", str(tmp_path / "nodes.json")]
    assert cli.main(base) == 0
    plain = capsys.readouterr().out
    assert cli.main(base + ["--what-if-outage", zone]) == 0
    got = capsys.readouterr().out
    assert got.startswith(plain) and "what-if" not in plain
    preds, prios = scheduler.provider("DefaultProvider")
    pods = scheduler.expand_simulation_pods(spec)
    want, nums = [], []
    for z in ("z0", "z1", "z2"):
        left = [x for x in nodes if x["metadata"]["labels"][zone] != z]
        res, _ = R.simulate(left, [], pods, set(preds), prios)
        ok = sum(1 for _, host, _ in res if host is not None)
        nums.append((z, 2, ok, len(res) - ok))
        want.append("what-if outage %s: nodes removed %d, scheduled %d, failed %d" % nums[-1])
    assert got[len(plain):].splitlines() == want
    assert all(failed > 0 for _, _, _, failed in nums)  # four nodes of 32 cpus do not hold 150 one-cpu pods
    assert cli.main(base + ["--what-if-outage", zone, "--what-if-json"]) == 0
    recs = json.loads(capsys.readouterr().out[len(plain):])
    assert [(r["name"], r["absent"], r["scheduled"], r["failed"]) for r in recs] == nums
    assert all(len(r["placements"]) == 150 for r in recs)
