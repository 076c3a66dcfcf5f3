"""CPU-only tests of the policy sweep (ksim_sweep_policy, include/ksim_polsweep.h): the properties of
the inputs and scenario lists that tests/test_gpu_sweep_policy.py sweeps, pinned for the reference alone
so that the GPU cases cannot pass vacuously, and the weight rules — the Python scenario builder
(scheduler.policy_rows) and the C entry's pre-device check (csrc/ksim_polsweep_rules.h, compiled into a
stand-alone program: the entry itself needs a handle, and a handle needs a device)."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import policy_sweep_inputs as PI
from ksim import abi, scheduler
from ksim.ingest import Cluster, Unsupported
from workloads import add_prefer_avoid, rnd_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "c", "polsweep_rules_check.cpp")
SIZES = [n for n, _ in PI.RND_SIZES]


# ---- the scenario list
def test_scenarios_are_eight_to_twelve_around_the_default_provider():
    scen = PI.scenarios_of()
    assert 8 <= len(scen) <= 12 and scen[0] == list(PI.DEFAULT_PRIORITIES)
    assert len({tuple(sorted(s)) for s in scen}) == len(scen)
    for s in scen:  # NodePreferAvoidPods, the addend priority, stays as the provider has it
        assert PI.weights_of(s)["NodePreferAvoidPodsPriority"] == 10000


@pytest.mark.parametrize("name", PI.RESTRICTED)
def test_pairs_differ_in_their_weight_alone_and_one_side_of_the_first_is_zero(name):
    scen = PI.scenarios_of()
    for a, b in PI.PAIRS[name]:
        assert PI.differ_only_in(scen[a], scen[b]) == {name}
    a, b = PI.PAIRS[name][0]
    assert 0 in (PI.weights_of(scen[a]).get(name, 0), PI.weights_of(scen[b]).get(name, 0))
    a, b = PI.PAIRS[name][1]
    assert PI.weights_of(scen[a]).get(name, 0) and PI.weights_of(scen[b]).get(name, 0)


def test_map_pair_differs_in_a_map_weight_alone():
    scen = PI.scenarios_of()
    a, b = PI.MAP_PAIR
    d = PI.differ_only_in(scen[a], scen[b])
    assert d and d <= set(PI.MAP)


# ---- the full workload under the reference alone
@pytest.mark.parametrize("n", SIZES)
def test_full_workload_meets_the_conditions_for_the_reference_alone(n):
    inp, scen, refs = PI.full_refs(n)
    c = PI.conditions(inp, scen, refs)
    for name in PI.RESTRICTED:  # dropping the priority moves a pod
        assert c["pair"][name][0], (name, c)
    assert c["map_pair"]
    assert c["failures"] > 0
    assert len(c["buckets"]) >= 3 and c["bucket0_overcommit"]
    assert PI.holds(c)


@pytest.mark.parametrize("n", SIZES)
def test_seed_is_the_first_that_holds(n):
    for seed in range(PI.SEEDS[n]):
        inp, scen, refs = PI.full_refs(n, seed)
        assert not PI.holds(PI.conditions(inp, scen, refs))


def test_full_workload_loads_everything_the_provider_reads():
    inp = PI.full_input(18)
    cl = inp.cluster()
    preds, prios = inp.keys()
    pl = scheduler.plan(cl, preds, prios)
    assert cl.spread_active and pl.affinity is not None
    assert pl.affinity["n_terms"] or pl.affinity["n_carries"]  # inter-pod terms: the IPA instantiations
    assert pl.cfg.weights[abi.W_SPREAD] == 1 and pl.cfg.weights[abi.W_INTERPOD] == 1
    assert PI.X.max_reduce_classes(cl) > 1
    big = PI.full_input(1030).cluster()
    assert big.n_nodes == 1030 and big.n_nodes > 1024 and big.n_nodes % 256 and big.n_nodes % 64


def test_every_scenario_fails_the_huge_pod_on_every_listed_node():
    inp, scen, refs = PI.full_refs(18)
    k = [x["metadata"]["name"] for x in inp.queue].index("pod-huge")
    for r in refs:
        assert r["out"][k] == -1
        h = r["hist"][list(r["pod"]).index(k)]
        assert h[abi.R_CPU] > 0


def test_outcome_recount_is_consistent():
    inp, scen, refs = PI.full_refs(70)
    cl = inp.cluster()
    for r in refs[:3]:
        rec = PI.outcome_of_answer(cl, (), r["out"])
        assert rec["listed"] == cl.n_nodes and sum(rec["free_cpu"]) == sum(rec["free_mem"]) == cl.n_nodes
        assert 0 < rec["used"] <= cl.n_nodes
    rec = PI.outcome_of(cl, range(cl.n_nodes), [])
    assert rec == dict(listed=0, used=0, free_cpu=[0] * 11, free_mem=[0] * 11)
    assert [PI.least(r, c) for r, c in ((0, 0), (5, 4), (4, 4), (0, 4), (1, 4), (3, 1000))] == [0, 0, 0, 10, 7, 9]


# ---- each instantiation's input
def test_instantiation_inputs_are_what_they_claim():
    preds, prios = PI.DEFAULT_PREDICATES, PI.DEFAULT_PRIORITIES
    plain = PI.plain_input()
    pl = scheduler.plan(plain.cluster(), preds, prios)
    assert pl.affinity is None and pl.volumes is None
    w = pl.cfg.weights
    k1 = max(int(pl.tables["n_tt"][c]) for c in np.unique(pl.pods["cls"]))
    k2 = max(int(pl.tables["n_na"][c]) for c in np.unique(pl.pods["cls"]))
    assert w[abi.W_TAINT_TOL] and w[abi.W_NODE_AFF] and k1 > 1 and k2 > 1 and PI.X.max_reduce_classes(plain.cluster()) <= abi.MAX_RCLASS
    spr = scheduler.plan(PI.spread_input().cluster(), preds, prios)
    assert spr.affinity is not None and not (spr.affinity["n_terms"] or spr.affinity["n_carry"] or spr.affinity["n_carries"])
    anti = PI.anti_input()
    ap = scheduler.plan(anti.cluster(), preds, prios)
    assert ap.affinity["n_terms"] and len(anti.cluster().residents) == 12
    vol = PI.volume_input()
    vp = scheduler.plan(vol.cluster(), *vol.keys())
    assert vp.volumes is not None


@pytest.mark.parametrize("which", ["plain_input", "spread_input", "anti_input", "volume_input"])
def test_instantiation_inputs_move_under_the_scenarios(which):
    inp = getattr(PI, which)()
    scen = PI.scenarios_of(inp.keys()[1])
    outs = {PI.oracle(inp, pri)["out"].tobytes() for pri in scen}
    assert len(outs) >= 2


# ---- the Python scenario builder
def _rows(inp, scenarios, **kw):
    preds, prios = inp.keys()
    return scheduler.policy_rows(inp.cluster(), preds, prios, scenarios, **kw)


def test_rows_follow_the_slots_and_the_spread_flag():
    inp = PI.full_input(18)
    scen = PI.scenarios_of()
    w = _rows(inp, scen)
    assert w.shape == (len(scen), abi.NW) and w.dtype == np.int64
    assert list(w[0]) == [1, 0, 1, 1, 1, 1, 1]
    assert w[1][abi.W_TAINT_TOL] == 0 and w[2][abi.W_TAINT_TOL] == 3
    assert w[3][abi.W_NODE_AFF] == 0 and w[4][abi.W_NODE_AFF] == 4
    assert w[5][abi.W_SPREAD] == 0 and w[6][abi.W_SPREAD] == 3
    assert w[7][abi.W_INTERPOD] == 0 and w[8][abi.W_INTERPOD] == 2
    assert w[9][abi.W_BALANCED] == 0 and list(w[10][:2]) == [0, 2]
    # without spread selectors SelectorSpreadPriority is a constant: no weight in its slot
    plain = PI.plain_input()
    assert not plain.cluster().spread_active and _rows(plain, scen)[6][abi.W_SPREAD] == 0


def test_rows_refuse_an_empty_scenario_and_unknown_keys():
    inp = PI.full_input(18)
    with pytest.raises(Unsupported, match="scenario 1 is empty"):
        _rows(inp, [list(PI.DEFAULT_PRIORITIES), []])
    with pytest.raises(Unsupported, match="outside the supported key set"):
        _rows(inp, [[("NoSuchPriority", 1)]])
    with pytest.raises(abi.KsimError):
        _rows(inp, [[("LeastRequestedPriority", 0)]])


def test_constants_may_differ_where_nothing_is_folded():
    inp = PI.full_input(18)
    preds, prios = inp.keys()
    assert scheduler.plan(inp.cluster(), preds, prios).na_add is None
    w = _rows(inp, [[("LeastRequestedPriority", 1)], [("LeastRequestedPriority", 1), ("NodePreferAvoidPodsPriority", 7)],
                    [("LeastRequestedPriority", 1), ("EqualPriority", 3), ("ImageLocalityPriority", 2)]])
    assert [list(r) for r in w] == [[1, 0, 0, 0, 0, 0, 0]] * 3


def test_folded_addends_must_be_named_at_the_schedulers_weight():
    nodes, running, pods = rnd_workload(5, n_nodes=24, n_pods=60)
    nodes, pods = add_prefer_avoid(5, copy.deepcopy(nodes), copy.deepcopy(pods))
    cl = Cluster.from_objects(nodes, running, list(reversed(pods)))
    preds, prios = scheduler.provider("DefaultProvider")
    na_add = scheduler.plan(cl, preds, prios).na_add
    assert na_add is not None  # NodePreferAvoidPods differs across the nodes: folded
    rows = lambda sc, add=na_add: scheduler.policy_rows(cl, preds, prios, sc, None, add)
    assert list(rows([PI.vary(prios, TaintToleration=0)])[0]) == [1, 0, 1, 0, 1, 1, 0]
    with pytest.raises(Unsupported, match="scenario 1: .*NodePreferAvoidPodsPriority"):
        rows([prios, [(n, w) for n, w in prios if n != "NodePreferAvoidPodsPriority"]])
    with pytest.raises(Unsupported, match="scenario 0"):
        rows([[(n, 5 if n == "NodePreferAvoidPodsPriority" else w) for n, w in prios]])
    # a scheduler without the priority loaded no addends: a scenario cannot add it here either
    lean = [(n, w) for n, w in prios if n != "NodePreferAvoidPodsPriority"]
    assert scheduler.plan(cl, preds, lean).na_add is None
    with pytest.raises(Unsupported, match="scenario 0"):
        scheduler.policy_rows(cl, preds, lean, [prios], None, None)
    assert len(scheduler.policy_rows(cl, preds, lean, [lean, PI.vary(lean, NodeAffinity=0)], None, None)) == 2


# ---- the C entry's weight rules
def test_weight_rules_under_the_system_compiler(tmp_path):
    exe = tmp_path / "polsweep_rules_check"
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, PROGRAM, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_rules_header_needs_no_device_header_and_the_entry_checks_before_the_device():
    src = open(os.path.join(CSRC, "ksim_polsweep_rules.h")).read()
    assert not re.search(r'#include\s*[<"](hip/|ksim_)', src)
    rt = open(os.path.join(CSRC, "ksim_sweep_rt.cpp")).read()
    body = rt[rt.index("int ksim_sweep_policy("):]
    assert body.index("ksim_policy_weight_rules(") < body.index("hipSetDevice")


def test_abi_names_the_entry_beside_the_unchanged_function_list():
    assert "ksim_sweep_policy" not in abi.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "ksim_polsweep.h")).read()
    assert "int ksim_sweep_policy(" in hdr and "KSIM_OUTCOME_BUCKETS 11" in hdr
    assert abi.OUTCOME_BUCKETS == 11 and [f for f, _ in abi.SweepOutcome._fields_] == ["listed", "used", "free_cpu", "free_mem"]
    assert hasattr(abi.lib(), "ksim_sweep_policy")


# ---- the command line
def test_cli_accepts_the_policy_flag_and_reads_the_policy_files_shape(tmp_path):
    import json

    from ksim import cli
    a = cli.parse_args(["--podspec", "pod.yaml", "--nodes", "nodes.json", "--what-if-policy", "p.json", "--what-if-json"])
    assert a.what_if_policy == "p.json" and a.what_if_json is True
    assert not hasattr(cli.parse_args(["--podspec", "pod.yaml", "--nodes", "nodes.json"]), "what_if_policy")
    f = tmp_path / "p.json"
    f.write_text(json.dumps([{"name": "spread-x3", "priorities": [{"name": "SelectorSpreadPriority", "weight": 3},
                                                                  {"name": "LeastRequestedPriority", "weight": 1}]},
                             {"priorities": [{"name": "MostRequestedPriority", "weight": 2}]}]))
    assert cli.load_policies(str(f)) == [("spread-x3", [("SelectorSpreadPriority", 3), ("LeastRequestedPriority", 1)]),
                                         ("policy-1", [("MostRequestedPriority", 2)])]
    for bad in ({"name": "x"}, [{"name": "x"}], [{"name": "x", "priorities": [{"name": "a"}]}],
                [{"name": "x", "priorities": [{"name": "a", "weight": 1, "argument": {"labelPreference": {}}}]}]):
        f.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            cli.load_policies(str(f))
