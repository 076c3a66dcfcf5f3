"""GPU parity of the scenario sweep's general form (ksim_sweep_general_kernel) where its header,
DESIGN.md §3 and the README make promises that tests/test_gpu_sweep_general.py does not reach: the
38,400-node cap (150 KiB of dynamic LDS), degenerate segment / wave geometries, ties over every
wave and segment position, lastNodeIndex beyond 2^32, exactly KSIM_MAX_RCLASS reduce classes, two
classes that both win, the top of the 27 score bits, the port-slot overflow return and the
documented refusals.  Every scenario is compared bit for bit with the C oracle on the cluster
reduced to the scenario's nodes, the way tests/test_gpu_sweep_general.py does it."""
import functools

import numpy as np
import pytest

import cpu_ref
from ksim import abi, ingest, scheduler, synth
from test_gpu_sweep_general import PREDS, _c2_cluster, _check, _oracle
from workloads import sixteen_class_workload, uniform_selector_workload

pytestmark = pytest.mark.gpu


def _sweep_and_check(g, cl, sets_, refs, scenarios=None, first=0, count=None, counter=0):
    """One sweep of the absent sets against the oracle's answers: placements, final counters, pods
    bound, no absent node chosen, the general form, the handle's state untouched.  Returns the
    placements and counters."""
    count = len(cl.pods) - first if count is None else count
    before = g.node_state()
    out, ctr, st = g.sweep(scenarios, first, count, absent=[a for _, a in sets_])
    assert st.mode == abi.MODE_PERSISTENT
    _check(sets_, refs, out, ctr, g.last_scheduled)
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == counter
    return out, ctr, st


def _default(cl, counter=0):
    """(plan, oracle config) of the cluster's queue under DefaultProvider."""
    preds, prios = scheduler.provider("DefaultProvider")
    return scheduler.plan(cl, preds, prios, last_node_index=counter), scheduler.make_config(preds, prios)


def _default_scheduler(cl, counter=0):
    preds, prios = scheduler.provider("DefaultProvider")
    return scheduler.GenericScheduler(cl, preds, prios, collect_reasons=False, last_node_index=counter)


def _random_tenth(n):
    rng = np.random.default_rng(20240611)
    return sorted(int(x) for x in rng.choice(n, n // 10, replace=False))


# ---- 1. segment and wave geometry: KS = ceil(n / 1024) rows a thread, threads with seg0 > n, waves without rows
GEOMETRY_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def _geometry_case(n):
    cl = _c2_cluster(n, 1200 if n >= 1023 else max(60, 40 * n), 2)
    sets_ = [("none", []), ("first", [0]), ("last", [n - 1]), ("every-node", list(range(n)))]
    if n > 32:
        sets_.append(("word-edge", [31, 32]))
    if n > 1024:
        sets_.append(("1023-1024", [1023, 1024]))
    sets_.append(("random-10pct", _random_tenth(n)))
    pl, cfg = _default(cl)
    refs = [_oracle(cl, pl, cfg, a, 0, len(cl.pods)) for _, a in sets_]
    return cl, sets_, refs


@pytest.mark.parametrize("n", GEOMETRY_N)
def test_segment_and_wave_geometry(n):
    cl, sets_, refs = _geometry_case(n)
    assert int((cl.pods["port_cnt"] > 0).sum()) >= 13  # host-port pods: the general form
    if n <= 65:
        assert (refs[0][0] < 0).any() and (refs[0][0] >= 0).any()  # the small clusters fill up
    g = _default_scheduler(cl)
    out, ctr, st = _sweep_and_check(g, cl, sets_, refs)
    assert st.kernel_launches == 1 and st.blocks == len(sets_)
    k = [label for label, _ in sets_].index("every-node")
    assert (out[k] == -1).all() and int(ctr[k]) == 0 and int(g.last_scheduled[k]) == 0
    if n == 1:
        assert (ctr == 0).all()  # never more than one fit node: lastNodeIndex stays
    g.close()


# ---- 2. ties across every wave and segment position, lastNodeIndex below and beyond 2^32
@functools.lru_cache(maxsize=None)
def _ties_case(n, counter):
    nodes, pods = uniform_selector_workload(n, 2 * n + 7)
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    sets_ = [("none", []), ("second", [1]), ("last-but-one", [n - 2]), ("1023-1024", [1023, 1024]),
             ("every-second", list(range(0, n, 2))), ("decoy", [n // 2])]
    pl, cfg = _default(cl, counter)
    refs = [_oracle(cl, pl, cfg, a, 0, len(cl.pods), counter=counter) for _, a in sets_]
    return cl, sets_, refs


@pytest.mark.parametrize("counter", [0, 2**32 - 5], ids=["from-0", "across-2^32"])
@pytest.mark.parametrize("n", [1027, 2051])
def test_ties_land_in_every_wave_and_segment_position(n, counter):
    """C, the nodes at the best total, starts at the n - 3 fit nodes and shrinks by one per pod, so
    lastNodeIndex % C walks through every wave and every position of the two- or three-row
    segments (the last one ragged); from 2^32 - 5 the counter crosses 2^32 after five pods."""
    cl, sets_, refs = _ties_case(n, counter)
    p = len(cl.pods)
    assert (cl.pods["flags"] & abi.POD_NEED_SELECTOR).all()
    g = _default_scheduler(cl, counter)
    assert g.last_node_index == counter
    out, ctr, _ = _sweep_and_check(g, cl, sets_, refs, counter=counter)
    assert int(ctr[0]) == counter + p  # past 2^32 in the second case
    m = n - 3
    rest = np.setdiff1d(np.arange(n), [0, n // 2, n - 1])
    assert np.array_equal(np.sort(out[0][:m]), rest) and np.array_equal(np.sort(out[0][m:2 * m]), rest)
    k = [label for label, _ in sets_].index("decoy")
    assert np.array_equal(out[k], out[0]) and int(ctr[k]) == int(ctr[0])  # a node no pod fits changes nothing
    for k in range(1, len(sets_) - 1):
        assert not np.array_equal(out[k], out[0]), sets_[k][0]
    g.close()


# ---- 3. two reduce classes that both win, ties inside a class that spans waves
def test_two_classes_win_one_after_the_other():
    n = 1027
    nodes, pods = uniform_selector_workload(n, 4115, taint_every=2, cpu="2", mem="4Gi")
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    sets_ = [("none", []), ("untainted", list(range(0, n, 2))), ("tainted", list(range(1, n, 2)))]
    pl, cfg = _default(cl)
    assert ((np.asarray(pl.tables["n_tt"]) * np.asarray(pl.tables["n_na"]))[cl.pods["cls"]] == 2).all()
    refs = [_oracle(cl, pl, cfg, a, 0, len(cl.pods)) for _, a in sets_]
    g = _default_scheduler(cl)
    out, _, _ = _sweep_and_check(g, cl, sets_, refs)
    bound = out[0][out[0] >= 0]
    assert len(bound) == 4096 and (out[0][-19:] == -1).all()
    assert int((bound % 2 == 1).sum()) == 2048 and int((bound % 2 == 0).sum()) == 2048  # both classes receive pods
    assert (out[1][out[1] >= 0] % 2 == 1).all() and (out[2][out[2] >= 0] % 2 == 0).all()
    g.close()


# ---- 4. exactly KSIM_MAX_RCLASS reduce classes, and the refusal beyond
def test_sixteen_reduce_classes():
    """4 x 4 classes (lane & 15 and the packed word's low four bits full).  TaintToleration and
    NodeAffinity pull in opposite directions, so several classes hold the best total at once for
    most pods (tests/test_sweep_general_host.py counts them): win masks with more than one bit."""
    nodes, pods = sixteen_class_workload(203, 4)
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    n = cl.n_nodes
    sets_ = [("none", []), ("first", [0]), ("last", [n - 1]),
             ("one-pair", [i for i in range(n) if i % 4 == 1 and (i // 4) % 4 == 2]),  # one taint, tier t2: class 6
             ("class-15", [i for i in range(n) if i % 4 == 3 and (i // 4) % 4 == 3]),  # three taints, tier t3
             ("no-taints", list(range(0, n, 4)))]
    pl, cfg = _default(cl)
    assert ((np.asarray(pl.tables["n_tt"]) * np.asarray(pl.tables["n_na"]))[cl.pods["cls"]] == abi.MAX_RCLASS).all()
    refs = [_oracle(cl, pl, cfg, a, 0, len(cl.pods)) for _, a in sets_]
    g = _default_scheduler(cl)
    out, _, _ = _sweep_and_check(g, cl, sets_, refs)
    got = out[0][out[0] >= 0]
    assert len({(int(i) % 4, (int(i) // 4) % 4) for i in got}) == 16  # every (taints, tier) pair receives pods
    for k in range(3, len(sets_)):
        assert not np.array_equal(out[k], out[0]), sets_[k][0]
    g.close()


def test_more_than_sixteen_reduce_classes_are_refused():
    nodes, pods = sixteen_class_workload(203, 5)
    cl = ingest.Cluster.from_objects(nodes, (), pods)
    p = len(cl.pods)
    g = _default_scheduler(cl)
    assert ((np.asarray(g.tables["n_tt"]) * np.asarray(g.tables["n_na"]))[cl.pods["cls"]] == 20).all()
    before = g.node_state()
    with pytest.raises(abi.KsimUnsupported, match="reduce classes"):
        g.sweep(None, 0, p, absent=[[], [0]])
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    # the handle still schedules the queue
    preds, prios = scheduler.provider("DefaultProvider")
    ref, _, _, ref_ctr = cpu_ref.run(cl, scheduler.make_config(preds, prios), 0, p, threads=4, tables=g.tables,
                                     na_add=g.na_add)
    got, _, _ = g.schedule(0, p)
    assert np.array_equal(got, ref) and g.last_node_index == ref_ctr
    g.close()


# ---- 5. the node cap: 38,400 nodes = 150 KiB of dynamic LDS, KS = 38, the last segment partial
@functools.lru_cache(maxsize=None)
def _cap_case():
    n = abi.SWEEP_GENERAL_MAX_NODES
    cl = _c2_cluster(n, 300, 2)
    sets_ = [("none", []), ("first", [0]), ("last", [n - 1]), ("last-segment-edge", [n - 21, n - 20]),
             ("random-10pct", _random_tenth(n))]
    pl, cfg = _default(cl)
    refs = [_oracle(cl, pl, cfg, a, 0, len(cl.pods)) for _, a in sets_]
    return cl, sets_, refs


def test_node_cap_runs_with_150_kib_of_lds():
    cl, sets_, refs = _cap_case()
    n = cl.n_nodes
    assert n == 38400 and n * 4 == 150 * 1024
    assert -(-n // 1024) == 38 and (n - 20) % 38 == 0 and (n - 20) // 38 == 1010  # thread 1010 owns the last 20 rows
    assert int((cl.pods["port_cnt"] > 0).sum()) > 50
    pl, _ = _default(cl)
    assert int((np.asarray(pl.tables["n_tt"]) * np.asarray(pl.tables["n_na"]))[cl.pods["cls"]].max()) == 2
    g = _default_scheduler(cl)
    out, _, st = _sweep_and_check(g, cl, sets_, refs)
    assert st.kernel_launches == 1 and st.blocks == len(sets_)  # five scenarios in one launch
    for k in range(2, len(sets_)):  # (node 0 takes none of the 300 pods)
        assert not np.array_equal(out[k], out[0]), sets_[k][0]
    g.close()


def test_one_node_beyond_the_cap_is_refused():
    cl = _c2_cluster(abi.SWEEP_GENERAL_MAX_NODES + 1, 300, 2)
    g = _default_scheduler(cl)
    with pytest.raises(abi.KsimUnsupported, match="38400"):
        g.sweep(None, 0, len(cl.pods), absent=[[], [0]])
    assert g.last_node_index == 0
    g.close()


# ---- 6. the top of the 27 score bits
TOP_WEIGHT = 2**27 // 10 - 1  # 13,421,771: scores reach 134,217,710 < 2^27
TOP_POLICIES = [[("LeastRequestedPriority", TOP_WEIGHT)],
                [("MostRequestedPriority", TOP_WEIGHT // 2),
                 ("BalancedResourceAllocation", TOP_WEIGHT - TOP_WEIGHT // 2)]]


def test_scores_at_the_top_of_27_bits():
    assert TOP_WEIGHT == 13421771 and TOP_POLICIES[1][0][1] == 6710885 and TOP_POLICIES[1][1][1] == 6710886
    cl = _c2_cluster(1500, 1200, 2)
    p = len(cl.pods)
    g = scheduler.GenericScheduler(cl, PREDS, TOP_POLICIES[0], collect_reasons=False)
    fit, _, score, _ = g.evaluate(0)
    assert 2**26 <= int(score[fit].max()) < 2**27  # the packed score's top bit is in use
    sets_ = [("none", []), ("last", [cl.n_nodes - 1])]
    refs = [_oracle(cl, g, scheduler.make_config(PREDS, pri), a, 0, p) for (_, a), pri in zip(sets_, TOP_POLICIES)]
    out, _, _ = _sweep_and_check(g, cl, sets_, refs, scenarios=TOP_POLICIES)
    assert not np.array_equal(out[0], out[1])
    # one weight higher, in one priority or in the sum: refused
    with pytest.raises(abi.KsimUnsupported, match="27 bits"):
        g.sweep([[("MostRequestedPriority", 6710886), ("BalancedResourceAllocation", 6710886)]], 0, p, absent=[[]])
    with pytest.raises(abi.KsimUnsupported, match="weight out of range"):
        g.sweep([[("LeastRequestedPriority", TOP_WEIGHT + 1)]], 0, p, absent=[[]])
    assert g.last_node_index == 0
    g.close()


# ---- 7. the port-slot overflow return
def test_port_slot_overflow_is_an_error_return_and_the_next_call_starts_clear():
    """One port slot a node: the first 50 pods of c2_objects(64, 3000, seed=7) never need a second
    one, the first 100 do.  The overflow is a bounded error return (ksim_commit checks the slot
    count before it stores) in the sweep's own error word, which every call clears."""
    nodes, pods = synth.c2_objects(64, 3000, seed=7)
    cl = ingest.Cluster.from_objects(nodes, (), pods, port_slots=1)
    wide = _c2_cluster(64, 3000, 7)  # the same objects with the slots the queue needs
    assert cl.port_slots == 1 and wide.port_slots > 1
    pl, cfg = _default(cl)
    _, _, s50, _ = cpu_ref.run(wide, cfg, 0, 50, threads=4, tables=pl.tables, na_add=pl.na_add)
    _, _, s100, _ = cpu_ref.run(wide, cfg, 0, 100, threads=4, tables=pl.tables, na_add=pl.na_add)
    assert int(s50["port_count"].max()) == 1 and int(s100["port_count"].max()) == 2
    sets_ = [("none", []), ("two-nodes", [5, 6])]
    refs = [_oracle(cl, pl, cfg, a, 0, 50) for _, a in sets_]  # (the oracle itself fails where a slot overflows)
    assert not np.array_equal(refs[0][0], refs[1][0])
    for _, a in sets_:  # both scenarios run out of slots within 100 pods, as the oracle does
        with pytest.raises(RuntimeError, match="-6"):
            _oracle(cl, pl, cfg, a, 0, 100)
    # 100 pods that need one slot only: the same scratch layout as the overflowing call, so the
    # error word of the call after it lies where the overflow was recorded
    refs_b = [_oracle(cl, pl, cfg, a, 1600, 100) for _, a in sets_]
    g = _default_scheduler(cl)
    _sweep_and_check(g, cl, sets_, refs, count=50)
    _sweep_and_check(g, cl, sets_, refs_b, first=1600, count=100)
    before = g.node_state()
    with pytest.raises(abi.KsimError) as e:
        g.sweep(None, 0, 100, absent=[a for _, a in sets_])
    assert e.value.code == abi.E_OVERFLOW
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == 0
    # the error word starts clear in every call
    _sweep_and_check(g, cl, sets_, refs_b, first=1600, count=100)
    _sweep_and_check(g, cl, sets_, refs, count=50)
    g.close()


# ---- 8. the remaining documented refusals
def test_auxiliary_priority_tables_are_refused():
    """A serviceAntiAffinity priority with services selecting pods loads the auxiliary counted
    priority, which only the launch-form kernels read.  The swept pod itself carries no affinity or
    spread state: a host-port pod no service selects."""
    from ksim import spread
    from workloads import rnd_spread_workload
    zone = "failure-domain.beta.kubernetes.io/zone"
    nodes, running, pods, objs = rnd_spread_workload(1, n_pods=20)
    plain = {"metadata": {"name": "plain", "namespace": "elsewhere"},
             "spec": {"containers": [{"resources": {"requests": {"cpu": "100m"}},
                                      "ports": [{"containerPort": 80, "hostPort": 8080, "protocol": "TCP"}]}]}}
    cl = ingest.Cluster.from_objects(nodes, running, pods + [plain], spread=spread.SpreadListers(**objs),
                                     aux=("service_anti_affinity", zone))
    assert cl.aux_active
    k = len(pods)
    assert cl.pods["aff_ident"][k] == 0 and cl.pods["aff_class"][k] == 0 and cl.pods["port_cnt"][k] == 1
    preds, _ = scheduler.provider("DefaultProvider")
    g = scheduler.GenericScheduler(cl, preds, [("SAA", 2), ("LeastRequestedPriority", 1)], collect_reasons=False,
                                   custom_priorities={"SAA": ("serviceAntiAffinity", zone)})
    with pytest.raises(abi.KsimUnsupported, match="auxiliary spreading priority or CheckServiceAffinity's lender table"):
        g.sweep(None, k, 1, absent=[[], [0]])
    with pytest.raises(abi.KsimUnsupported, match="inter-pod affinity or spread state"):
        g.sweep(None, 0, k + 1, absent=[[], [0]])
    g.close()


def test_node_sharded_handle_is_refused():
    """One rank of a two-rank node-sharded scheduler (not connected: the refusal precedes any
    launch) over a queue that is not resource-only."""
    cl = _c2_cluster(64, 3000, 7)
    preds, prios = scheduler.provider("DefaultProvider")
    s = scheduler.ShardedScheduler(cl, preds, prios, 0, 2)
    with pytest.raises(abi.KsimUnsupported, match="node-sharded handle sweeps resource-only pods only"):
        s.sweep(None, 0, 100, absent=[[], [0]])
    s.close()
