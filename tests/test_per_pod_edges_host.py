"""The per-pod edge tests' reference and inputs, checked alone (no device): what
tests/test_gpu_per_pod_edges.py compares the kernels with must itself equal the whole-queue C
oracle and the object-level oracle, and the inputs must have the properties the GPU cases rely
on — so a GPU failure there cannot be an input's fault."""
import bisect

import numpy as np
import pytest

import cpu_ref
import ksim_ref as R
import per_pod_inputs as I
from events import event_stream
from ksim import ingest, scheduler

CASES = {
    "rotation600": lambda: I.rotation(600),
    "rotation1025": lambda: I.rotation(1025),
    "rotation16385": lambda: I.rotation(16385, 40),
    "rotation262145": lambda: I.rotation(262145, 12),
    "saturate600": lambda: I.saturate(600),
    "saturate1025": lambda: I.saturate(1025),
    "sixteen600": lambda: I.sixteen(600),
    "selector600": lambda: I.selector(600, 200),
    "spread600x60": lambda: I.spread(600, 60),
    "spread600x61": lambda: I.spread(600, 61),
    "ports17": lambda: I.ports17(),
    "ports_late": lambda: I.ports_late(m=300),
}
_REC = {}


def _recorded(name):
    """(case, whole-queue oracle run, the Mirror's recorded stepping) — computed once per case."""
    if name not in _REC:
        case = CASES[name]()
        whole = cpu_ref.run(case.cl, None, 0, case.n_calls, threads=4, plan=scheduler.plan(case.cl, case.preds, case.prios))
        rec, final = I.record(I.Mirror(case.cl, case.preds, case.prios), I.assume_all(case), case.fit)
        _REC[name] = (case, whole, rec, final)
    return _REC[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_stepping_equals_the_whole_queue_run(name):
    case, (out, reasons, state, ctr, _), rec, final = _recorded(name)
    assert [e[0] for _, e in rec] == out.tolist()
    for i, (_, e) in enumerate(rec):
        assert e[2].tolist() == reasons[i].tolist(), i
    assert final["counter"] == ctr
    for key in I.DYNAMIC:
        assert np.array_equal(final[key], state[key]), key


def test_schedule_only_commits_nothing_but_the_counter():
    case = I.saturate(300)
    a, b = I.Mirror(case.cl, case.preds, case.prios), I.Mirror(case.cl, case.preds, case.prios)
    for k in range(200):
        node, _ = a.schedule(k, False)
        assert all(np.array_equal(a.state[key], b.state[key]) for key in a.state)
        if node >= 0:
            a.pod_add(node, k)
        assert b.schedule(k, True)[0] == node
        assert a.counter == b.counter
    assert all(np.array_equal(a.state[key], b.state[key]) for key in a.state)


@pytest.mark.parametrize("n", [2, 63, 600, 1025])
def test_rotation_law(n):
    case = I.rotation(n)
    rec, _ = I.record(I.Mirror(case.cl, case.preds, case.prios), I.assume_all(case), case.fit)
    assert [e[0] for _, e in rec] == [(n - 1 - k) % n for k in range(n + 3)]
    assert [e[1] for _, e in rec] == list(range(1, n + 4))
    assert all(e[3] == n for _, e in rec)


@pytest.mark.parametrize("n,chunk", [(600, 256), (600, 512), (1030, 1024), (2049, 2048), (2049, 512), (16385, 256),
                                     (262145, 512)])
def test_probes_reach_both_sides_of_every_boundary(n, chunk):
    ranks = set(I.probe_ranks(n, chunk))
    nodes = {n - 1 - r for r in ranks}
    for b in range(1, (n + chunk - 1) // chunk):
        assert {chunk * b - 1, chunk * b} <= nodes
    if n <= 20000:
        for seg in range(256, n, 256):  # every 256-node segment inside a fat block, too
            assert {seg - 1, seg} <= nodes
    assert {0, n - 1} <= nodes and set(I.FIXED_RANKS) & set(range(n)) <= ranks
    if n <= 2049:
        case, steps = I.probes(n, chunk)
        rec, _ = I.record(I.Mirror(case.cl, case.preds, case.prios), steps, case.fit)
        hit = [e[0] for _, e in rec if e is not None]
        aimed = [s[1] % n for s, _ in rec if s[0] == "counter"]
        assert hit == [n - 1 - r for r in aimed] and set(aimed) == ranks
        vals = [s[1] for s, _ in rec if s[0] == "counter"]
        assert any(v < 2 ** 32 <= v + n for v in vals) and any(2 ** 32 <= v < 2 ** 32 + n for v in vals)


def test_sixteen_has_sixteen_classes_and_fit_errors():
    case, _, rec, _ = _recorded("sixteen600")
    assert len(case.cl.pods) == 2407 and (I.reduce_classes(case) == 16).all()
    assert sum(e[0] < 0 for _, e in rec) >= 5


def test_saturate_has_single_fits_and_fit_errors_over_every_node():
    case, _, rec, _ = _recorded("saturate600")
    ctr = [0] + [e[1] for _, e in rec]
    single = [i for i, (_, e) in enumerate(rec) if e[0] >= 0 and ctr[i + 1] == ctr[i]]
    assert single and all(rec[i][1][3] == 1 for i in single)
    fails = [e for _, e in rec if e[0] < 0]
    assert len(fails) >= 20 and all(e[3] == 0 for e in fails)
    # every node gives at least one reason (a full node also lacks cpu or memory now and then)
    assert all(int(e[2].sum()) >= 600 for e in fails)
    assert sorted({e[3] for _, e in rec})[:3] == [0, 1, 2]


def test_selector_mix_changes_width_inside_every_tag_cycle():
    case = I.selector(600)
    order = I.selector_order()
    K = I.reduce_classes(case)[order]
    assert len(set(order)) == len(order) and len(K) >= 520 + 3 * 254
    for first in range(0, 540 - 254 + 1):
        assert {1, 2, 16} <= set(K[first:first + 254].tolist())
    assert all(K[k] != K[k + 1] for k in range(539))
    wide = [540 + 254 * j for j in range(4)]   # one tag cycle apart, one-class pods between
    assert K[wide].tolist() == [16] * 4 and set(np.delete(K[540:], [w - 540 for w in wide]).tolist()) == {1}


@pytest.mark.parametrize("Z", [60, 61])
def test_spread_zone_count(Z):
    case = I.spread(600, Z)
    assert I.zone_count(case) == Z
    assert (case.cl.pods["aff_class"] > 0).sum() > 50  # pods with spread selectors: a pass A each


def test_spread_after_plain_pods_has_pass_a_only_later():
    case = I.spread(600, 60, extra_pods=I.plain_pods(300))
    cls = case.cl.pods["aff_class"]
    assert not cls[:300].any() and (cls[300:] > 0).sum() > 50


def test_ports17_second_pod_skips_the_first_ones_node():
    case, _, rec, _ = _recorded("ports17")
    assert int(case.cl.pods["port_cnt"].max()) == 17
    (a, b) = [e for (s, e) in rec if case.cl.pods[s[1]]["port_cnt"]]
    assert a[3] == 600 and b[3] == 599 and a[0] == 600 - 1 - 20 and b[0] != a[0]


def test_ports_late_loads_every_block_but_the_first():
    case, _, rec, _ = _recorded("ports_late")
    pc = case.cl.cols["port_count"]
    assert not pc[:256].any() and (pc[256:] == 48).all() and (case.cl.pods["port_cnt"] == 16).all()
    assert [e[3] for _, e in rec] == [2048 - k for k in range(300)]  # every pod takes a node out
    # the pods walk down from the top: every commit changes the record of a late block
    assert all(e[0] >= 256 for _, e in rec) and len({e[0] // 256 for _, e in rec}) >= 2


# ----------------------------------------------------------------------------- cache events
POLICY = (["GeneralPredicates", "CheckNodeCondition", "PodToleratesNodeTaints", "CheckNodeMemoryPressure",
           "CheckNodeDiskPressure"], [("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)])


def _row(node, held):
    ns = ingest.node_static(node)
    d = [I.resource_desc(p)[0] for p in held.values()]
    return I.node_row(ns.alloc[0], ns.alloc[1], ns.allowed, sum(int(x["add_cpu"]) for x in d),
                      sum(int(x["add_mem"]) for x in d), sum(int(x["nz_cpu"]) for x in d),
                      sum(int(x["nz_mem"]) for x in d), len(d))


@pytest.mark.parametrize("seed", [0, 1])
def test_mirror_events_match_the_object_oracle(seed):
    """A 300-node informer stream (node add / remove, pod add / confirm / move / update / remove,
    scheduleOne) through the object-level oracle's cache and through Mirror.node_add / node_remove /
    pod_add / pod_remove / schedule: the same decisions, FitError texts, lastNodeIndex and node
    state.  (Node updates are left out on both sides: the Mirror has none.)"""
    preds, prios = POLICY
    ref = R.SchedulerCache(set(preds), prios)
    m = I.Mirror(I.rotation(0, 0).cl, preds, prios)
    names, held = [], {}          # listed names (bytewise), name -> {pod key: pod}

    def qidx(pod):
        return m.queue(I.resource_desc(pod))

    def add(pod):
        nn = pod["spec"]["nodeName"]
        held.setdefault(nn, {})[R.pod_key(pod)] = pod
        if nn in names:
            m.pod_add(names.index(nn), qidx(pod))

    def remove(pod):
        nn = pod["spec"]["nodeName"]
        held[nn].pop(R.pod_key(pod))
        if nn in names:
            m.pod_remove(names.index(nn), qidx(pod))

    decisions = fails = 0
    for kind, x in event_stream(seed, ref, n_events=500, n_nodes=300, features=False):
        if kind == "update_node":
            continue
        if kind == "schedule":
            want = ref.schedule_one(x)
            node, reasons = m.schedule(qidx(x), True)
            got = (names[node], None) if node >= 0 else (None, scheduler.fit_error_message(len(names), reasons, ()))
            assert got == want, x["metadata"]["name"]
            decisions += 1
            fails += node < 0
            if node >= 0:
                held.setdefault(names[node], {})[R.pod_key(x)] = dict(x, spec=dict(x["spec"], nodeName=names[node]))
            continue
        if kind == "add_node":
            name = x["metadata"]["name"]
            rank = bisect.bisect_left([s.encode() for s in names], name.encode())
            m.node_add(rank, _row(x, held.get(name, {})))
            names.insert(rank, name)
        elif kind == "remove_node":
            rank = names.index(x["metadata"]["name"])
            m.node_remove(rank)
            del names[rank]
        elif kind == "add_pod":
            cur = ref.pod_states.get(R.pod_key(x))
            if cur is not None and cur["spec"]["nodeName"] != x["spec"]["nodeName"]:
                remove(cur)
                add(x)
            elif cur is None:
                add(x)
        elif kind == "remove_pod":
            remove(ref.pod_states[R.pod_key(x)])
        elif kind == "update_pod":
            remove(x[0])
            add(x[1])
        getattr(ref, kind)(*x) if kind == "update_pod" else getattr(ref, kind)(x)
    assert decisions > 200 and m.counter == ref.sched.last_node_index
    assert names == sorted(ref.listed, key=lambda s: s.encode())
    for i, name in enumerate(names):
        ni = ref.nodes[name]
        s = m.state
        assert (s["req_cpu"][i], s["req_mem"][i], s["nz_cpu"][i], s["nz_mem"][i], s["pod_count"][i]) == \
            (ni.requested.cpu, ni.requested.mem, ni.nonzero_cpu, ni.nonzero_mem, len(ni.pods)), name
