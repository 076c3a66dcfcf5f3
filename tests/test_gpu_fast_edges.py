"""The float64 fast path (csrc/ksim_f64.h: kf64::feval) at its score edges, caps and geometries.

Every cluster of tests/fast_edge_inputs.py goes through every form that evaluates rows in
float64 — the fast persistent kernel cached, uncached and streaming (ksim_pfast.hip), tree mode
(ksim_tree.hip), the policy sweep's tree and scan forms (ksim_sweep.hip) — and through two int64
forms as cross-checks, each against the C oracle, bit for bit: placements, FitError histograms,
lastNodeIndex and the node state.  Then the fast kernel's instantiations (1, 2, 4 rows per row
thread), its LDS-fit rule on either side, the class, weight and score caps, short calls around the
descriptor ring, and a table that ties everywhere.  ksim_last_form tells which form ran."""
import numpy as np
import pytest

import cpu_ref
import fast_edge_inputs as fe
from ksim import abi, scheduler, synth

pytestmark = pytest.mark.gpu

CASES = fe.all_edge_cases()
CASE_IDS = [c[0] for c in CASES]
ENV_KNOBS = ("KSIM_NO_PCACHE", "KSIM_FORCE_STREAM", "KSIM_NO_PFAST", "KSIM_SWEEP_SCAN", "KSIM_MAX_GRID")
# form id -> (mode, environment, check of (last_form, stats.mode))
FORMS = {
    "cached": (abi.MODE_PERSISTENT, {}, lambda f, m: f & 5 == 5 and m == abi.MODE_PERSISTENT),
    "uncached": (abi.MODE_PERSISTENT, {"KSIM_NO_PCACHE": "1"}, lambda f, m: f & 7 == 1),
    "stream": (abi.MODE_PERSISTENT, {"KSIM_FORCE_STREAM": "1"}, lambda f, m: f & 3 == 3),
    "tree": (abi.MODE_TREE, {}, lambda f, m: m == abi.MODE_TREE),
    "general": (abi.MODE_PERSISTENT, {"KSIM_NO_PFAST": "1"}, lambda f, m: f == 0 and m == abi.MODE_PERSISTENT),
    "launch": (abi.MODE_LAUNCH, {}, lambda f, m: f == 0 and m == abi.MODE_LAUNCH),
}
_REF = {}


def _rows(form):
    return (form >> abi.FORM_ROWS_SHIFT) & 0xFF


def _ref(key, cl, preds, prios):
    """The C oracle's run of the whole queue, computed once per cluster and policy."""
    if key not in _REF:
        _REF[key] = cpu_ref.run(cl, scheduler.make_config(preds, prios), threads=4)
    return _REF[key]


def _env(monkeypatch, env):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _run(cl, preds, prios, mode, calls=None, **kw):
    """Schedule the queue in `calls` (counts, default one call): placements, histograms, the form
    and stats of every call, the counter and the node state."""
    g = scheduler.GenericScheduler(cl, preds, prios, mode=mode, **kw)
    try:
        m = len(cl.pods)
        calls = [m] if calls is None else calls
        assert sum(calls) == m
        outs, rss, forms, stats, first = [], [], [], [], 0
        for c in calls:
            o, r, st = g.schedule(first, c)
            outs.append(o)
            rss.append(r)
            forms.append(g.last_form)
            stats.append((st.mode, st.blocks))
            first += c
        rs = np.concatenate(rss) if rss[0] is not None else None
        return dict(out=np.concatenate(outs), reasons=rs, forms=forms, stats=stats, ctr=g.last_node_index,
                    state=g.node_state())
    finally:
        g.close()


def _check(res, ref):
    out, reasons, state, ctr = ref
    assert np.array_equal(res["out"], out)
    failed = out < 0
    if res["reasons"] is not None:
        assert np.array_equal(res["reasons"][failed], reasons[failed])
    assert res["ctr"] == ctr
    for k in fe.STATE_KEYS:
        assert np.array_equal(res["state"][k], state[k]), k


# ------------------------------------------------------------------ §3: every cluster, every form
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name,cl,prios", CASES, ids=CASE_IDS)
def test_edge_cluster_matches_c_oracle(name, cl, prios, form, monkeypatch):
    mode, env, ok = FORMS[form]
    _env(monkeypatch, env)
    ref = _ref(name, cl, fe.PREDS, prios)
    assert not any((ref[2][k] >= 2 ** 48).any() for k in ("req_cpu", "req_mem", "nz_cpu", "nz_mem"))
    res = _run(cl, fe.PREDS, prios, mode)
    assert ok(res["forms"][0], res["stats"][0][0]), (hex(res["forms"][0]), res["stats"])
    _check(res, ref)


@pytest.mark.parametrize("scan", [False, True], ids=["tree", "scan"])
@pytest.mark.parametrize("name,cl,prios", CASES, ids=CASE_IDS)
def test_edge_cluster_sweep_matches_c_oracle(name, cl, prios, scan, monkeypatch):
    """The policy sweep's tree and scan forms over the same clusters, one scenario = the policy."""
    _env(monkeypatch, {"KSIM_SWEEP_SCAN": "1"} if scan else {})
    ref = _ref(name, cl, fe.PREDS, prios)
    g = scheduler.GenericScheduler(cl, fe.PREDS, prios, collect_reasons=False)
    try:
        before = g.node_state()
        out, ctr, st = g.sweep([prios], 0, len(cl.pods))
        assert st.mode == (abi.MODE_PERSISTENT if scan else abi.MODE_TREE)
        assert np.array_equal(out[0], ref[0])
        assert int(ctr[0]) == ref[3]
        after = g.node_state()
        for k in fe.STATE_KEYS:
            assert np.array_equal(before[k], after[k]), k
    finally:
        g.close()


# ------------------------------------------------------------------ §4: geometry, caps and ties
LR_BRA = fe.LR_BRA


def _grid(n, max_grid=None):
    """min(CUs, KSIM_MAX_GRID, ceil(n / 64)) on a device of at least 141 CUs (the largest grid here)."""
    return min(max_grid or 1 << 30, (n + 63) // 64)


def _c3_cluster(n, m, seed, classes=None, fill=0.7, pod_values=6):
    """C3-shaped nodes and pods; allowed_pods sums to fill * m, spread evenly, so the queue
    saturates.  classes = k: k distinct cpu requests (one memory size) instead of the C3 pods;
    pod_values = v: the C3 pods drawn from the first v cpu and memory sizes (v * v classes)."""
    cpu, mem = synth.c3_nodes(n, seed)
    if classes is None and pod_values == 6:
        pcpu, pmem = synth.c3_pods(m, seed)
    elif classes is None:
        r = synth.splitmix64(seed + 1000, 2 * m)
        pcpu = synth._pick(r[0::2], [100, 250, 500, 1000, 2000, 4000][:pod_values])
        pmem = synth._pick(r[1::2], [(256 << k) * synth.MI for k in range(pod_values)])
    else:
        r = synth.splitmix64(seed + 77, m)
        pcpu = 100 + 10 * (r % np.uint64(classes)).astype(np.int64)
        pcpu[:classes] = 100 + 10 * np.arange(classes)  # every class occurs
        pmem = np.full(m, synth.GI, np.int64)
    cap = int(fill * m)
    i = np.arange(n, dtype=np.int64)
    allowed = ((i + 1) * cap // n - i * cap // n).astype(np.int32)
    return synth.resource_cluster(["g-%06d" % k for k in range(n)], cpu, mem, allowed, pcpu, pmem)


def _saturating_run(cl, prios, mode, want_form, want_blocks=None, preds=None, saturates=True, **kw):
    """Two calls of a saturating queue against the oracle; want_form(form, stats mode) for both."""
    preds = fe.PREDS if preds is None else preds
    ref = cpu_ref.run(cl, scheduler.make_config(preds, prios), threads=8)
    if saturates:
        assert (ref[0] < 0).sum() >= 100 and (ref[0] >= 0).sum() >= 100
    m = len(cl.pods)
    res = _run(cl, preds, prios, mode, calls=[m * 2 // 5, m - m * 2 // 5], **kw)
    for f, (md, blocks) in zip(res["forms"], res["stats"]):
        assert want_form(f, md), (hex(f), md)
        if want_blocks is not None:
            assert blocks == want_blocks
    _check(res, ref)
    return res


def _cached(rows=None):
    return lambda f, m: f & 7 == 5 and (rows is None or _rows(f) == rows)


def _uncached(rows=None):
    return lambda f, m: f & 7 == 1 and (rows is None or _rows(f) == rows)


def _stream(rows=None):
    return lambda f, m: f & 7 == 3 and (rows is None or _rows(f) == rows)


@pytest.mark.parametrize("no_cache", [False, True], ids=["cached", "uncached"])
@pytest.mark.parametrize("max_grid,n,m,rows_wg,rpt,last", [(None, 9000, 6000, 64, 1, 40), (4, 2399, 5000, 600, 2, 599),
                                                           (2, 1999, 4000, 1000, 4, 999)])
def test_rows_per_thread_instantiations(max_grid, n, m, rows_wg, rpt, last, no_cache, monkeypatch):
    """ksim_pfast_kernel<1|2|4, false, cached|uncached>: the grid is min(CUs, KSIM_MAX_GRID,
    ceil(n/64)), a workgroup holds ceil(n/grid) rows and the last one fewer."""
    env = {"KSIM_NO_PCACHE": "1"} if no_cache else {}
    if max_grid:
        env["KSIM_MAX_GRID"] = max_grid
    _env(monkeypatch, env)
    grid = _grid(n, max_grid)
    assert (n + grid - 1) // grid == rows_wg and n - (grid - 1) * rows_wg == last
    # (1,000 rows beside their cached evaluations fit the LDS budget up to 28 classes: 25 of the 36)
    cl = _c3_cluster(n, m, seed=50 + rpt, pod_values=5 if rows_wg == 1000 else 6)
    _saturating_run(cl, LR_BRA, abi.MODE_PERSISTENT, (_uncached if no_cache else _cached)(rpt), want_blocks=grid)


@pytest.mark.parametrize("classes,cached", [(28, True), (29, False)])
def test_lds_fit_by_class_count(classes, cached, monkeypatch):
    """1,000 rows per workgroup: 96 B a row and 2 B a (class, row) fit 150 KiB up to 28 classes."""
    _env(monkeypatch, {"KSIM_MAX_GRID": 2})
    cl = _c3_cluster(1999, 4000, seed=61, classes=classes)
    _saturating_run(cl, LR_BRA, abi.MODE_PERSISTENT, (_cached if cached else _uncached)(4), want_blocks=2)


@pytest.mark.parametrize("n,classes,want", [(1567, 1, _cached(4)), (1568, 1, _uncached(4)), (1600, 3, _uncached(4)),
                                            (1601, 3, _stream(4))],
                         ids=["1567-cached", "1568-uncached", "1600-full-lds", "1601-stream"])
def test_lds_fit_by_rows_single_workgroup(n, classes, want, monkeypatch):
    """One workgroup: the cached form up to 1,567 rows, the uncached one up to the full 150 KiB
    (1,600 rows), the streaming form beyond."""
    _env(monkeypatch, {"KSIM_MAX_GRID": 1})
    cl = _c3_cluster(n, 3200, seed=62, classes=classes)
    _saturating_run(cl, LR_BRA, abi.MODE_PERSISTENT, want, want_blocks=1)


@pytest.mark.parametrize("n,classes,want", [(2740, 64, _cached(2)), (2744, 64, _uncached(2)), (2740, 65, _uncached(2)),
                                            (2740, 1, _cached(2))],
                         ids=["64x685-cached", "64x686-uncached", "65-uncached", "1-cached"])
def test_class_count_caps(n, classes, want, monkeypatch):
    """64 tree classes (one lane per class) at the LDS edge, and the 65th that turns the cached
    form off."""
    _env(monkeypatch, {"KSIM_MAX_GRID": 4})
    cl = _c3_cluster(n, 5000, seed=63, classes=classes)
    _saturating_run(cl, LR_BRA, abi.MODE_PERSISTENT, want, want_blocks=4)


@pytest.mark.parametrize("classes,tree", [(64, True), (65, False)])
def test_tree_mode_class_cap(classes, tree, monkeypatch):
    _env(monkeypatch, {})
    cl = _c3_cluster(700, 2000, seed=64, classes=classes)
    _saturating_run(cl, LR_BRA, abi.MODE_TREE, lambda f, m: (m == abi.MODE_TREE) == tree)


def _weights(lr, bra, mr=0):
    w = [("LeastRequestedPriority", lr), ("BalancedResourceAllocation", bra)]
    return w + ([("MostRequestedPriority", mr)] if mr else [])


WEIGHT_CLUSTER = None


def _weight_cluster():
    global WEIGHT_CLUSTER
    if WEIGHT_CLUSTER is None:
        WEIGHT_CLUSTER = _c3_cluster(300, 2000, seed=65)
    return WEIGHT_CLUSTER


@pytest.mark.parametrize("w,want", [((1638, 1638), _cached(1)), ((1638, 1639), _uncached(1)),
                                    ((1092, 1092, 1092), _cached(1)), ((1092, 1092, 1093), _uncached(1)),
                                    ((6710886, 6710886), _uncached(1))],
                         ids=["32760-cached", "32770-uncached", "32760-mr-cached", "32770-mr-uncached", "27bit-fast"])
def test_weight_caps_of_the_fast_kernel(w, want, monkeypatch):
    """The cached form keeps int16 evaluations (sum(w) * 10 < 32767); the fast kernel packs the
    score into 27 bits (sum(w) * 10 < 2^27)."""
    _env(monkeypatch, {})
    _saturating_run(_weight_cluster(), _weights(*w), abi.MODE_PERSISTENT, want)


@pytest.mark.parametrize("w,tree", [((3276, 3277), True), ((3277, 3277), False), ((2184, 2184, 2185), True),
                                    ((2185, 2185, 2184), False)],
                         ids=["65530-tree", "65540-not", "65530-mr-tree", "65540-mr-not"])
def test_weight_cap_of_tree_mode(w, tree, monkeypatch):
    """Tree mode packs score + 1 into 16 bits (sum(w) * 10 <= 65534)."""
    _env(monkeypatch, {})
    _saturating_run(_weight_cluster(), _weights(*w), abi.MODE_TREE, lambda f, m: (m == abi.MODE_TREE) == tree)


def test_weights_beyond_27_bits_leave_the_persistent_kernels(monkeypatch):
    _env(monkeypatch, {})
    prios = _weights(6710886, 6710887)
    _saturating_run(_weight_cluster(), prios, abi.MODE_AUTO, lambda f, m: f == 0 and m == abi.MODE_LAUNCH)
    g = scheduler.GenericScheduler(_weight_cluster(), fe.PREDS, prios, mode=abi.MODE_PERSISTENT)
    try:
        with pytest.raises(abi.KsimUnsupported):
            g.schedule(0, 10)
    finally:
        g.close()


@pytest.mark.parametrize("prios,preds,saturates", [([], None, True), (fe.MR, None, True),
                                                   (LR_BRA, ["CheckNodeCondition"], False)],
                         ids=["equal-priority", "mr-only", "condition-only-predicates"])
def test_other_policies_in_the_cached_form(prios, preds, saturates, monkeypatch):
    """EqualPriority (no weights), MostRequested alone, and a predicate set without
    PodFitsResources (nothing fails on resources or pod counts)."""
    _env(monkeypatch, {})
    cl = _c3_cluster(300, 2000, seed=66)
    _saturating_run(cl, prios, abi.MODE_PERSISTENT, _cached(1), preds=preds, saturates=saturates)


def test_degenerate_rows_with_reasons_in_the_cached_form(monkeypatch):
    _env(monkeypatch, {})
    cl = fe.degenerate_cluster()
    ref = _ref("degenerate", cl, fe.PREDS, fe.LR_MR_BRA)
    assert (ref[0] < 0).any() and (ref[0] >= 0).any()
    m = len(cl.pods)
    res = _run(cl, fe.PREDS, fe.LR_MR_BRA, abi.MODE_PERSISTENT, calls=[m // 3, m - m // 3], collect_reasons=True)
    assert all(f & 7 == 5 for f in res["forms"])
    _check(res, ref)


SHORT_CALLS = [1, 1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257]


@pytest.mark.parametrize("form", ["cached", "uncached", "stream"])
def test_short_calls_back_to_back(form, monkeypatch):
    """Calls around the 16-slot descriptor ring, its 8-pod refill and the 8-bit tag wrap, both
    parities of `first`: the concatenation equals one reference run."""
    mode, env, ok = FORMS[form]
    _env(monkeypatch, env)
    cl = _c3_cluster(200, sum(SHORT_CALLS), seed=67, fill=0.85)
    ref = cpu_ref.run(cl, scheduler.make_config(fe.PREDS, LR_BRA), threads=4)
    assert (ref[0] < 0).sum() >= 100
    res = _run(cl, fe.PREDS, LR_BRA, mode, calls=SHORT_CALLS)
    assert all(ok(f, m) for f, (m, _) in zip(res["forms"], res["stats"]))
    _check(res, ref)


@pytest.mark.parametrize("no_cache", [False, True], ids=["cached", "uncached"])
def test_uniform_cluster_ties_everywhere(no_cache, monkeypatch):
    """1,999 identical nodes and one pod class: the whole table ties, the tie set shrinks by one
    per pod and refills when its last node drops."""
    env = {"KSIM_MAX_GRID": 2}
    if no_cache:
        env["KSIM_NO_PCACHE"] = "1"
    _env(monkeypatch, env)
    n = 1999
    cl = synth.resource_cluster(["u-%04d" % i for i in range(n)], np.full(n, 32000, np.int64),
                                np.full(n, 128 * synth.GI, np.int64), np.full(n, 110, np.int32),
                                np.full(3 * n, 4000, np.int64), np.full(3 * n, 8 * synth.GI, np.int64))
    ref = cpu_ref.run(cl, scheduler.make_config(fe.PREDS, LR_BRA), threads=8)
    assert len(set(ref[0][:n].tolist())) == n and len(set(ref[0][n:2 * n].tolist())) == n
    res = _run(cl, fe.PREDS, LR_BRA, abi.MODE_PERSISTENT, calls=[n + 7, 2 * n - 7])
    assert all((_uncached if no_cache else _cached)(4)(f, m) for f, (m, _) in zip(res["forms"], res["stats"]))
    _check(res, ref)
