"""The histogram sub-form of the fast kernel's cached form (ksim_pfast.hip, KSIM_FORM_HIST): every
case runs in the default form, with KSIM_NO_PHIST=1 (the plain cached form) and under the C oracle,
and the three agree bit for bit — placements, FitError histograms, lastNodeIndex, node state.
ksim_last_form shows bit 8 exactly where the sub-form applies: the cached form is eligible, the
weight sum x 10 is at most 63, and the [classes][64] uint16 counts fit LDS beside rows and cache.

Geometries: one workgroup of one 64-row segment, a workgroup of 65 rows (one row in its second
segment) and a ragged last workgroup, 4 rows per thread (28 segment masks), a table that ties
everywhere, a queue that saturates until F = 1 and F = 0, 64 classes with and without room for the
counts, the score cap on either side, and short calls on one handle around the descriptor ring."""
import numpy as np
import pytest

import cpu_ref
import fast_edge_inputs as fe
from ksim import abi, scheduler, synth

pytestmark = pytest.mark.gpu

ENV_KNOBS = ("KSIM_NO_PHIST", "KSIM_NO_PCACHE", "KSIM_FORCE_STREAM", "KSIM_NO_PFAST", "KSIM_MAX_GRID")
SCORE_CAP = 63


def _score_sum(prios):
    return 10 * sum(w for _, w in prios)


CASES = [c for c in fe.all_edge_cases() if _score_sum(c[2]) <= SCORE_CAP]
CASE_IDS = [c[0] for c in CASES]
assert len(CASES) == len(fe.all_edge_cases())  # every policy of the module is within the cap


def _rows(form):
    return (form >> abi.FORM_ROWS_SHIFT) & 0xFF


def _hist(rows=None):
    """FAST | CACHED | HIST, not STREAM."""
    return lambda f: f & 15 == 13 and (rows is None or _rows(f) == rows)


def _plain(rows=None):
    """FAST | CACHED without HIST."""
    return lambda f: f & 15 == 5 and (rows is None or _rows(f) == rows)


def _run(cl, preds, prios, calls=None, **kw):
    g = scheduler.GenericScheduler(cl, preds, prios, mode=abi.MODE_PERSISTENT, **kw)
    try:
        m = len(cl.pods)
        calls = [m] if calls is None else calls
        assert sum(calls) == m
        outs, rss, forms, blocks, first = [], [], [], [], 0
        for c in calls:
            o, r, st = g.schedule(first, c)
            outs.append(o)
            rss.append(r)
            forms.append(g.last_form)
            blocks.append(st.blocks)
            first += c
        rs = np.concatenate(rss) if rss[0] is not None else None
        return dict(out=np.concatenate(outs), reasons=rs, forms=forms, blocks=blocks, ctr=g.last_node_index,
                    state=g.node_state())
    finally:
        g.close()


def _check(res, ref, reasons_required=False):
    out, reasons, state, ctr = ref
    assert np.array_equal(res["out"], out)
    failed = out < 0
    assert res["reasons"] is not None or not reasons_required
    if res["reasons"] is not None:
        assert np.array_equal(res["reasons"][failed], reasons[failed])
    assert res["ctr"] == ctr
    for k in fe.STATE_KEYS:
        assert np.array_equal(res["state"][k], state[k]), k


def _three_ways(monkeypatch, cl, prios, default_form, env=None, calls=None, blocks=None, ref=None, preds=None, **kw):
    """Default form (default_form tells which), KSIM_NO_PHIST=1 (always plain cached), the oracle."""
    preds = fe.PREDS if preds is None else preds
    if ref is None:
        ref = cpu_ref.run(cl, scheduler.make_config(preds, prios), threads=8)
    for no_hist in (False, True):
        for k in ENV_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, str(v))
        if no_hist:
            monkeypatch.setenv("KSIM_NO_PHIST", "1")
        res = _run(cl, preds, prios, calls=calls, **kw)
        want = _plain(_rows(res["forms"][0])) if no_hist else default_form
        assert all(want(f) for f in res["forms"]), [hex(f) for f in res["forms"]]
        if blocks is not None:
            assert res["blocks"] == [blocks] * len(res["forms"])
        _check(res, ref, reasons_required=bool(kw.get("collect_reasons")))
    return ref


def _c3_cluster(n, m, seed, classes=None, fill=0.7, pod_values=6):
    """C3-shaped nodes and pods whose allowed_pods sums to fill * m, spread evenly, so the queue
    saturates (tests/test_gpu_fast_edges.py: the same builder).  classes = k: k distinct cpu
    requests; pod_values = v: the C3 pods drawn from the first v cpu and memory sizes."""
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
        pcpu[:classes] = 100 + 10 * np.arange(classes)
        pmem = np.full(m, synth.GI, np.int64)
    cap = int(fill * m)
    i = np.arange(n, dtype=np.int64)
    allowed = ((i + 1) * cap // n - i * cap // n).astype(np.int32)
    return synth.resource_cluster(["h-%06d" % k for k in range(n)], cpu, mem, allowed, pcpu, pmem)


def _saturates(ref):
    assert (ref[0] < 0).sum() >= 100 and (ref[0] >= 0).sum() >= 100


# ------------------------------------------------------------------ every edge cluster
@pytest.mark.parametrize("name,cl,prios", CASES, ids=CASE_IDS)
def test_edge_cluster_three_ways(name, cl, prios, monkeypatch):
    _three_ways(monkeypatch, cl, prios, _hist())


# ------------------------------------------------------------------ geometries
def test_one_workgroup_one_segment_one_class(monkeypatch):
    cl = _c3_cluster(64, 1500, seed=71, classes=1)
    _saturates(_three_ways(monkeypatch, cl, fe.LR_BRA, _hist(1), blocks=1))


@pytest.mark.parametrize("n,last", [(130, 65), (129, 64)])
def test_two_workgroups_of_65_rows(n, last, monkeypatch):
    """KSIM_MAX_GRID=2: 65 rows a workgroup — the second row wave holds one row — and with 129 rows a
    last workgroup one row short."""
    assert (n + 1) // 2 == 65 and n - 65 == last
    cl = _c3_cluster(n, 2000, seed=72)
    _saturates(_three_ways(monkeypatch, cl, fe.LR_BRA, _hist(1), env={"KSIM_MAX_GRID": 2}, blocks=2))


def test_four_rows_per_thread_28_segments(monkeypatch):
    """1,000 rows in one workgroup: 4 rows per row thread, the masks span 4 x 7 segments (25 classes:
    96 B a row + 50 B of cache + 3,200 B of counts fit 150 KiB)."""
    cl = _c3_cluster(1000, 3000, seed=73, pod_values=5)
    _saturates(_three_ways(monkeypatch, cl, fe.LR_BRA, _hist(4), env={"KSIM_MAX_GRID": 1}, blocks=1))


def test_uniform_cluster_ties_everywhere(monkeypatch):
    """1,999 identical nodes, one class: every row is at the top, the rank walks across segments and
    both workgroups, the tie set shrinks by one per pod and refills when its last node drops."""
    n = 1999
    cl = synth.resource_cluster(["t-%04d" % i for i in range(n)], np.full(n, 32000, np.int64),
                                np.full(n, 128 * synth.GI, np.int64), np.full(n, 110, np.int32),
                                np.full(3 * n, 4000, np.int64), np.full(3 * n, 8 * synth.GI, np.int64))
    ref = cpu_ref.run(cl, scheduler.make_config(fe.PREDS, fe.LR_BRA), threads=8)
    assert len(set(ref[0][:n].tolist())) == n and len(set(ref[0][n:2 * n].tolist())) == n
    _three_ways(monkeypatch, cl, fe.LR_BRA, _hist(4), env={"KSIM_MAX_GRID": 2}, calls=[n + 7, 2 * n - 7], blocks=2, ref=ref)


def test_saturating_queue_until_nothing_fits(monkeypatch):
    """70 % fill on two workgroups, reasons collected: the top buckets empty one after another,
    the last pods that fit see F = 1, the rest fail with F = 0."""
    cl = _c3_cluster(300, 3000, seed=74)
    ref = cpu_ref.run(cl, scheduler.make_config(fe.PREDS, fe.LR_BRA), threads=8)
    _saturates(ref)
    first_fail = int(np.argmax(ref[0] < 0))
    assert (ref[0][first_fail:] < 0).sum() >= 100  # a long run of F = 0 after the table filled
    _three_ways(monkeypatch, cl, fe.LR_BRA, _hist(1), env={"KSIM_MAX_GRID": 2}, calls=[1200, 1800], blocks=2, ref=ref,
                collect_reasons=True)


# ------------------------------------------------------------------ eligibility
def _weights(lr, bra):
    return [("LeastRequestedPriority", lr), ("BalancedResourceAllocation", bra)]


@pytest.mark.parametrize("w,want", [((3, 3), _hist(1)), ((3, 4), _plain(1))], ids=["60-hist", "70-plain-cached"])
def test_score_cap(w, want, monkeypatch):
    """lane = score: the weight sum x 10 is at most 63."""
    cl = _c3_cluster(300, 2000, seed=75)
    _saturates(_three_ways(monkeypatch, cl, _weights(*w), want))


@pytest.mark.parametrize("n,want", [(2400, _hist(2)), (2740, _plain(2))], ids=["64x600-hist", "64x685-plain-cached"])
def test_counts_fit_beside_rows_and_cache(n, want, monkeypatch):
    """64 classes on 4 workgroups: at 600 rows the 8 KiB of counts fit, at 685 rows only rows and
    cache do — the plain cached form, not the uncached one."""
    cl = _c3_cluster(n, 5000, seed=76, classes=64)
    _saturates(_three_ways(monkeypatch, cl, fe.LR_BRA, want, env={"KSIM_MAX_GRID": 4}, blocks=4))


def test_no_pcache_turns_the_sub_form_off_too(monkeypatch):
    cl = _c3_cluster(200, 600, seed=77)
    ref = cpu_ref.run(cl, scheduler.make_config(fe.PREDS, fe.LR_BRA), threads=4)
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KSIM_NO_PCACHE", "1")
    res = _run(cl, fe.PREDS, fe.LR_BRA)
    assert res["forms"][0] & 15 == 1
    _check(res, ref)


# ------------------------------------------------------------------ short calls on one handle
def test_short_calls_rebuild_the_histograms(monkeypatch):
    """Calls of 1, 7, 8, 9 and 17 pods, then the rest: the ring is refilled, both parities of `first`
    occur, and every call rebuilds cache and counts from the table the previous one left."""
    calls = [1, 7, 8, 9, 17]
    cl = _c3_cluster(200, 900, seed=78, fill=0.85)
    ref = cpu_ref.run(cl, scheduler.make_config(fe.PREDS, fe.LR_BRA), threads=4)
    assert (ref[0] < 0).sum() >= 100
    _three_ways(monkeypatch, cl, fe.LR_BRA, _hist(1), calls=calls + [900 - sum(calls)], ref=ref)
