"""The owner's fix of the fast kernel's histogram sub-form (ksim_pfast.hip): the row waves leave the
finished fix granule of pod + 1 for every row pod can commit to, a workgroup-local word per row wave
tells the owner it is done, and the owner stores the granule of its row before the main barrier.  Every case
runs in the default form (ksim_last_form shows the sub-form), with KSIM_NO_PHIST=1 (the plain cached
form, whose owner computes the fix itself) and under the C oracle, and the three agree bit for bit —
placements, FitError histograms where collected, lastNodeIndex, node state.

The shapes are the smallest at which the new path can go wrong: one workgroup that owns every pod
while the class changes with every pod; two workgroups of 65 rows (a second row wave of one row, a
ragged last workgroup) under 64 classes; four candidate granules per lane; a top bucket of one row
whose commit lands below, on and above the next bucket; and calls of 1, 2 and 3 pods on one handle.
What each cluster is said to do is asserted on the oracle's result, which needs no GPU."""
import numpy as np
import pytest

import cpu_ref
import fast_edge_inputs as fe
from ksim import scheduler, synth
from test_gpu_fast_hist import _c3_cluster, _hist, _saturates, _three_ways

pytestmark = pytest.mark.gpu


def _ref(cl, prios):
    return cpu_ref.run(cl, scheduler.make_config(fe.PREDS, prios), threads=8)


def _alternating_cluster(n, m, fill=0.7):
    """C3-shaped nodes; the queue alternates between two resource-only classes, pod by pod."""
    cpu, mem = synth.c3_nodes(n, 81)
    odd = np.arange(m) % 2
    pcpu = np.where(odd, 1000, 250).astype(np.int64)
    pmem = np.where(odd, 1 * synth.GI, 2 * synth.GI).astype(np.int64)
    cap = int(fill * m)
    i = np.arange(n, dtype=np.int64)
    allowed = ((i + 1) * cap // n - i * cap // n).astype(np.int32)
    return synth.resource_cluster(["h-%06d" % k for k in range(n)], cpu, mem, allowed, pcpu, pmem)


def test_one_workgroup_two_classes_alternating(monkeypatch):
    """64 rows, one workgroup: it owns every pod, and pod + 1's class always differs from pod's — the
    tightest order of granules, done words and tail inside one workgroup.  Reasons collected."""
    cl = _alternating_cluster(64, 1500)
    ref = _ref(cl, fe.LR_BRA)
    _saturates(ref)
    _three_ways(monkeypatch, cl, fe.LR_BRA, _hist(1), blocks=1, ref=ref, collect_reasons=True)


@pytest.mark.parametrize("n,last", [(130, 65), (129, 64)])
def test_two_workgroups_of_65_rows_64_classes(n, last, monkeypatch):
    """KSIM_MAX_GRID=2: 65 rows a workgroup (the second row wave holds one row; with 129 rows the last
    workgroup is one short), the owner alternates, and 64 classes fill the lane = class re-evaluation."""
    assert (n + 1) // 2 == 65 and n - 65 == last
    cl = _c3_cluster(n, 2000, seed=82, classes=64)
    ref = _ref(cl, fe.LR_BRA)
    _saturates(ref)
    assert set(np.unique(ref[0][ref[0] >= 0] // 65).tolist()) == {0, 1}  # both workgroups own pods
    _three_ways(monkeypatch, cl, fe.LR_BRA, _hist(1), env={"KSIM_MAX_GRID": 2}, blocks=2, ref=ref)


def test_one_workgroup_of_1000_rows(monkeypatch):
    """1,000 rows in one workgroup: 4 rows per row thread, so a lane computes up to four candidate
    granules, and the owner's rank crosses the 28 segments.  9 classes."""
    cl = _c3_cluster(1000, 3000, seed=83, pod_values=3)
    ref = _ref(cl, fe.LR_BRA)
    _saturates(ref)
    _three_ways(monkeypatch, cl, fe.LR_BRA, _hist(4), env={"KSIM_MAX_GRID": 1}, blocks=1, ref=ref)


# ------------------------------------------------------------------ a top bucket of one row
LARGE = (7, 99)  # one larger node in each 65-row workgroup


def _single_top_cluster(m=900):
    """130 nodes of 8 cpu / 32 GiB but for one of 32 cpu / 128 GiB in each workgroup of 65; pods of
    four sizes, the largest of which fits the larger nodes only."""
    n = 130
    cpu = np.full(n, 8000, np.int64)
    mem = np.full(n, 32 * synth.GI, np.int64)
    for j in LARGE:
        cpu[j], mem[j] = 32000, 128 * synth.GI
    r = synth.splitmix64(84, m)
    pcpu = synth._pick(r, [500, 1000, 1000, 2000, 2000, 9000])
    pmem = pcpu * 4 * synth.MI
    return synth.resource_cluster(["h-%06d" % k for k in range(n)], cpu, mem, np.full(n, 110, np.int32), pcpu, pmem)


def _lr_eval(cpu, mem, allowed, uc, um, cnt, pc, pm):
    """LeastRequestedPriority (weight 1) of one pod on every node, -1 where it does not fit."""
    tc, tm = uc + pc, um + pm
    sc = ((cpu - tc) * 10 // cpu + (mem - tm) * 10 // mem) // 2
    return np.where((tc <= cpu) & (tm <= mem) & (cnt + 1 <= allowed), sc, -1)


def _single_top_commits(cl, out):
    """Replays the oracle's placements.  For every commit to a workgroup's larger node while that
    node is alone in the workgroup's top bucket of the pod's class: where the node's post-commit
    score for the next pod's class lands against the best other row of the workgroup."""
    c = cl.cols
    cpu, mem, allowed = c["alloc_cpu"], c["alloc_mem"], c["allowed_pods"].astype(np.int64)
    pcpu, pmem = np.asarray(cl.pods["req_cpu"], np.int64), np.asarray(cl.pods["req_mem"], np.int64)
    uc, um, cnt = np.zeros(130, np.int64), np.zeros(130, np.int64), np.zeros(130, np.int64)
    alone = {0: 0, 1: 0}
    landing = dict(below=0, on=0, above=0)
    for p, node in enumerate(out.tolist()):
        if node < 0:
            continue
        if node in LARGE and p + 1 < len(out):
            w = node // 65
            rows = slice(65 * w, 65 * w + 65)
            e = _lr_eval(cpu[rows], mem[rows], allowed[rows], uc[rows], um[rows], cnt[rows], pcpu[p], pmem[p])
            j = node - 65 * w
            if e[j] == e.max() and (e == e[j]).sum() == 1:
                alone[w] += 1
                uc2, um2, cnt2 = uc[rows].copy(), um[rows].copy(), cnt[rows].copy()
                uc2[j] += pcpu[p]; um2[j] += pmem[p]; cnt2[j] += 1
                e2 = _lr_eval(cpu[rows], mem[rows], allowed[rows], uc2, um2, cnt2, pcpu[p + 1], pmem[p + 1])
                nxt = np.delete(e2, j).max()
                landing["below" if e2[j] < nxt else "on" if e2[j] == nxt else "above"] += 1
        uc[node] += pcpu[p]; um[node] += pmem[p]; cnt[node] += 1
    return alone, landing


def test_top_bucket_of_one_row(monkeypatch):
    """Each workgroup's top bucket holds exactly one row, its larger node, for a while: the commit to
    it empties the bucket, and the row comes back below, on and above the next bucket (KSIM_MAX_GRID=2)."""
    cl = _single_top_cluster()
    ref = _ref(cl, fe.LR)
    alone, landing = _single_top_commits(cl, ref[0])
    assert alone[0] >= 1 and alone[1] >= 1, alone
    assert min(landing.values()) >= 1, landing
    _three_ways(monkeypatch, cl, fe.LR, _hist(1), env={"KSIM_MAX_GRID": 2}, blocks=2, ref=ref)


# ------------------------------------------------------------------ short calls on one handle
def test_calls_of_1_2_3_pods_then_the_rest(monkeypatch):
    """A call of one pod has no next pod; calls of 1, 2 and 3 start at both parities of `first`; and
    the done words start again with every call."""
    calls = [1, 2, 3]
    cl = _c3_cluster(200, 900, seed=85, fill=0.85)
    ref = _ref(cl, fe.LR_BRA)
    assert (ref[0] < 0).sum() >= 100 and (ref[0] >= 0).sum() >= 100
    _three_ways(monkeypatch, cl, fe.LR_BRA, _hist(1), calls=calls + [900 - sum(calls)], ref=ref)
