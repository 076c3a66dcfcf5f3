"""Host-side checks of the fast path's edge inputs (tests/fast_edge_inputs.py): the C oracle is
pinned on every cluster against a plain-Python restatement written here (so it does not carry the
GPU tests on its own authority at these values), and the conditions that make the clusters
discriminating are asserted.  No device."""
import math

import numpy as np
import pytest

import cpu_ref
import fast_edge_inputs as fe
from ksim import abi, scheduler

CASES = fe.all_edge_cases()
IDS = [c[0] for c in CASES]


def _frac_score(num, cap):  # least_requested.go:44-53 / most_requested.go:45-55 per resource
    return lambda t: 0 if cap == 0 or t > cap else num(t, cap) * 10 // cap


def restate(cl, prios):
    """selectHost + AddPod over the resource-only predicates in Python ints (LR, MR) and Python
    floats (BRA): (placements, final lastNodeIndex)."""
    w = dict(prios)
    wl, wm, wb = (w.get(k, 0) for k in ("LeastRequestedPriority", "MostRequestedPriority", "BalancedResourceAllocation"))
    c = cl.cols
    n = cl.n_nodes
    ac, am, al, fl = ([int(x) for x in c[k]] for k in ("alloc_cpu", "alloc_mem", "allowed_pods", "flags"))
    rc, rm, zc, zm, cnt = ([int(x) for x in c[k]] for k in ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pod_count"))
    ctr, out = 0, []
    for P in cl.pods:
        qc, qm, pzc, pzm, pf = int(P["req_cpu"]), int(P["req_mem"]), int(P["nz_cpu"]), int(P["nz_mem"]), int(P["flags"])
        fit = [i for i in range(n) if not (fl[i] & abi.N_NOT_READY) and cnt[i] + 1 <= al[i]
               and not (pf & abi.POD_ANY_REQUEST and (ac[i] < qc + rc[i] or am[i] < qm + rm[i]))
               and not (pf & abi.POD_BEST_EFFORT and fl[i] & abi.N_MEM_PRESSURE)]
        if not fit:
            out.append(-1)
            continue
        win = fit[0]
        if len(fit) > 1:
            score = {}
            for i in fit:
                tc, tm = zc[i] + pzc, zm[i] + pzm
                lr = (_frac_score(lambda t, cap: cap - t, ac[i])(tc) + _frac_score(lambda t, cap: cap - t, am[i])(tm)) // 2
                mr = (_frac_score(lambda t, cap: t, ac[i])(tc) + _frac_score(lambda t, cap: t, am[i])(tm)) // 2
                fc = float(tc) / float(ac[i]) if ac[i] else 1.0
                fm = float(tm) / float(am[i]) if am[i] else 1.0
                br = 0 if fc >= 1.0 or fm >= 1.0 else int((1.0 - abs(fc - fm)) * 10.0)
                score[i] = wl * lr + wm * mr + wb * br
            best = max(score.values())
            tied = [i for i in reversed(fit) if score[i] == best]  # descending name rank
            win = tied[ctr % len(tied)]
            ctr += 1
        out.append(win)
        rc[win] += int(P["add_cpu"]); rm[win] += int(P["add_mem"]); zc[win] += pzc; zm[win] += pzm; cnt[win] += 1
    return np.array(out, np.int32), ctr


def _ref(cl, prios):
    return cpu_ref.run(cl, scheduler.make_config(fe.PREDS, prios), threads=2)


@pytest.mark.parametrize("name,cl,prios", CASES, ids=IDS)
def test_c_oracle_equals_python_restatement(name, cl, prios):
    ref, _, state, ctr = _ref(cl, prios)
    want, want_ctr = restate(cl, prios)
    assert np.array_equal(ref, want)
    assert ctr == want_ctr
    for k in ("req_cpu", "req_mem", "nz_cpu", "nz_mem"):
        assert not (state[k] >= 2 ** 48).any(), k  # the float64 kernels never hand over
    assert (ref >= 0).any()


@pytest.mark.parametrize("exact", [False, True], ids=["edge", "exact"])
@pytest.mark.parametrize("k", range(1, 10))
def test_lr_edge_first_placements_are_distinct(k, exact):
    """All n nodes tie at score k and each commit removes one from the tie set: the first n
    placements are n distinct nodes, so one wrong evaluation changes the sequence."""
    cl = fe.lr_edge_cluster(k, exact=exact)
    n = cl.n_nodes
    c = cl.cols
    for a, z in (("alloc_cpu", "nz_cpu"), ("alloc_mem", "nz_mem")):
        cap, t = c[a].astype(object), c[z].astype(object) + 1
        assert ((cap - t) * 10 // cap == k).all()
        assert ((cap - t - 1) * 10 // cap == k - 1).all()
    ref, _, _, _ = _ref(cl, fe.LR)
    assert len(set(ref[:n].tolist())) == n and (ref[:n] >= 0).all()


@pytest.mark.parametrize("exact", [False, True], ids=["edge", "exact"])
@pytest.mark.parametrize("k", range(1, 10))
def test_mr_edge_nodes_sit_on_the_smallest_total_scoring_k(k, exact):
    c = fe.mr_edge_cluster(k, exact=exact).cols
    for a, z in (("alloc_cpu", "nz_cpu"), ("alloc_mem", "nz_mem")):
        cap, t = c[a].astype(object), c[z].astype(object) + 1
        assert (t * 10 // cap == k).all() and ((t - 1) * 10 // cap == k - 1).all()


@pytest.mark.parametrize("k", range(1, 10))
def test_exact_clusters_need_the_remainder_correction(k):
    """In the exact clusters half the nodes sit on totals whose float64 quotient estimate
    truncates to k - 1 (only the exact remainder restores k) in both resources, and the other half
    on totals that need no correction: a floor division without it breaks the tie set."""
    assert len([c for c in fe.EXACT_POOL if fe.truncates_low(c, k)]) >= 8
    for cl, num in ((fe.lr_edge_cluster(k, exact=True), lambda cap, t: cap - t), (fe.mr_edge_cluster(k, exact=True), lambda cap, t: t)):
        c = cl.cols
        low = np.zeros((2, cl.n_nodes), bool)
        for j, (a, z) in enumerate((("alloc_cpu", "nz_cpu"), ("alloc_mem", "nz_mem"))):
            for i in range(cl.n_nodes):
                cap, x = int(c[a][i]), num(int(c[a][i]), int(c[z][i]) + 1) * 10
                assert x // cap == k
                low[j, i] = int(float(x) * (1.0 / float(cap))) < k
        assert low[:, 0::2].all() and not low[:, 1::2].any()


def test_bra_groups_tie_at_their_score():
    groups = fe.bra_ulp_clusters()
    assert len({s for s, _ in groups}) >= 9
    seen = set()
    for s, cl in groups:
        c = cl.cols
        assert 65 <= cl.n_nodes <= 300
        for i in range(cl.n_nodes):
            row = (int(c["alloc_cpu"][i]), int(c["alloc_mem"][i]), int(c["nz_cpu"][i]) + 1, int(c["nz_mem"][i]) + 1)
            assert fe.bra_score(row[2], row[0], row[3], row[1]) == s
            seen.add(row)
    assert seen == set(fe.ulp_family())  # every combination is in some group cluster


def test_ulp_family_is_one_ulp_sensitive():
    """The family separates a correctly rounded quotient from a merely faithful one: for at least
    1,000 combinations one ulp on either fraction changes the truncated score, and for some the
    float64 result differs from the exact rational's."""
    def score(fc, fm):
        return int((1.0 - abs(fc - fm)) * 10.0)
    sensitive = inexact = 0
    for cc, cm, tc, tm in fe.ulp_family():
        fc, fm = float(tc) / float(cc), float(tm) / float(cm)
        s = score(fc, fm)
        near = [(math.nextafter(fc, d), fm) for d in (0.0, 2.0)] + [(fc, math.nextafter(fm, d)) for d in (0.0, 2.0)]
        sensitive += any(score(a, b) != s for a, b in near)
        inexact += s != 10 - abs(tc * 10 // cc - tm * 10 // cm)
    assert sensitive >= 1000
    assert inexact >= 100


def test_degenerate_cluster_places_and_fails():
    cl = fe.degenerate_cluster()
    c = cl.cols
    assert (c["alloc_cpu"] == 0).any() and (c["alloc_mem"] == 0).any() and ((c["alloc_cpu"] == 0) & (c["alloc_mem"] == 0)).any()
    assert ((c["alloc_cpu"] == 1) & (c["alloc_mem"] == 1)).any()
    assert (c["nz_cpu"] + 1 == c["alloc_cpu"]).any() and (c["nz_mem"] + 1 == c["alloc_mem"]).any()
    assert (c["flags"] & abi.N_MEM_PRESSURE).any() and (c["flags"] & abi.N_NOT_READY).any()
    ref, reasons, _, _ = _ref(cl, fe.LR_MR_BRA)
    assert (ref >= 0).sum() >= 100 and (ref < 0).sum() >= 10
    assert (reasons[ref < 0].sum(axis=1) >= cl.n_nodes).all()  # every node gives a reason
    be = (cl.pods["flags"] & abi.POD_BEST_EFFORT) != 0
    assert (ref[be] >= 0).any() and (ref[~be] >= 0).any()


def test_clusters_stay_small():
    for name, cl, _ in CASES:
        assert 65 <= cl.n_nodes <= 300, name
        assert len(cl.pods) <= 3 * cl.n_nodes, name
