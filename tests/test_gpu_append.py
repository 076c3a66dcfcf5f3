"""ksim_append_pods (include/ksim.h) / GenericScheduler.append_pods: the queue grown call by call
— geometric regrowth of the device arrays with their contents kept, port and scalar offsets rebased
onto the arrays already loaded, the tree-class set extended (and the cached form and tree mode
turned off by a 65th class), the planned trees and the launch graph dropped — must schedule exactly
as the same queue loaded at once, checked against the oracles after every call."""
import copy
import ctypes as C

import numpy as np
import pytest

import cpu_ref
import ksim_ref as R
from ksim import abi, ingest, scheduler, synth
from workloads import rnd_workload

pytestmark = pytest.mark.gpu

STATE_KEYS = ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pod_count")
LR_BRA = [("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)]
# queue positions: the first load, one pod, 1,500 pods (25 classes), up to 64 classes, the 65th class, the rest
CUTS = [0, 500, 501, 2001, 2301, 2302, 2500]


def _resource_queue():
    """600 nodes; 2,500 pods whose distinct cpu requests (tree classes) number 5 in [0, 501),
    25 in [501, 2001), 64 in [2001, 2301), then one pod of a 65th and 198 more of all 65."""
    n, m = 600, CUTS[-1]
    cpu, mem = synth.c3_nodes(n, 71)
    r = synth.splitmix64(72, m)
    ncls = np.empty(m, np.int64)
    for lo, hi, k in ((0, 501, 5), (501, 2001, 25), (2001, 2301, 64), (2301, 2500, 65)):
        ncls[lo:hi] = k
    cls = (r % ncls.astype(np.uint64)).astype(np.int64)
    cls[501:526] = np.arange(25)     # every class of a batch occurs in it
    cls[2001:2065] = np.arange(64)
    cls[2301] = 64
    pcpu = 100 + 10 * cls
    i = np.arange(n, dtype=np.int64)
    allowed = ((i + 1) * 2300 // n - i * 2300 // n).astype(np.int32)  # the queue's tail overflows the cluster
    cl = synth.resource_cluster(["a-%04d" % k for k in range(n)], cpu, mem, allowed, pcpu, np.full(m, synth.GI, np.int64))
    assert len(set(pcpu[:501].tolist())) == 5 and len(set(pcpu[:2001].tolist())) == 25
    assert len(set(pcpu[:2301].tolist())) == 64 and len(set(pcpu[:2302].tolist())) == 65
    return cl


def _prefix(cl, k):
    c0 = copy.copy(cl)
    c0.pods = cl.pods[:k].copy()
    return c0


@pytest.mark.parametrize("mode", [abi.MODE_AUTO, abi.MODE_TREE], ids=["auto", "tree"])
def test_resource_queue_grown_by_appends(mode, monkeypatch):
    for k in ("KSIM_NO_PCACHE", "KSIM_FORCE_STREAM", "KSIM_NO_PFAST", "KSIM_MAX_GRID"):
        monkeypatch.delenv(k, raising=False)
    cl = _resource_queue()
    preds = list(scheduler.DEFAULT_PREDICATES)
    cfg = scheduler.make_config(preds, LR_BRA)
    g = scheduler.GenericScheduler(_prefix(cl, CUTS[1]), preds, LR_BRA, mode=mode)
    outs, rss = [], []

    def step(count, want):
        """Schedule the next `count` pods; everything so far equals the oracle's run of the prefix."""
        first = sum(len(o) for o in outs)
        o, r, st = g.schedule(first, count)
        outs.append(o)
        rss.append(r)
        ref, ref_rs, ref_state, ref_ctr = cpu_ref.run(cl, cfg, 0, first + count, threads=4)
        out = np.concatenate(outs)
        assert np.array_equal(out, ref)
        assert np.array_equal(np.concatenate(rss)[out < 0], ref_rs[out < 0])
        assert g.last_node_index == ref_ctr
        s = g.node_state()
        for k in STATE_KEYS:
            assert np.array_equal(s[k], ref_state[k]), k
        if mode == abi.MODE_TREE:
            assert (st.mode == abi.MODE_TREE) == (want == "cached")
        else:
            assert g.last_form & 7 == (5 if want == "cached" else 1), hex(g.last_form)
        return out

    try:
        step(300, "cached")
        g.append_pods(cl.pods[CUTS[1]:CUTS[2]])             # one pod: the arrays double (500 -> 1,000)
        g.append_pods(cl.pods[CUTS[2]:CUTS[3]])             # 1,500 pods, 25 classes: a second regrowth
        with pytest.raises(abi.KsimError):
            g.schedule(0, CUTS[3] + 1)                      # (the range check follows the queue)
        step(1000, "cached")                                # across the first load's end
        g.append_pods(cl.pods[:0])                          # nothing: accepted
        g.append_pods(cl.pods[CUTS[3]:CUTS[4]])             # up to 64 classes
        step(800, "cached")
        g.append_pods(cl.pods[CUTS[4]:CUTS[5]])             # the 65th class
        g.append_pods(cl.pods[CUTS[5]:CUTS[6]])
        out = step(CUTS[6] - 2100, "uncached")
        assert (out < 0).sum() >= 100 and len(out) == CUTS[6]
    finally:
        g.close()


@pytest.mark.parametrize("mode", [abi.MODE_AUTO, abi.MODE_LAUNCH], ids=["auto", "launch"])
@pytest.mark.parametrize("seed,split", [(3, 61), (9, 100)])
def test_feature_queue_split_with_its_own_port_and_scalar_arrays(seed, split, mode):
    """Host ports, selectors and extended requests: the second batch arrives with its own ports /
    scalars arrays and offsets relative to them; results equal the object oracle's."""
    nodes, running, pods = rnd_workload(seed, n_nodes=31, n_pods=150)
    preds, prios = scheduler.provider("DefaultProvider")
    want, want_lni = R.simulate(nodes, running, pods, set(preds), list(prios))
    cl = ingest.Cluster.from_objects(nodes, running, list(reversed(pods)))  # scheduling order (LIFO pop)
    allp = scheduler.plan(cl, preds, prios).pods                             # the descriptors as loaded
    K0, S0 = int(allp["port_off"][split]), int(allp["scalar_off"][split])
    assert 0 < K0 < len(cl.pod_ports) and 0 < S0 < len(cl.pod_scalars)       # both batches carry both kinds
    c0 = _prefix(cl, split)
    c0.pod_ports, c0.pod_scalars = cl.pod_ports[:K0].copy(), cl.pod_scalars[:S0].copy()
    g = scheduler.GenericScheduler(c0, preds, prios, mode=mode)
    try:
        o1, r1, _ = g.schedule(0, split - 20)
        tail = allp[split:].copy()
        tail["port_off"] -= K0
        tail["scalar_off"] -= S0
        g.append_pods(tail, cl.pod_ports[K0:].copy(), cl.pod_scalars[S0:].copy())
        o2, r2, _ = g.schedule(split - 20, len(pods) - split + 20)
        out, rs = np.concatenate([o1, o2]), np.concatenate([r1, r2])
        assert [cl.pod_names[k] for k in range(len(out))] == [name for name, _, _ in want]
        for k, (name, host, msg) in enumerate(want):
            if host is not None:
                assert out[k] >= 0 and cl.names[int(out[k])] == host, name
            else:
                assert out[k] < 0, name
                assert scheduler.fit_error_message(cl.n_nodes, rs[k], cl.scalar_names.items) == msg, name
        assert g.last_node_index == want_lni
        assert (out < 0).any() and (out >= 0).any()
    finally:
        g.close()


def test_append_error_paths():
    """KSIM_E_STATE before the class tables are loaded; KSIM_E_INVAL for a port or scalar range
    outside the arrays passed with the batch (and the queue is unchanged after the refusal)."""
    cl = _prefix(_resource_queue(), 10)
    preds = list(scheduler.DEFAULT_PREDICATES)
    h = abi.Handle(scheduler.make_config(preds, LR_BRA))
    try:
        table = cl.node_table()
        h.call("ksim_load_nodes", C.byref(table))
        with pytest.raises(abi.KsimError) as ei:
            h.call("ksim_append_pods", abi.vptr(cl.pods), len(cl.pods), None, 0, None, 0)
        assert ei.value.code == abi.E_STATE and "classes first" in str(ei.value)
    finally:
        h.close()
    g = scheduler.GenericScheduler(cl, preds, LR_BRA)
    try:
        ports = np.array([80, 81], np.uint64)
        for field, cnt in (("port_off", "port_cnt"), ("scalar_off", "scalar_cnt")):
            bad = cl.pods[:1].copy()
            bad[field], bad[cnt] = 1, 2
            with pytest.raises(abi.KsimError) as ei:
                g.append_pods(bad, ports, np.zeros(2, abi.SCALAR_DTYPE))
            assert ei.value.code == abi.E_INVAL and "out of bounds" in str(ei.value)
            bad[field] = -1
            with pytest.raises(abi.KsimError) as ei:
                g.append_pods(bad, ports, np.zeros(2, abi.SCALAR_DTYPE))
            assert ei.value.code == abi.E_INVAL
        with pytest.raises(abi.KsimError):
            g.schedule(0, 11)                    # still 10 pods
        out, _, _ = g.schedule(0, 10)
        ref, _, _, _ = cpu_ref.run(cl, scheduler.make_config(preds, LR_BRA), threads=1)
        assert np.array_equal(out, ref)
    finally:
        g.close()
