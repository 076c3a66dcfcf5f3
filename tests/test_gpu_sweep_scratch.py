"""One scheduler carried through every sweep form in a row (tests/sweep_scratch_inputs.py): the scan
and general forms share one scratch slot of the handle, which is first small (scan), then outgrown
(general), reused at the larger size (scan again), outgrown once more (drain, with its prefix queues)
and reused (general again); the tree form keeps a slot of its own in between.  Every answer must be,
bit for bit, that of a fresh scheduler that makes only that call, and the handle's own state must come
out untouched.  KSIM_SWEEP_CHUNK=2 over five scenarios: three launches, the last one ragged."""
import numpy as np
import pytest

import cpu_ref
import sweep_scratch_inputs as I
from ksim import abi, scheduler

pytestmark = pytest.mark.gpu

FAST, GENERAL, CAP = I.FAST, I.GENERAL, I.CAP


def _new():
    preds, prios = scheduler.provider("DefaultProvider")
    return scheduler.GenericScheduler(I.cluster(), preds, prios, collect_reasons=False)


def _fast(g, monkeypatch, scan):
    if scan:
        monkeypatch.setenv("KSIM_SWEEP_SCAN", "1")
    else:
        monkeypatch.delenv("KSIM_SWEEP_SCAN", raising=False)
    out, ctr, st = g.sweep(None, 0, FAST, absent=I.node_sets())
    return dict(out=out, ctr=ctr, bound=g.last_scheduled.copy()), st


def _general(g, monkeypatch):
    monkeypatch.delenv("KSIM_SWEEP_SCAN", raising=False)
    out, ctr, st = g.sweep(None, FAST, GENERAL, absent=I.node_sets(), explain=CAP)
    return dict(out=out, ctr=ctr, bound=g.last_scheduled.copy(), **{k: v.copy() for k, v in g.last_failures.items()}), st


def _drain(g, monkeypatch):
    monkeypatch.delenv("KSIM_SWEEP_SCAN", raising=False)
    out, pre, ctr, st = g.sweep_drain(I.node_sets(), I.requeue(), FAST, GENERAL, explain=CAP)
    return dict(out=out, pre=np.concatenate(pre), ctr=ctr, bound=g.last_scheduled.copy(), rehosted=g.last_rehosted.copy(),
                **{k: v.copy() for k, v in g.last_failures.items()}), st


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (what, key)


def test_one_handle_through_every_form(monkeypatch):
    monkeypatch.setenv("KSIM_SWEEP_CHUNK", "2")
    calls = [("scan", lambda g: _fast(g, monkeypatch, True), abi.MODE_PERSISTENT),
             ("general", lambda g: _general(g, monkeypatch), abi.MODE_PERSISTENT),
             ("scan", lambda g: _fast(g, monkeypatch, True), abi.MODE_PERSISTENT),
             ("tree", lambda g: _fast(g, monkeypatch, False), abi.MODE_TREE),
             ("drain", lambda g: _drain(g, monkeypatch), abi.MODE_PERSISTENT),
             ("general", lambda g: _general(g, monkeypatch), abi.MODE_PERSISTENT)]
    fresh = {}
    for what, call, _ in calls:  # each call alone on a scheduler of its own
        if what not in fresh:
            g = _new()
            fresh[what], _ = call(g)
            g.close()
    g = _new()
    before, counter = g.node_state(), g.last_node_index
    got = []
    for k, (what, call, mode) in enumerate(calls):
        ans, st = call(g)
        got.append(ans)
        assert st.mode == mode, (k, what)
        assert st.blocks == 2 and st.kernel_launches == 3, (k, what, st.blocks, st.kernel_launches)
        _same(ans, fresh[what], (k, what))
    _same(got[0], got[2], "scan twice")
    _same(got[0], got[3], "scan and tree")
    # the sweeps are not vacuous: pods are placed, never on an absent node; losing the node the first
    # pod takes (the last one, on the untouched cluster) changes the answer; prefixes are placed
    for ans in got:
        assert (ans["bound"] > 0).all()
        for k, a in enumerate(I.node_sets()):
            assert not np.isin(ans["out"][k][ans["out"][k] >= 0], a).any()
    assert got[0]["out"][0][0] == I.N - 1 and got[0]["out"][2][0] not in (-1, I.N - 1)
    assert (got[1]["listed"] == [1100, 1099, 1099, 1098, 990]).all() and (got[4]["listed"] == got[1]["listed"]).all()
    assert (got[4]["pre"] >= 0).all() and (got[4]["rehosted"] == 2).all()
    after = g.node_state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert g.last_node_index == counter
    g.close()
    # the handle's scratch went with it: a new scheduler in this process works as ever
    monkeypatch.delenv("KSIM_SWEEP_CHUNK")
    g = _new()
    out, _, _ = g.schedule(0, FAST)
    ref, _, _, ctr = cpu_ref.run(I.cluster(), g.cfg, 0, FAST, threads=4, tables=g.tables, na_add=g.na_add)
    assert np.array_equal(out, ref) and g.last_node_index == ctr and (out >= 0).any()
    g.close()
