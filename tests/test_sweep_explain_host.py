"""CPU-only tests of the explained scenario sweep (ksim_sweep_explain, include/ksim_whatif.h): the
header as plain C, the export beside an unchanged ksim.h ABI, the binding and the `explain`
keywords, the argument check that needs no device, and — under the C oracle — the properties of
the inputs that tests/test_gpu_sweep_explain.py relies on, so that a later edit of a builder
cannot hollow those cases out."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import explain_inputs as E
from ksim import abi, scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ksim_whatif.h")


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_plain_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "ksim_whatif.h"\n'
                   'int main(void) {\n'
                   '  int32_t count[2], listed[2], pod[2 * 3], hist[2 * 3 * KSIM_NREASONS];\n'
                   '  ksim_sweep_failures f;\n'
                   '  f.cap = 3; f.count = count; f.listed = listed; f.pod = pod; f.hist = hist;\n'
                   '  return ksim_sweep_explain(0, 0, 0, 2, 0, 1, 0, 0, 0, &f, 0) == KSIM_E_INVAL ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["cc", "-std=" + std, "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                   check=True)


def test_header_includes_ksim_h_and_states_the_semantics():
    src = open(HEADER).read()
    assert '#include "ksim.h"' in src and 'extern "C"' in src
    text = " ".join(src.replace("*", " ").split())
    for word in ("bit for bit", "first failing predicate", "predicatesOrdering", "Absent nodes are not evaluated",
                 "listed[s] is n_nodes", "queue order", "left unwritten", "lists no node", "ErrNoNodesAvailable",
                 "fail == NULL or cap == 0", "KSIM_E_INVAL", "count - out_scheduled[s]"):
        assert word in text, word
    fns = re.findall(r"^\s*(?:int|void|const char\*)\s+(ksim_\w+)\(", src, re.M)
    assert fns == ["ksim_sweep_explain"]


def test_library_exports_the_entry_beside_an_unchanged_abi():
    L = abi.lib()
    assert hasattr(L, "ksim_sweep_explain")
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7
    assert len(abi.EXPORTS) == len(set(abi.EXPORTS)) == 33
    assert "ksim_sweep_explain" not in abi.EXPORTS
    assert "ksim_sweep_explain" not in open(os.path.join(INCLUDE, "ksim.h")).read()
    assert len(L.ksim_sweep_explain.argtypes) == 11


def test_binding_mirrors_the_struct():
    f = abi.SweepFailures
    assert [n for n, _ in f._fields_] == ["cap", "count", "listed", "pod", "hist"]
    assert ctypes.sizeof(f) == 40 and f.count.offset == 8 and f.hist.offset == 32
    m = re.search(r"typedef struct ksim_sweep_failures \{(.*?)\} ksim_sweep_failures;", open(HEADER).read(), re.S)
    assert re.findall(r"(\w+);", m.group(1)) == [n for n, _ in f._fields_]


def test_sweep_and_what_if_accept_explain():
    s = inspect.signature(scheduler.GenericScheduler.sweep).parameters
    assert list(s)[1:] == ["scenarios", "first", "count", "absent", "explain"] and s["explain"].default is None
    w = inspect.signature(scheduler.ClusterCapacity.what_if).parameters
    assert list(w)[1:] == ["outages", "first", "count", "explain"] and w["explain"].default is False
    assert "ksim_sweep_explain" in scheduler.GenericScheduler.sweep.__doc__


@pytest.mark.parametrize("cap,pod,hist", [(-1, True, True), (4, False, True), (4, True, False)])
def test_bad_record_arguments_are_refused_before_anything_else(cap, pod, hist):
    """cap < 0, or a cap without record arrays: KSIM_E_INVAL under the function's name (checked before
    the handle, so no device is needed)."""
    L = abi.lib()
    a = np.zeros(4 * abi.NREASONS, np.int32)
    f = abi.SweepFailures(cap, abi.ptr(a, ctypes.c_int32), abi.ptr(a, ctypes.c_int32),
                          abi.ptr(a, ctypes.c_int32) if pod else None, abi.ptr(a, ctypes.c_int32) if hist else None)
    assert L.ksim_sweep_explain(None, None, None, 1, 0, 1, None, None, None, ctypes.byref(f), None) == abi.E_INVAL
    assert L.ksim_last_error(None).decode().startswith("ksim_sweep_explain: a negative record cap")


# ---- the inputs of tests/test_gpu_sweep_explain.py under the C oracle
def _slots(r):
    return np.nonzero(r["hist"].sum(0))[0].tolist()


def test_general_input_fails_on_many_reasons_at_once():
    cl, sets_, refs = E.general_refs(1100, 3600)
    assert cl.n_nodes == 1100 and cl.n_nodes % 32 != 0 and cl.n_nodes > 1024  # two-row segments, ragged mask word
    assert int((cl.pods["port_cnt"] > 0).sum()) > 100  # not resource-only: the general form
    preds, prios = scheduler.provider("DefaultProvider")
    pl = scheduler.plan(cl, preds, prios)
    assert int((np.asarray(pl.tables["n_tt"]) * np.asarray(pl.tables["n_na"]))[cl.pods["cls"]].max()) == 2
    labels = [label for label, _ in sets_]
    assert labels == ["none", "first", "last", "word-edge", "1023-1024", "random-10pct", "all-but-5-7", "every-node"]
    r = refs[0]  # no node absent
    assert r["count"] == 408 and int(r["pod"][0]) == 2974
    assert _slots(r) == [abi.R_NOT_READY, abi.R_UNSCHEDULABLE, abi.R_PODS, abi.R_CPU, abi.R_MEMORY, abi.R_HOST_PORTS,
                         abi.R_NODE_SELECTOR, abi.R_TAINTS]
    assert len({h.tobytes() for h in r["hist"]}) == 364
    assert ((r["hist"] > 0).sum(1) >= 3).all() and (r["hist"].sum(1) > cl.n_nodes).all()  # several slots per node
    assert E.binds_after_failures(r["out"]) == 85
    for (label, a), r in zip(sets_, refs):
        assert r["listed"] == cl.n_nodes - len(a), label
        if label == "every-node":
            assert r["count"] == 3600 and not r["hist"].any()
            continue
        assert r["count"] >= 100, label
        assert len(_slots(r)) >= 6, label
        assert E.binds_after_failures(r["out"]) >= 1, label
        if label != "none":  # every set changes the answer
            assert not (r["count"] == refs[0]["count"] and np.array_equal(r["hist"], refs[0]["hist"])), label


@pytest.mark.parametrize("n,p,failed", [(130, 420, 46), (65, 210, 24)])
def test_small_general_inputs_fail_too(n, p, failed):
    """n = 130 and n = 65: waves without rows (three, two of sixteen hold any)."""
    cl, sets_, refs = E.general_refs(n, p)
    assert cl.n_nodes == n and refs[0]["count"] == failed
    for (label, a), r in zip(sets_, refs):
        if label != "every-node":
            assert 0 < r["count"] < p and len(_slots(r)) >= 4 and E.binds_after_failures(r["out"]) >= 1, label


def test_resource_only_input_has_long_runs_of_failures():
    cl, preds, prios = E.c3_cluster()
    assert cl.n_nodes == 1100 and len(cl.pods) == 60000
    # the whole queue under the reference, no node absent
    r = E.oracle(cl, None, None, scheduler.make_config(preds, prios), [])
    assert r["count"] == 26893 and int(r["pod"][0]) == 31130
    assert _slots(r) == [abi.R_CPU, abi.R_MEMORY]
    assert len({h.tobytes() for h in r["hist"]}) == 302
    assert E.binds_after_failures(r["out"]) == 961
    # The resource-only forms refuse the whole range (60,000 pods of up to 8 GiB could pass 2^48), so the
    # GPU cases schedule the first RES_FIRST pods, which all fit, and sweep the rest: the same failures
    pre, state, ctr = E.resource_prefix()
    assert E.RES_FIRST == 30000 and (pre >= 0).all() and np.array_equal(pre, r["out"][:E.RES_FIRST])
    qmax = int(max(cl.pods["req_mem"].max(), cl.pods["req_cpu"].max()))
    assert len(cl.pods) * qmax >= 2**48 > (len(cl.pods) - E.RES_FIRST) * qmax + int(cl.cols["alloc_mem"].max())
    cl, scen, sets_, refs = E.resource_refs(False)
    assert scen is None and [label for label, _ in sets_] == ["none", "first", "word-edge", "random-10pct", "every-node"]
    assert refs[0]["count"] == 26893 and int(refs[0]["pod"][0]) == 31130 - E.RES_FIRST
    assert np.array_equal(refs[0]["hist"], r["hist"]) and refs[0]["counter"] == r["counter"]
    crossing = []
    for (label, a), r in zip(sets_, refs):
        assert r["listed"] == cl.n_nodes - len(a), label
        assert r["count"] > 1000, label  # the GPU cases' cap of 1000 truncates every scenario
        if label == "every-node":
            continue
        assert _slots(r) == [abi.R_CPU, abi.R_MEMORY], label
        kept = r["pod"][:1000]
        # runs of consecutive failures (the tree form copies a class's last histogram) before the cap
        # and binds between them (the copy is dropped)
        runs = np.split(kept, np.nonzero(np.diff(kept) != 1)[0] + 1)
        assert max(len(x) for x in runs) >= 8 and len(runs) >= 50, label
        crossing.append(int(r["pod"][1000]) == int(r["pod"][999]) + 1)
    assert any(crossing) and not all(crossing)  # the cap falls inside a run of failures, and between two
    cl, scen, sets_, refs = E.resource_refs(True)
    assert len(scen) == 2 and all(not a for _, a in sets_)
    assert refs[0]["count"] == 26893 and refs[1]["count"] > 1000
    assert not np.array_equal(refs[0]["out"], refs[1]["out"])
    _, _, _, refs = E.resource_refs(False, 6000)
    assert all(r["count"] > 3000 for r in refs)


def test_nodename_input_fails_on_hostname_everywhere():
    cl, its_node = E.nodename_input()
    preds, prios = scheduler.provider("DefaultProvider")
    pl = scheduler.plan(cl, preds, prios)
    cfg = scheduler.make_config(preds, prios)
    assert int(cl.pods["host"][E.NODENAME_POD]) == its_node and int((cl.pods["host"] >= 0).sum()) == 1
    with_it, without = (E.oracle(cl, pl.tables, pl.na_add, cfg, a) for a in ([], [its_node]))
    assert with_it["out"][E.NODENAME_POD] == its_node and without["out"][E.NODENAME_POD] == -1
    k = int(np.nonzero(without["pod"] == E.NODENAME_POD)[0][0])
    assert int(without["hist"][k][abi.R_HOSTNAME]) == without["listed"] == cl.n_nodes - 1
