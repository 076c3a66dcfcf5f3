"""CPU-only tests of the volume sweep (ksim_sweep_volumes, include/ksim_volsweep.h): the header as plain
C, the export beside an unchanged ABI, the binding, the argument checks that need no device, and — on
the oracles alone — the conditions that make the inputs of tests/test_gpu_sweep_volumes.py
discriminating (tests/volume_sweep_inputs.py), so that a later edit of a builder cannot hollow those
cases out."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import volume_sweep_inputs as V
from ksim import abi, scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ksim_volsweep.h")
FN = re.compile(r"^\s*(?:int|void|const char\*)\s+(ksim_\w+)\(", re.M)


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_plain_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "ksim_volsweep.h"\n'
                   'int main(void) {\n'
                   '  int32_t node[1] = {0}, ident[1] = {1}, cls[1] = {0}, out[2];\n'
                   '  ksim_sweep_residents res;\n'
                   '  res.n = 1; res.node = node; res.aff_ident = ident; res.aff_class = cls;\n'
                   '  return ksim_sweep_volumes(0, 0, 2, &res, 0, 0, 1, out, 0, 0, 0, 0, 0) == KSIM_E_INVAL ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["cc", "-std=" + std, "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                   check=True)


def test_header_declares_one_function_and_states_the_semantics():
    src = open(HEADER).read()
    for h in ("ksim.h", "ksim_whatif.h", "ksim_drain.h", "ksim_affsweep.h"):
        assert '#include "%s"' % h in src
    assert 'extern "C"' in src and "typedef" not in src
    assert FN.findall(src) == ["ksim_sweep_volumes"]
    text = " ".join(src.replace("*", " ").split())
    for word in ("without the placed pods bound to them", "exactly as in ksim_sweep_drain", "rq == NULL: no prefixes",
                 "NoDiskConflict, the three MaxPD filters and NoVolumeZoneConflict",
                 "starts from the handle's current mounts", "carries that prefix's mounts", "its mounts are never read",
                 "counts, counter and error word are left untouched", "exactly as in ksim_sweep_affinity",
                 "Always the general form", "Scenario weights are not taken", "checked before the device is touched",
                 "KSIM_E_OVERFLOW", "the next call starts from a cleared word", "no volume tables loaded", "KSIM_MAX_RCLASS",
                 "KSIM_SWEEP_SPREAD_MAX_ZONES", "node-sharded", "KSIM_SWEEP_GENERAL_MAX_NODES", "predate a node event",
                 "27-bit score"):
        assert word in text, word


def test_library_exports_the_entry_beside_an_unchanged_abi():
    L = abi.lib()
    assert hasattr(L, "ksim_sweep_volumes") and len(L.ksim_sweep_volumes.argtypes) == 13
    assert L.ksim_sweep_volumes.argtypes == L.ksim_sweep_affinity.argtypes
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7
    assert len(abi.EXPORTS) == len(set(abi.EXPORTS)) == 33
    assert "ksim_sweep_volumes" not in abi.EXPORTS
    for name, fns in (("ksim_whatif.h", ["ksim_sweep_explain"]), ("ksim_drain.h", ["ksim_sweep_drain"]),
                      ("ksim_affsweep.h", ["ksim_sweep_affinity"])):
        src = open(os.path.join(INCLUDE, name)).read()
        assert "ksim_sweep_volumes" not in src and FN.findall(src) == fns
    assert "ksim_sweep_volumes" not in open(os.path.join(INCLUDE, "ksim.h")).read()


def test_signatures():
    d = inspect.signature(scheduler.GenericScheduler.sweep_volumes).parameters
    assert list(d)[1:] == ["absent", "requeue", "first", "count", "explain", "bound"]
    assert (d["requeue"].default, d["first"].default, d["count"].default, d["explain"].default, d["bound"].default) == \
        (None, 0, None, None, ())
    # the existing surfaces keep their parameters
    assert list(inspect.signature(scheduler.GenericScheduler.sweep_affinity).parameters) == list(d)
    assert list(inspect.signature(scheduler.GenericScheduler.sweep).parameters)[1:] == ["scenarios", "first", "count", "absent",
                                                                                       "explain"]
    assert list(inspect.signature(scheduler.GenericScheduler.sweep_drain).parameters)[1:] == ["absent", "requeue", "first",
                                                                                             "count", "explain"]
    assert "ksim_sweep_volumes" in scheduler.GenericScheduler.sweep_volumes.__doc__
    for f in (scheduler.ClusterCapacity.what_if, scheduler.ClusterCapacity.drain_what_if):
        doc = " ".join(f.__doc__.split())
        assert "GenericScheduler.sweep_volumes" in doc and "volume state are refused" not in doc


def _call(n_scen=2, rq=None, first=0, count=1, out=True, fail=None):
    L = abi.lib()
    o = np.zeros(8, np.int32)
    rc = L.ksim_sweep_volumes(None, None, n_scen, None, ctypes.byref(rq) if rq is not None else None, first, count,
                              abi.vptr(o) if out else None, None, None, None,
                              ctypes.byref(fail) if fail is not None else None, None)
    return rc, L.ksim_last_error(None).decode()


@pytest.mark.parametrize("case,what", [
    ("no-scenarios", "bad scenario count or pod range"), ("no-range-no-rq", "bad scenario count or pod range"),
    ("negative-first", "bad scenario count or pod range"), ("no-off", "null re-queue lists"),
    ("no-out", "null argument"), ("negative-cap", "a negative record cap"), ("null-handle", "null argument")])
def test_argument_errors_that_need_no_device(case, what):
    """Each is KSIM_E_INVAL under the function's name, checked before the handle (here NULL)."""
    args = {}
    if case == "no-scenarios":
        args["n_scen"] = 0
    elif case == "no-range-no-rq":
        args["count"] = 0
    elif case == "negative-first":
        args["first"] = -1
    elif case == "no-off":
        args["rq"] = abi.SweepRequeue(None, None, None)
    elif case == "no-out":
        args["out"] = False
    elif case == "negative-cap":
        args["fail"] = abi.SweepFailures(-1, None, None, None, None)
    rc, msg = _call(**args)
    assert rc == abi.E_INVAL and msg.startswith("ksim_sweep_volumes: ") and re.search(what, msg), msg


# ---- the conditions that make the inputs discriminating, on the oracles alone
@pytest.mark.parametrize("case", V.HAND)
def test_hand_cases_answer_as_written(case):
    """The reference's answers, set by set, are the ones written out in V.HAND_WANT; the two oracles
    agree; every case has an outage whose answer differs from the outage of nothing."""
    inp = V.hand_input(case)
    cl = inp.cluster()
    sets_ = V.hand_sets(case)
    assert sets_[0] == ("none", []) and len(sets_) == len(V.HAND_WANT[case]) and 2 <= cl.n_nodes <= 4
    answers = []
    for (label, a), want in zip(sets_, V.HAND_WANT[case]):
        ref, c = V.oracle_ref(inp, a), V.oracle_cpu(inp, a)
        assert np.array_equal(ref["out"], c["out"]) and ref["counter"] == c["counter"], label
        got = [(nm, cl.names[w] if w >= 0 else None) for nm, w in zip(ref["names"], ref["out"])]
        assert got == [(nm, w if isinstance(w, str) else None) for nm, w in want], label
        assert ref["msgs"] == [(nm, V.hand_message(ref["listed"], w)) for nm, w in want if not isinstance(w, str)], label
        answers.append(got)
    assert any(a != answers[0] for a in answers[1:])


def test_hand_cases_fail_with_the_three_messages():
    seen = {w for case in V.HAND for want in V.HAND_WANT[case] for _, w in want if not isinstance(w, str)}
    assert seen == set(V.VOLUME_REASONS)
    inp = V.hand_input("pv-zone")
    ref = V.oracle_ref(inp, V.hand_sets("pv-zone")[1][1])
    assert ref["msgs"] == [("q", "0/2 nodes are available: 2 node(s) had no available volume zone.")]


@pytest.mark.parametrize("case", V.DRAIN)
def test_drain_cases_on_the_reference(case):
    inp = V.drain_input(case)
    cl = inp.cluster()
    sets_ = [("none", []), ("n1", [cl.index["n1"]])]
    _, requeue, queues = V.drain_plan(inp, sets_)
    assert [len(r) for r in requeue] == [0, 1]
    ref = V.oracle_ref(inp, sets_[1][1], queue=queues[1] + inp.queue)
    if case == "rehost-keeps-off":
        none = V.oracle_ref(inp, [])
        host = int(ref["out"][0])
        assert host >= 0 and int(none["out"][0]) == host          # q alone would take the node that re-hosts r
        assert int(ref["out"][1]) >= 0 and int(ref["out"][1]) != host  # ... and is kept off it by r's disk
    else:
        assert int(ref["out"][0]) == -1 and ref["msgs"][0][1] == V.hand_message(2, abi.R_MAX_VOLUME_COUNT)


@pytest.mark.parametrize("n_nodes", sorted(V.RND))
def test_random_workloads_exercise_the_volume_predicates_in_every_set(n_nodes):
    seen = set()
    for zones in (False, True):
        inp, sets_, refs = V.rnd_refs(n_nodes, zones)
        assert 2 <= inp.max_vols <= 4
        labels = [label for label, _ in sets_]
        assert labels[:3] == ["none", "first", "last"] and labels[-2:] == ["tenth", "all"]
        assert sum(x.startswith("zone-") for x in labels) == (3 if zones else 0)
        assert len(sets_[-2][1]) == max(1, n_nodes // 10) and len(sets_[-1][1]) == n_nodes
        seen |= V.reasons_seen(refs)
        # in every set that lists a node a placement changes when the volume predicates are dropped
        plain = inp.without_volume_predicates()
        for (label, a), r in zip(sets_[:-1], refs):
            assert (V.oracle_cpu(plain, a)["out"] != r["out"]).any(), (zones, label)
            assert r["count"] >= 3, (zones, label)  # records with a cap of 2 are cut
        assert refs[-1]["count"] == len(inp.queue) and refs[-1]["listed"] == 0
    # every one of the three volume reasons occurs among the failed pods of this size
    assert seen == set(V.VOLUME_REASONS)
    # the oracle's two forms agree, with the FitError texts
    inp, sets_, refs = V.rnd_refs(n_nodes, True)
    if n_nodes == 16:
        k = 3
        o = V.oracle_ref(inp, sets_[k][1])
        assert np.array_equal(o["out"], refs[k]["out"]) and o["counter"] == refs[k]["counter"]
        scal = inp.cluster().scalar_names.items
        assert [scheduler.fit_error_message(refs[k]["listed"], h, scal) for h in refs[k]["hist"]] == [m for _, m in o["msgs"]]


def test_seeds_are_the_first_that_hold():
    assert all(t[2] == 0 for t in V.RND.values())


def test_geometry_and_combined_inputs_carry_what_their_tests_need():
    import spread_sweep_inputs as X
    for n in (1, 63, 64, 65, 1025):
        inp = V.geometry_input(n)
        cl = inp.cluster()
        assert cl.n_nodes == n and (np.asarray(cl.pods)["vol_class"] > 0).sum() >= 15
        ref = V.oracle_cpu(inp, [])
        assert (ref["out"] >= 0).any()
        if n > 1:
            assert (V.oracle_cpu(inp.without_volume_predicates(), [])["out"] != ref["out"]).any()
    mm = V.many_mounts_input()
    cl = mm.cluster()
    busy = cl.index["busy"]
    assert int(cl.volumes["slot_count"][busy]) >= 17
    ref = V.oracle_ref(mm, [])
    assert [cl.names[w] if w >= 0 else None for w in ref["out"]] == ["busy", "small", "busy", "small"]
    sp = V.spread_input()
    pods = np.asarray(sp.cluster().pods)
    assert sp.cluster().spread_active and sp.cluster().affinity["n_terms"] == 0
    assert ((pods["vol_class"] > 0) & (pods["aff_class"] > 0)).sum() >= 10
    af = V.affinity_input()
    pods = np.asarray(af.cluster().pods)
    assert af.cluster().affinity["n_terms"] > 0 and ((pods["vol_class"] > 0) & (pods["aff_class"] > 0)).sum() >= 10
    cls = V.classes_input()
    assert X.max_reduce_classes(cls.cluster()) > 1 and (np.asarray(cls.cluster().pods)["vol_class"] > 0).sum() >= 10
    # in each of them the volume predicates move a pod
    for inp in (sp, af, cls, V.caps_input()):
        assert (V.oracle_cpu(inp.without_volume_predicates(), [])["out"] != V.oracle_cpu(inp, [])["out"]).any()
