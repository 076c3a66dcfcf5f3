"""CPU-only tests of the affinity sweep (ksim_sweep_affinity, include/ksim_affsweep.h): the header as
plain C, the export beside an unchanged ABI, the binding, the argument checks that need no device,
and — on the oracles alone — the conditions that make the inputs of tests/test_gpu_sweep_affinity.py
discriminating (tests/affinity_sweep_inputs.py), so that a later edit of a builder cannot hollow those
cases out."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import affinity_sweep_inputs as A
from ksim import abi, scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ksim_affsweep.h")
FN = re.compile(r"^\s*(?:int|void|const char\*)\s+(ksim_\w+)\(", re.M)


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_plain_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "ksim_affsweep.h"\n'
                   'int main(void) {\n'
                   '  int32_t node[1] = {0}, ident[1] = {1}, cls[1] = {0}, out[2];\n'
                   '  ksim_sweep_residents res;\n'
                   '  res.n = 1; res.node = node; res.aff_ident = ident; res.aff_class = cls;\n'
                   '  return ksim_sweep_affinity(0, 0, 2, &res, 0, 0, 1, out, 0, 0, 0, 0, 0) == KSIM_E_INVAL ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["cc", "-std=" + std, "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                   check=True)


def test_header_declares_one_function_and_states_the_semantics():
    src = open(HEADER).read()
    assert '#include "ksim_drain.h"' in src and 'extern "C"' in src
    assert FN.findall(src) == ["ksim_sweep_affinity"]
    text = " ".join(src.replace("*", " ").split())
    for word in ("without the placed pods bound to them", "exactly as in ksim_sweep_drain", "rq == NULL: no prefixes",
                 "MatchInterPodAffinity, InterPodAffinityPriority and SelectorSpread included",
                 "counts, counter and error word are left untouched", "minus the contribution of every resident",
                 "nothing is taken out", "KSIM_E_INVAL naming the scenario", "Always the general form",
                 "Scenario weights are not taken", "checked before the device is touched", "no affinity tables loaded",
                 "KSIM_MAX_RCLASS", "KSIM_SWEEP_SPREAD_MAX_ZONES", "node-sharded", "KSIM_SWEEP_GENERAL_MAX_NODES",
                 "predate a node event"):
        assert word in text, word


def test_library_exports_the_entry_beside_an_unchanged_abi():
    L = abi.lib()
    assert hasattr(L, "ksim_sweep_affinity") and len(L.ksim_sweep_affinity.argtypes) == 13
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7
    assert len(abi.EXPORTS) == len(set(abi.EXPORTS)) == 33
    assert "ksim_sweep_affinity" not in abi.EXPORTS
    for name, fns in (("ksim_whatif.h", ["ksim_sweep_explain"]), ("ksim_drain.h", ["ksim_sweep_drain"])):
        src = open(os.path.join(INCLUDE, name)).read()
        assert "ksim_sweep_affinity" not in src and FN.findall(src) == fns
    assert "ksim_sweep_affinity" not in open(os.path.join(INCLUDE, "ksim.h")).read()


def test_binding_mirrors_the_struct():
    r = abi.SweepResidents
    assert [n for n, _ in r._fields_] == ["n", "node", "aff_ident", "aff_class"]
    assert ctypes.sizeof(r) == 32 and (r.n.offset, r.node.offset, r.aff_ident.offset, r.aff_class.offset) == (0, 8, 16, 24)
    m = re.search(r"typedef struct ksim_sweep_residents \{(.*?)\} ksim_sweep_residents;", open(HEADER).read(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in r._fields_]


def test_signatures():
    d = inspect.signature(scheduler.GenericScheduler.sweep_affinity).parameters
    assert list(d)[1:] == ["absent", "requeue", "first", "count", "explain", "bound"]
    assert (d["requeue"].default, d["first"].default, d["count"].default, d["explain"].default, d["bound"].default) == \
        (None, 0, None, None, ())
    # the existing surfaces keep their parameters
    assert list(inspect.signature(scheduler.GenericScheduler.sweep).parameters)[1:] == ["scenarios", "first", "count", "absent",
                                                                                       "explain"]
    assert list(inspect.signature(scheduler.GenericScheduler.sweep_drain).parameters)[1:] == ["absent", "requeue", "first",
                                                                                             "count", "explain"]
    assert "ksim_sweep_affinity" in scheduler.GenericScheduler.sweep_affinity.__doc__


def _call(n_scen=2, rq=None, first=0, count=1, out=True, fail=None):
    L = abi.lib()
    o = np.zeros(8, np.int32)
    rc = L.ksim_sweep_affinity(None, None, n_scen, None, ctypes.byref(rq) if rq is not None else None, first, count,
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
    assert rc == abi.E_INVAL and msg.startswith("ksim_sweep_affinity: ") and re.search(what, msg), msg


def test_cluster_keeps_the_running_pods_residents():
    inp = A.rnd_input(18)
    cl = inp.cluster()
    res = cl.residents
    assert res.dtype == np.int32 and res.shape[1] == 3 and 0 < len(res) <= len(inp.running)
    assert ((res[:, 1] > 0) | (res[:, 2] > 0)).all()
    assert (res[:, 0] >= 0).all() and (res[:, 0] < cl.n_nodes).all()
    assert res[:, 1].max() <= cl.affinity["n_ident"] and res[:, 2].max() <= cl.affinity["n_aclass"]
    # the counts the tables load are those of the residents: taking all of them out leaves zero
    t = cl.affinity
    cnt = t["cnt"].copy()
    for w, ident, _ in res:
        for c, (s, k) in enumerate(zip(t["pair_sel"].tolist(), t["pair_key"].tolist())):
            if ident > 0 and (int(t["ident_sel"][ident - 1, s >> 6]) >> (s & 63)) & 1 and t["dom"][k, w] >= 0:
                cnt[t["pair_off"][c] + t["dom"][k, w]] -= 1
    assert t["cnt"].any() and not cnt.any()


# ---- the conditions that make the inputs discriminating, on the oracles alone
@pytest.mark.parametrize("case", sorted(A.HAND))
def test_hand_cases_change_under_their_outage(case):
    """The reference's answer in the outage, and that it differs from the answer of a sweep whose
    counts still hold the lost pod (written out in A.HAND: the snapshot's answer, on the nodes left)."""
    inp = A.hand_input(case)
    cl = inp.cluster()
    _, _, _, want, naive = A.HAND[case]
    (_, none), (_, outage) = A.hand_sets(case)
    ref = A.oracle_ref(inp, outage)
    assert ref["out"].tolist() == [cl.index[want] if want else -1]
    assert want != naive
    whole = A.oracle_ref(inp, none)
    assert whole["out"].tolist() == [cl.index[naive] if naive else -1]  # uncorrected counts repeat the snapshot's answer
    c = A.oracle_cpu(inp, outage)
    assert np.array_equal(c["out"], ref["out"]) and c["counter"] == ref["counter"]
    if want is None:
        assert "didn't match pod affinity rules" in ref["msgs"][0][1]


@pytest.mark.parametrize("n_nodes", [n for n, _, _ in A.RND_SIZES])
def test_random_workloads_exercise_affinity_in_every_set(n_nodes):
    inp, sets_, refs = A.rnd_refs(n_nodes)
    labels = [label for label, _ in sets_]
    assert labels[:3] == ["none", "first", "last"] and sum(x.startswith("zone-") for x in labels) == 4
    # every one of the three inter-pod reasons occurs among the failed pods
    for bit in A.INTERPOD_REASONS:
        assert sum(int((r["hist"][:, bit] > 0).sum()) for r in refs) > 0, bit
    # in every set a placement changes when InterPodAffinityPriority is dropped from the policy
    plain = A.without_priority(inp)
    for (label, a), r in zip(sets_, refs):
        assert (A.oracle_cpu(plain, a)["out"] != r["out"]).any(), label
    # affinity-carrying running pods are lost in the zone sets
    assert sum(A.lost_affinity_pods(inp, a) for label, a in sets_ if label.startswith("zone-")) >= 5
    # the oracle's two forms agree (the table-level one checks the records and the large inputs)
    k = labels.index("zone-z1")
    o = A.oracle_ref(inp, sets_[k][1])
    assert np.array_equal(o["out"], refs[k]["out"]) and o["counter"] == refs[k]["counter"]
    scal = inp.cluster().scalar_names.items
    assert [scheduler.fit_error_message(refs[k]["listed"], h, scal) for h in refs[k]["hist"]] == [m for _, m in o["msgs"]]


def test_combined_inputs_carry_what_their_tests_need():
    import spread_sweep_inputs as X
    sp = A.spread_input()
    pods = np.asarray(sp.cluster().pods)
    t = sp.cluster().affinity
    both = (pods["aff_class"] > 0) & (t["spread_pair"][np.maximum(pods["aff_class"] - 1, 0)] >= 0) & \
        (t["ac"][np.maximum(pods["aff_class"] - 1, 0), 3] > 0)
    assert both.sum() >= 5  # pods that read both priorities in step 1b
    assert t["n_terms"] > 0 and sp.cluster().spread_active
    cls = A.classes_input()
    assert X.max_reduce_classes(cls.cluster()) > 1 and cls.cluster().affinity["n_terms"] > 0
