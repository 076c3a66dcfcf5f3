"""CPU-only tests of the drain sweep (ksim_sweep_drain, include/ksim_drain.h): the header as plain C,
the export beside an unchanged ksim.h / ksim_whatif.h ABI, the binding, the new methods' signatures,
default_evictable and requeue_copy, the argument checks that need no device, and — under the C
oracle — the properties of the inputs that tests/test_gpu_sweep_drain.py relies on, so that a later
edit of a builder cannot hollow those cases out."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import drain_inputs as D
from ksim import abi, scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ksim_drain.h")
FN = re.compile(r"^\s*(?:int|void|const char\*)\s+(ksim_\w+)\(", re.M)


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_header_compiles_as_plain_c(tmp_path, std):
    src = tmp_path / "t.c"
    src.write_text('#include "ksim_drain.h"\n'
                   'int main(void) {\n'
                   '  int64_t off[3] = {0, 1, 1}, pod[1] = {0};\n'
                   '  int32_t out[1], rehosted[2];\n'
                   '  ksim_sweep_requeue rq;\n'
                   '  ksim_sweep_failures f;\n'
                   '  rq.off = off; rq.pod = pod; rq.out_node = out;\n'
                   '  f.cap = 0; f.count = 0; f.listed = 0; f.pod = 0; f.hist = 0;\n'
                   '  return ksim_sweep_drain(0, 0, 2, &rq, 0, 0, 0, 0, 0, rehosted, &f, 0) == KSIM_E_INVAL ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["cc", "-std=" + std, "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                   check=True)


def test_header_declares_one_function_and_states_the_semantics():
    src = open(HEADER).read()
    assert '#include "ksim.h"' in src and '#include "ksim_whatif.h"' in src and 'extern "C"' in src
    assert FN.findall(src) == ["ksim_sweep_drain"]
    text = " ".join(src.replace("*", " ").split())
    for word in ("exactly ksim_sweep_nodes", "never evaluated or counted", "name order of the remaining nodes is unchanged",
                 "name ranks of the loaded table", "over the prefix pods too", "scenario's own columns",
                 "counter and error word are left untouched", "lists no node fails every pod, prefix included",
                 "always runs in the general form", "take no prefix queues", "count == 0 is allowed",
                 "scheduled once per appearance", "position in the scenario's own queue", "checked before the handle",
                 "KSIM_MAX_RCLASS", "node-sharded", "INT32_MAX", "spec.nodeName removed, status dropped"):
        assert word in text, word


def test_library_exports_the_entry_beside_an_unchanged_abi():
    L = abi.lib()
    assert hasattr(L, "ksim_sweep_drain") and len(L.ksim_sweep_drain.argtypes) == 12
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7
    assert len(abi.EXPORTS) == len(set(abi.EXPORTS)) == 33
    assert "ksim_sweep_drain" not in abi.EXPORTS
    assert "ksim_sweep_drain" not in open(os.path.join(INCLUDE, "ksim.h")).read()
    whatif = open(os.path.join(INCLUDE, "ksim_whatif.h")).read()
    assert "drain" not in whatif and FN.findall(whatif) == ["ksim_sweep_explain"]


def test_binding_mirrors_the_struct():
    r = abi.SweepRequeue
    assert [n for n, _ in r._fields_] == ["off", "pod", "out_node"]
    assert ctypes.sizeof(r) == 24 and (r.off.offset, r.pod.offset, r.out_node.offset) == (0, 8, 16)
    m = re.search(r"typedef struct ksim_sweep_requeue \{(.*?)\} ksim_sweep_requeue;", open(HEADER).read(), re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in r._fields_]


def test_signatures():
    d = inspect.signature(scheduler.GenericScheduler.sweep_drain).parameters
    assert list(d)[1:] == ["absent", "requeue", "first", "count", "explain"]
    assert (d["first"].default, d["count"].default, d["explain"].default) == (0, None, None)
    w = inspect.signature(scheduler.ClusterCapacity.drain_what_if).parameters
    assert list(w)[1:] == ["outages", "first", "count", "explain", "evictable"]
    assert (w["first"].default, w["count"].default, w["explain"].default, w["evictable"].default) == (0, None, False, None)
    # the existing surfaces keep their parameters
    assert list(inspect.signature(scheduler.GenericScheduler.sweep).parameters)[1:] == ["scenarios", "first", "count", "absent",
                                                                                       "explain"]
    assert list(inspect.signature(scheduler.ClusterCapacity.what_if).parameters)[1:] == ["outages", "first", "count", "explain"]
    assert "ksim_sweep_drain" in scheduler.GenericScheduler.sweep_drain.__doc__


def test_default_evictable_is_kubectl_drains_rule():
    ev = scheduler.default_evictable
    plain = {"metadata": {"name": "a"}, "spec": {"nodeName": "n"}, "status": {"phase": "Running"}}
    assert ev(plain) and ev({"metadata": {"name": "a"}, "spec": {}}) and ev({})
    assert ev({"metadata": {"ownerReferences": [{"kind": "ReplicaSet", "name": "r"}]}})
    assert not ev({"metadata": {"ownerReferences": [{"kind": "ReplicaSet"}, {"kind": "DaemonSet", "name": "d"}]}})
    assert not ev({"metadata": {"annotations": {"kubernetes.io/config.mirror": "abc"}}})
    assert ev({"metadata": {"annotations": {"other": "x"}, "ownerReferences": None}})
    assert not ev({"status": {"phase": "Succeeded"}}) and not ev({"status": {"phase": "Failed"}})
    assert ev({"status": {"phase": "Pending"}})


def test_requeue_copy_strips_node_name_and_status_only():
    pod = {"metadata": {"name": "a", "labels": {"app": "x"}, "ownerReferences": [{"kind": "ReplicaSet", "name": "r"}]},
           "spec": {"nodeName": "n1", "nodeSelector": {"tier": "a"}, "tolerations": [{"key": "k"}],
                    "containers": [{"ports": [{"hostPort": 80}], "resources": {"requests": {"cpu": "1"}}}]},
           "status": {"phase": "Running", "hostIP": "10.0.0.1"}}
    keep = repr(pod)
    new = scheduler.requeue_copy(pod)
    assert repr(pod) == keep  # the argument is left alone
    assert "status" not in new and "nodeName" not in new["spec"]
    want = {k: v for k, v in pod.items() if k != "status"}
    want["spec"] = {k: v for k, v in pod["spec"].items() if k != "nodeName"}
    assert new == want
    new["spec"]["containers"][0]["ports"][0]["hostPort"] = 81  # a deep copy
    assert pod["spec"]["containers"][0]["ports"][0]["hostPort"] == 80
    assert scheduler.requeue_copy({"metadata": {"name": "b"}}) == {"metadata": {"name": "b"}}


def _call(rq, n_scen=2, first=0, count=1, out=True, fail=None):
    L = abi.lib()
    o = np.zeros(8, np.int32)
    rc = L.ksim_sweep_drain(None, None, n_scen, ctypes.byref(rq) if rq is not None else None, first, count,
                            abi.vptr(o) if out else None, None, None, None, ctypes.byref(fail) if fail is not None else None,
                            None)
    return rc, L.ksim_last_error(None).decode()


def _rq(off, pod=True, out=True):
    off = np.asarray(off, np.int64)
    a, b = np.zeros(8, np.int64), np.zeros(8, np.int32)
    rq = abi.SweepRequeue(abi.ptr(off, ctypes.c_int64), abi.ptr(a, ctypes.c_int64) if pod else None,
                          abi.ptr(b, ctypes.c_int32) if out else None)
    rq._keep = (off, a, b)
    return rq


@pytest.mark.parametrize("case,what", [
    ("no-rq", "null re-queue lists"), ("no-off", "null re-queue lists"), ("off0", r"off\[0\] must be 0"),
    ("decreasing", "off decreases at scenario 1"), ("no-pod", "without a pod or out_node array"),
    ("no-out", "without a pod or out_node array"), ("too-long", "the queue of scenario 1 exceeds INT32_MAX pods"),
    ("nothing", "neither re-queued pods nor a pod range"), ("no-scenarios", "bad scenario count or pod range"),
    ("negative-count", "bad scenario count or pod range"), ("negative-cap", "a negative record cap"),
    ("cap-without-arrays", "a cap without record arrays")])
def test_argument_errors_that_need_no_device(case, what):
    """Each is KSIM_E_INVAL under the function's name, checked before the handle (here NULL)."""
    args = dict(rq=_rq([0, 1, 2]))
    if case == "no-rq":
        args["rq"] = None
    elif case == "no-off":
        args["rq"] = abi.SweepRequeue(None, None, None)
    elif case == "off0":
        args["rq"] = _rq([1, 1, 2])
    elif case == "decreasing":
        args["rq"] = _rq([0, 2, 1])
    elif case == "no-pod":
        args["rq"] = _rq([0, 1, 2], pod=False)
    elif case == "no-out":
        args["rq"] = _rq([0, 1, 2], out=False)
    elif case == "too-long":
        args.update(rq=_rq([0, 1, 2**31 - 1]), count=2)  # m_1 + count = 2^31 - 2 + 2 > INT32_MAX
    elif case == "nothing":
        args.update(rq=_rq([0, 0, 0], pod=False, out=False), count=0, out=False)
    elif case == "no-scenarios":
        args["n_scen"] = 0
    elif case == "negative-count":
        args["count"] = -1
    else:
        a = np.zeros(4 * abi.NREASONS, np.int32)
        p = abi.ptr(a, ctypes.c_int32)
        args["fail"] = abi.SweepFailures(-1, p, p, p, p) if case == "negative-cap" else abi.SweepFailures(4, p, p, None, p)
    rc, msg = _call(**args)
    assert rc == abi.E_INVAL and msg.startswith("ksim_sweep_drain: ") and re.search(what, msg), msg


def test_well_formed_lists_reach_the_handle_check():
    """m_s + count == INT32_MAX is allowed; the next check is the NULL handle's."""
    rc, msg = _call(_rq([0, 1, 2**31 - 2]), count=2)
    assert rc == abi.E_INVAL and msg == "ksim_sweep_drain: null argument"
    rc, msg = _call(_rq([0, 0, 1]), count=0, out=False)  # count == 0 needs no out_node
    assert rc == abi.E_INVAL and msg == "ksim_sweep_drain: null argument"
    rc, msg = _call(_rq([0, 0, 1]), count=1, out=False)
    assert rc == abi.E_INVAL and msg == "ksim_sweep_drain: null argument"


# ---- the inputs of tests/test_gpu_sweep_drain.py under the C oracle
def _row(r, r0):
    back = int((r["pre"] >= 0).sum())
    return (r["listed"], r["m"], back, r["m"] - back, int((r["out"] < 0).sum()), int((r0["out"] < 0).sum()), r["counter"])


def _prefix_slots(r):
    return np.nonzero(r["hist"][r["pod"] < r["m"]].sum(0))[0].tolist()


# label: (listed nodes, evicted, re-hosted, stranded, queue failures with re-queue, in the plain outage, final counter)
PINNED = {
    (130, 420, 300): {"first": (129, 2, 2, 0, 49, 46, 64), "none": (130, 0, 0, 0, 46, 46, 68),
                      "last": (129, 2, 2, 0, 48, 46, 68), "word-edge": (128, 3, 3, 0, 48, 49, 68),
                      "random-10pct": (117, 27, 27, 0, 80, 58, 61), "random-third": (87, 92, 52, 40, 112, 65, 51),
                      "tier-a": (94, 80, 47, 33, 111, 65, 49), "tier-b": (80, 122, 50, 72, 117, 69, 45),
                      "tier-c": (86, 98, 42, 56, 114, 73, 44), "all-but-5-7": (2, 296, 2, 294, 120, 118, 0),
                      "every-node": (0, 300, 0, 300, 120, 120, 0)},
    (65, 210, 150): {"first": (64, 2, 2, 0, 24, 23, 34), "none": (65, 0, 0, 0, 23, 23, 34),
                     "last": (64, 2, 2, 0, 25, 23, 34), "word-edge": (63, 2, 2, 0, 25, 24, 33),
                     "random-10pct": (59, 12, 8, 4, 38, 30, 22), "random-third": (44, 51, 20, 31, 51, 34, 20),
                     "tier-a": (50, 36, 13, 23, 46, 28, 22), "tier-b": (44, 44, 16, 28, 53, 37, 16),
                     "tier-c": (36, 69, 21, 48, 56, 38, 19), "all-but-5-7": (2, 144, 0, 144, 60, 60, 0),
                     "every-node": (0, 149, 0, 149, 60, 60, 0)},
    (1100, 3600, 2600): {"first": (1099, 2, 2, 0, 413, 411, 570), "none": (1100, 0, 0, 0, 411, 411, 571),
                         "last": (1099, 2, 2, 0, 416, 411, 566), "word-edge": (1098, 6, 6, 0, 422, 411, 572),
                         "1023-1024": (1098, 2, 2, 0, 416, 413, 571), "random-10pct": (990, 262, 262, 0, 695, 464, 556),
                         "random-third": (734, 851, 387, 464, 957, 578, 417), "tier-a": (742, 857, 409, 448, 980, 581, 416),
                         "tier-b": (731, 891, 361, 530, 964, 604, 387), "tier-c": (727, 852, 376, 476, 960, 609, 405),
                         "all-but-5-7": (2, 2598, 5, 2593, 1000, 995, 0), "every-node": (0, 2600, 0, 2600, 1000, 1000, 0)},
}


@pytest.mark.parametrize("n,p,R", D.SIZES)
def test_recipe_gives_the_pinned_outcomes(n, p, R):
    cl, Q, sets_, refs, plain = D.refs(n, p, R)
    _, _, host = D.cluster(n, p, R)
    running = {(130, 420, 300): 300, (65, 210, 150): 149, (1100, 3600, 2600): 2600}[(n, p, R)]
    assert cl.n_nodes == n and len(host) == running and Q == p - R and len(cl.pods) == Q + running
    assert int((cl.pods["port_cnt"][:Q] > 0).sum()) > 0 and int((cl.pods["port_cnt"][Q:] > 0).sum()) > 0
    assert [label for label, _ in sets_] == list(PINNED[(n, p, R)])
    for (label, a), r, r0 in zip(sets_, refs, plain):
        assert _row(r, r0) == PINNED[(n, p, R)][label], label
        assert r["listed"] == n - len(a) and np.array_equal(r["requeue"], D.requeue_of(n, p, R, a)), label
        assert r["count"] == int((r["pre"] < 0).sum()) + int((r["out"] < 0).sum()), label
    # what the GPU cases rely on
    both = [label for (label, _), r in zip(sets_, refs) if 0 < int((r["pre"] >= 0).sum()) < r["m"]]
    assert len(both) >= 1  # a scenario both strands and re-hosts prefix pods
    differ = [label for (label, _), r, r0 in zip(sets_, refs, plain) if not np.array_equal(r["out"], r0["out"])]
    assert len(differ) >= 5  # a sweep that ignored the prefix fails
    ms = [r["m"] for r in refs]
    assert any(ms[k] == 0 and ms[k - 1] > 0 and ms[k + 1] > 0 for k in range(1, len(ms) - 1))  # an empty prefix between two
    seen = [set(r["requeue"].tolist()) for r in refs]
    assert any(seen[i] & seen[j] for i in range(len(seen)) for j in range(i))  # a pod index shared by two scenarios
    slots = set()
    for r in refs:
        slots |= set(_prefix_slots(r))
    assert len(slots) >= 5, slots  # the stranded pods' reasons
    every = refs[[label for label, _ in sets_].index("every-node")]
    assert (every["pre"] == -1).all() and (every["out"] == -1).all() and every["counter"] == 0 and not every["hist"].any()
    assert np.array_equal(every["pod"], np.arange(every["m"] + Q))


def test_stranded_pods_reach_seven_reason_slots_at_130():
    _, _, sets_, refs, _ = D.refs(130, 420, 300)
    slots = set()
    for (label, _), r in zip(sets_, refs):
        if label.startswith("tier-"):
            slots |= set(_prefix_slots(r))
    assert sorted(slots) == [0, 4, 5, 6, 10, 11, 12]


@pytest.mark.parametrize("strip", ["queue", "prefix"])
def test_stripped_variants_keep_the_other_part_general(strip):
    n, p, R = 130, 420, 300
    cl, Q, _ = D.cluster(n, p, R, strip)
    part = cl.pods[:Q] if strip == "queue" else cl.pods[Q:]
    other = cl.pods[Q:] if strip == "queue" else cl.pods[:Q]
    assert not part["port_cnt"].any() and not (part["flags"] & abi.POD_NEED_SELECTOR).any()
    assert other["port_cnt"].any() and (other["flags"] & abi.POD_NEED_SELECTOR).any()
    tier_a = dict((label, a) for label, a in D.all_sets(n, p, R))["tier-a"]
    r, full = D.oracle(n, p, R, tier_a, strip=strip), D.oracle(n, p, R, tier_a)
    assert 0 < int((r["pre"] >= 0).sum()) < r["m"] and 0 < int((r["out"] >= 0).sum()) < Q
    assert not (np.array_equal(r["pre"], full["pre"]) and np.array_equal(r["out"], full["out"]))  # stripping changes the run
