"""CPU-only tests of the scenario sweep over SelectorSpread queues: the zone cap mirrored in the
binding, the headers' account of what is swept and what is still refused, the unchanged C ABI, and
the properties of the inputs (tests/spread_sweep_inputs.py) that tests/test_gpu_sweep_spread.py relies
on, under the reference: the listers change the placements, in the whole cluster and in an outage, so
a sweep that dropped the spread priority could not pass."""
import os
import re

import numpy as np
import pytest

import spread_sweep_inputs as X
from ksim import abi, scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SWEEP_H = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc", "ksim_sweep.h")


def _text(name):
    return " ".join(open(os.path.join(INCLUDE, name)).read().replace("*", " ").split())


def test_zone_cap_is_mirrored_and_fits_the_lds():
    src = open(SWEEP_H).read()
    m = re.search(r"^#define\s+KSIM_SWEEP_SPREAD_MAX_ZONES\s+(\d+)", src, re.M)
    assert m and int(m.group(1)) == abi.SWEEP_SPREAD_MAX_ZONES >= 256
    # evaluations at the node cap + both buffers of 64-bit zone words + 1 KiB of reduction words in 160 KiB
    assert abi.SWEEP_GENERAL_MAX_NODES * 4 + 2 * abi.SWEEP_SPREAD_MAX_ZONES * 8 + 1024 <= 160 * 1024


def test_headers_name_what_is_swept_and_what_is_refused():
    sweep = _text("ksim.h")
    for word in ("SelectorSpread queues are swept", "KSIM_SWEEP_SPREAD_MAX_ZONES", "own copy of cnt",
                 "the handle's counts are not written", "a pod in the range with inter-pod affinity"):
        assert word in sweep, word
    drain = _text("ksim_drain.h")
    for word in ("SelectorSpread state alone is swept", "inter-pod affinity state", "KSIM_SWEEP_SPREAD_MAX_ZONES"):
        assert word in drain, word
    whatif = _text("ksim_whatif.h")
    assert "SelectorSpread queues" in whatif and "inter-pod affinity state is still refused" in whatif


def test_abi_is_unchanged():
    L = abi.lib()
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7
    assert len(abi.EXPORTS) == len(set(abi.EXPORTS)) == 33
    assert not any("spread" in name for name in abi.EXPORTS)


def _differs(refs, plain, sets_):
    """Placements that differ with the listers: in the unreduced cluster, and the most in an outage."""
    d = {label: int((a["out"] != b["out"]).sum()) for (label, _), a, b in zip(sets_, refs, plain)}
    outages = [v for k, v in d.items() if k not in ("none", "every-node")]
    return d["none"], max(outages)


@pytest.mark.parametrize("policy", sorted(X.POLICIES))
@pytest.mark.parametrize("zones", [True, False], ids=["zones", "no-zones"])
@pytest.mark.parametrize("n_nodes", [n for n, _ in X.RND_SIZES])
def test_listers_change_the_random_workloads(n_nodes, zones, policy):
    inp, sets_, refs = X.rnd_refs(n_nodes, zones, policy)
    _, _, plain = X.rnd_refs(n_nodes, zones, policy, False)
    labels = [label for label, _ in sets_]
    assert labels[:3] == ["none", "first", "last"] and labels[-1] == "every-node"
    assert ("all-zoned" in labels) == zones and sum(x.startswith("zone-") for x in labels) == (3 if zones else 0)
    whole, outage = _differs(refs, plain, sets_)
    assert whole > len(inp.queue) // 4 and outage > len(inp.queue) // 4
    # the oracle's two forms agree on it (the table-level one checks the records and the large inputs)
    k = labels.index("first")
    c = X.oracle_cpu(inp, policy, sets_[k][1])
    assert np.array_equal(c["out"], refs[k]["out"]) and c["counter"] == refs[k]["counter"]


def test_the_all_zoned_outage_leaves_no_zoned_node():
    for n, _ in X.RND_SIZES:
        inp, sets_, _ = X.rnd_refs(n, True, "default")
        cl = inp.cluster()
        gone = set(dict(sets_)["all-zoned"])
        left = [x for x in inp.nodes if cl.index[x["metadata"]["name"]] not in gone]
        assert left and len(left) < n and not any(X.ZONE in x["metadata"]["labels"] for x in left)
        assert any(X.ZONE in x["metadata"]["labels"] for x in inp.nodes)


@pytest.mark.parametrize("n", [1025, 2049])
def test_uniform_input_ties_widely(n):
    inp, sets_, refs = X.uniform_refs(n)
    _, _, plain = X.uniform_refs(n, False)
    whole, outage = _differs(refs, plain, sets_)
    assert whole > 200 and outage > 200
    assert n % 1024 == 1 and inp.cluster().n_nodes == n  # ragged two- and three-row segments
    none = refs[0]
    assert (none["out"] >= 0).all() and none["counter"] == len(inp.queue)  # more than one node fits every pod
    # the ties walk the segment positions: the placements spread over the whole name order
    assert none["out"].min() < 64 and none["out"].max() >= n - 64 and len(set(none["out"].tolist())) > 250


def test_classes_input_has_several_reduce_classes():
    inp, sets_, refs = X.classes_refs()
    assert X.max_reduce_classes(inp.cluster()) > 1
    _, _, plain = X.classes_refs(False)
    whole, outage = _differs(refs, plain, sets_)
    assert whole > 300 and outage > 300
    assert [label for label, _ in sets_] == ["none", "first", "zone-z2", "all-zoned"]


def test_overflow_input_meets_its_conditions():
    inp = X.overflow_input()
    sets_ = X.sets_of(inp.cluster())
    for label, a in sets_:
        if label == "every-node":
            continue
        ref = X.oracle_ref(inp, "default", a)
        plain = X.oracle_ref(inp, "default", a, with_listers=False)
        after, full_higher = X.overflow_conditions(inp, ref, a)
        assert after > 0 and full_higher > 0, label
        assert (ref["out"] < 0).sum() > 3 and (ref["out"] != plain["out"]).any(), label
        if label in ("none", "zone-z1"):
            assert after >= 20 and full_higher >= 20, label
            c = X.oracle_cpu(inp, "default", a)
            assert np.array_equal(c["out"], ref["out"]) and c["count"] == len(ref["msgs"])
            scal = inp.cluster().scalar_names.items
            assert [scheduler.fit_error_message(c["listed"], h, scal) for h in c["hist"]] == [m for _, m in ref["msgs"]]


def test_first_pod_input():
    inp = X.first_pod_input()
    cl = inp.cluster()
    assert not inp.running
    pods = np.asarray(cl.pods)
    lone = np.array([x["metadata"]["name"].startswith("lone") for x in inp.queue])
    assert lone.any() and (pods["aff_class"][lone] == 0).all() and (pods["aff_class"][~lone] > 0).all()
    sets_ = X.sets_of(cl)
    ref = X.oracle_ref(inp, "default", [])
    plain = X.oracle_ref(inp, "default", [], with_listers=False)
    assert (ref["out"] >= 0).all() and (ref["out"] != plain["out"]).sum() > 10
    # the first pod of the service: every count is 0, so the listers cannot move it
    first_svc = int(np.nonzero(~lone)[0][0])
    assert ref["out"][first_svc] == plain["out"][first_svc]
    assert any((X.oracle_ref(inp, "default", a)["out"] != X.oracle_ref(inp, "default", a, with_listers=False)["out"]).any()
               for label, a in sets_ if label.startswith("zone-"))


def test_caps_input_sits_at_both_caps():
    inp = X.caps_input()
    cl = inp.cluster()
    assert cl.n_nodes == abi.SWEEP_GENERAL_MAX_NODES
    assert len(scheduler.outage_sets(cl, X.ZONE)) == abi.SWEEP_SPREAD_MAX_ZONES
    ref = X.oracle_cpu(inp, "default", [])
    plain = X.oracle_cpu(inp, "default", [], with_listers=False)
    assert (ref["out"] >= 0).all() and (ref["out"] != plain["out"]).any()
