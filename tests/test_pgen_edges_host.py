"""CPU-only: the designed inputs of tests/test_gpu_pgen_edges.py (tests/pgen_edge_inputs.py) have the
properties their GPU cases rely on, and their reference is sound: the table-level C oracle in pieces with
carried state equals the whole-queue run, and equals the object oracle (oracle/ksim_ref.py) where the
sizes allow.  cpu_ref itself is pinned to the object oracle in tests/test_oracle_c_features.py."""
import numpy as np
import pytest

import ksim_ref as R
import pgen_edge_inputs as I
from ksim import abi

LEADS = (7, 255)  # call index of the first designed pod: any, and the one whose tag is the cleared word's


def test_pieces_equal_the_whole_queue():
    c = I.ring()
    whole, parts = c.reference(), c.reference(I.PIECES)
    assert np.array_equal(whole["out"], parts["out"]) and whole["ctr"] == parts["ctr"]
    for k in ("req_cpu", "req_mem", "pod_count", "port_count"):
        assert np.array_equal(whole["state"][k], parts["state"][k]), k
    for k in ("cnt", "carried", "vcount"):
        assert np.array_equal(whole["extra"][k], parts["extra"][k]), k
    assert (whole["out"] >= 0).all() and c.m > sum(x for x in I.PIECES if x)


@pytest.mark.parametrize("n", [1, 191, 192, 193, 384, 385, 768, 255, 256, 257, 512, 513, 769, 1024, 1025])
def test_geometry_queues_saturate(n):
    """Every size of the plan-geometry cases: the queue fills the table, so the last row is chosen (or a
    row within the last four: a few nodes are not ready), rows of every 64-row wave are, and pods fail."""
    c = I.geometry(n, light=True)
    r = c.reference()
    out = r["out"]
    assert (out < 0).sum() >= 12 and out.max() >= n - 4
    assert len(np.unique(out[out >= 0] // 64)) == (n + 63) // 64
    assert c.plan.affinity is not None and c.plan.volumes is not None
    if n >= 191:  # the features the kernels branch on are all in the queue
        p = c.plan.pods
        assert (p["vol_class"] > 0).any() and (p["aff_class"] > 0).any() and c.cl.port_slots == 0
        assert c.plan.volumes["slots"].shape[0] == 3 and r["extra"]["vcount"].max() <= 2
        assert set(I.pod_classes(c)) == {2}  # (PreferNoSchedule taints: two TaintToleration classes)
        failed = r["reasons"][out < 0]
        assert failed[:, abi.R_PODS].any()


def _object_oracle(case, max_vols=None):
    """The object oracle (oracle/ksim_ref.py) over the case's objects against the case's reference."""
    from ksim import scheduler
    o = case.marks["objs"]
    preds, prios = scheduler.provider("DefaultProvider")
    custom = {k: v for k, v in R.volume_predicates(R.VolumeListers(o.get("pvs", ()), o.get("pvcs", ())), max_vols).items()
              if k in preds}
    spread = R.SpreadListers(services=o["services"]) if "services" in o else None
    want, lni = R.simulate(o["nodes"], o.get("running", []), list(reversed(o["pods"])), set(preds), list(prios), custom,
                           spread=spread)
    ref = case.reference()
    got = [case.cl.names[w] if w >= 0 else None for w in ref["out"]]
    assert [h for _, h, _ in want] == got and lni == ref["ctr"]


def test_designed_inputs_against_the_object_oracle():
    """Where the sizes allow: the C2x-shaped geometry queue, the no-hypothesis queue and the shared-commit
    tag-cycle queue at smaller tables, and the volume queue whole."""
    _object_oracle(I.geometry(60))
    _object_oracle(I.geometry(60, light=True))
    _object_oracle(I.nohyp(n=75, m=150))
    _object_oracle(I.volumes9(n=14, m=330), max_vols=11)
    _object_oracle(I.tag_commit(7, n=240))
    _object_oracle(I.tag_ipa(7, n=400))


def test_nohyp_queue_has_every_kind():
    c = I.nohyp()
    kinds, p, out = c.marks["kinds"], c.plan.pods, c.reference()["out"]
    assert {"gpu", "eph", "ext", "zone", "host", "plain"} == set(kinds)
    assert kinds[0] == "gpu" and kinds[-1] == "gpu"
    for k, kind in enumerate(kinds):
        assert (p["add_gpu"][k] > 0) == (kind == "gpu") and (p["add_eph"][k] > 0) == (kind == "eph")
        assert (p["scalar_cnt"][k] > 0) == (kind == "ext")
        assert p["aff_class"][k] > 0 or kind not in ("zone", "host", "plain")  # (plain: a service selects it)
    a = c.plan.affinity
    assert int(a["n_dom"][a["zone_key"]]) == 25
    # consecutive shared-domain commits owned by different workgroups (of 192 rows), and refusals too
    z = [k for k, kind in enumerate(kinds) if kind == "zone"]
    runs = [(k, k + 1) for k in z if k + 1 in z and out[k] >= 0 and out[k + 1] >= 0]
    assert sum(out[a_] // 192 != out[b_] // 192 for a_, b_ in runs) >= 10
    assert (out[z] < 0).any() and (out[z] >= 0).sum() >= 60
    # a preferred zone-keyed term is read (the InterPodAffinity priority, pass A)
    assert any(kinds[k] == "zone" and (k // 12) % 2 == 1 for k in range(c.m))


@pytest.mark.parametrize("Z", [28, 29])
def test_zone_cap_inputs(Z):
    c = I.zones(Z)
    a = c.plan.affinity
    assert int(a["n_dom"][a["zone_key"]]) == Z and (c.reference()["out"] >= 0).all()


def test_volume_input_reaches_the_ninth_slot():
    c = I.volumes9()
    r = c.reference()
    out, reasons = r["out"], r["reasons"]
    assert r["extra"]["vcount"].max() >= 12 and c.plan.volumes["slots"].shape[0] > 8
    failed = reasons[out < 0]
    assert failed[:, abi.R_MAX_VOLUME_COUNT].any() and failed[:, abi.R_DISK_CONFLICT].any()
    # a find across the boundary: a pod is refused for a disk its node holds in slot 8 or later
    slots, cnt = r["extra"]["vslots"], r["extra"]["vcount"]
    assert (cnt[:10] > 8).sum() >= 5 and (slots[8:, :10] != 0).any()
    # an add across it: pods placed on a node that held eight mounts or more
    per_node = np.bincount(out[out >= 0], minlength=c.n)
    assert per_node[:10].max() >= 9 and per_node[10:].sum() == 0


@pytest.mark.parametrize("lead", LEADS)
def test_tag_cycle_pass_a_values_differ(lead):
    """InterPodAffinity: the two pods read different, non-zero maxima, held by different late workgroups, and
    the first pod's maximum in place of the second's moves the second pod (to E, a row of the first
    workgroup: the reader that would hold the stale record)."""
    c = I.tag_ipa(lead)
    m, out = c.marks, c.reference()["out"]
    stale = I.tag_ipa(lead, stale=True).reference()["out"]
    assert stale[m["second"]] == m["E"] != out[m["second"]] and m["E"] < I.LATE_FROM
    assert np.array_equal(stale[:m["second"]], out[:m["second"]])
    assert m["second"] - m["first"] == 256 and m["first"] == lead
    assert out[m["first"]] == m["A"] and out[m["second"]] == m["B"]
    assert m["A"] // 192 != m["B"] // 192 and min(m["A"], m["B"]) >= I.LATE_FROM
    p = c.plan.pods
    passa = (p["aff_class"] > 0) | (p["aff_ident"] > 0)
    assert list(np.flatnonzero(passa)) == [m["first"], m["second"]]  # nobody else writes the pass-A record
    assert (p["vol_class"] > 0).sum() >= c.m - 2 and (p["port_cnt"] > 0).all()


@pytest.mark.parametrize("lead", LEADS)
def test_tag_cycle_zone_sums_differ(lead):
    """SelectorSpread: the two pods' services count in different zones (6 + 6 against 10 + 10), and the
    slot's other pass-A pods in between write words 0-3 only (no service selects them)."""
    c = I.tag_spread(lead)
    m, a = c.marks, c.plan.affinity
    sp = np.asarray(a["spread_pair"])
    p = c.plan.pods
    has_sp = np.array([cl > 0 and sp[cl - 1] >= 0 for cl in p["aff_class"]])
    assert list(np.flatnonzero(has_sp)) == [m["first"], m["second"]]
    between = np.arange(m["first"] + 4, m["second"], 4)
    assert (p["aff_class"][between] > 0).all() and not has_sp[between].any()
    assert int(a["n_dom"][a["zone_key"]]) == 4
    out = c.reference()["out"]
    # the second pod lands on a z0 / z1 row of the first workgroup; on the first pod's zone sums (stale=True:
    # its service counted in z0 / z1) it would land on a z2 / z3 row
    stale = I.tag_spread(lead, stale=True).reference()["out"]
    k = m["second"]
    assert out[k] < I.LATE_FROM and out[k] % 4 in (0, 1) and stale[k] < I.LATE_FROM and stale[k] % 4 in (2, 3)
    # the services' running pods per zone (zone = rank % 4), all on late rows: 6 + 6 against 10 + 10
    zones = {"sa": [0] * 4, "sb": [0] * 4}
    for x in c.marks["objs"]["running"]:
        app = x["metadata"]["labels"].get("app")
        if app in zones:
            rank = int(x["spec"]["nodeName"].split("-")[1])
            assert rank >= I.LATE_FROM
            zones[app][rank % 4] += 1
    assert zones == {"sa": [6, 6, 0, 0], "sb": [0, 0, 10, 10]}
    late = I.tag_spread(lead, load=False)  # the layout whose designed pods land on late rows
    lo = late.reference()["out"]
    assert lo[m["first"]] >= I.LATE_FROM or lo[m["second"]] >= I.LATE_FROM
    assert list(np.flatnonzero(has_sp)) == [m["first"], m["second"]]


@pytest.mark.parametrize("lead", LEADS)
def test_tag_cycle_class_words(lead):
    c = I.tag_classes(lead)
    m, K, out = c.marks, I.pod_classes(c), c.reference()["out"]
    assert K[m["first"]] == 4 and K[m["second"]] == 4
    assert (np.delete(K, [m["first"], m["second"]]) == 1).all()
    # the four-class pods land on untainted rows of late workgroups: the winning class's maximum is theirs
    for k in (m["first"], m["second"]):
        assert out[k] >= I.LATE_FROM and out[k] % 4 == 0
    assert out[m["first"]] != out[m["second"]]


@pytest.mark.parametrize("lead", LEADS)
def test_tag_cycle_shared_commits(lead):
    c = I.tag_commit(lead)
    m, out = c.marks, c.reference()["out"]
    a, b = int(out[m["first"]]), int(out[m["second"]])
    assert b >= I.LATE_FROM   # a late owner: the first workgroup looks at the commit word before it is written
    assert a % 4 == 2 and b % 4 == 3                                        # different zones
    assert (out[m["probes"]] >= 0).all()
    # the probes of the second label avoid its zone and the first label's probes the first's
    for k, g in zip(m["probes"], "xyxy"):
        assert out[k] % 4 != (a if g == "x" else b) % 4
    # the grp=y probes land on z2 rows of the first workgroup, and counting grp=y at the first commit's node
    # (what a stale commit word says) moves them
    ys = [k for k, g in zip(m["probes"], "xyxy") if g == "y"]
    stale = I.tag_commit(lead, stale=True).reference()["out"]
    assert stale[m["second"]] == a
    assert a < I.LATE_FROM and out[ys[0]] < I.LATE_FROM and out[ys[0]] % 4 == 2 and stale[ys[0]] % 4 != 2
    for k in ys:
        assert stale[k] != out[k]
    # only these six pods commit to a shared domain
    p = c.plan.pods
    assert list(np.flatnonzero(p["aff_class"] > 0)) == [m["first"], m["second"]] + list(m["probes"])


def test_c2_inputs():
    for n in (449, 897, 1059, 1060):
        c = I.c2_uniform(n)
        out = c.reference()["out"]
        assert (out < 0).sum() >= 40 and out.max() == n - 2 and set(I.pod_classes(c)) == {2}
    c = I.c2_sixteen()
    assert set(I.pod_classes(c)) == {16}
    for lead in LEADS:
        c = I.c2_tag_classes(lead)
        K = I.pod_classes(c)
        assert K[lead] == 16 and K[lead + 256] == 16 and (np.delete(K, [lead, lead + 256]) == 1).all()
        assert (c.plan.pods["flags"] & abi.POD_NEED_SELECTOR).all()


@pytest.mark.parametrize("D,Z", [(57, 0), (58, 0), (53, 4), (54, 4)])
def test_aux_domain_inputs(D, Z):
    """4 + Z + 3 + D pass-A words on either side of 64."""
    c = I.aux_domains(D, Z)
    a = c.plan.affinity
    assert a["aux_pair"] is not None and int(a["n_dom"][a["aux_key"]]) == D and (c.reference()["out"] >= 0).all()
    assert (int(a["n_dom"][a["zone_key"]]) if Z else 0) == Z
    assert (4 + Z + 3 + D <= 64) == (D in (57, 53))


@pytest.mark.parametrize("refs", [346, 348])
def test_record_bound_inputs(refs):
    """592 fixed bytes + 16 per volume ref (+ at most 16 of zone verdict words): within 6,144 or beyond."""
    c = I.record_bound(refs)
    p = c.plan.pods
    assert (p["vol_class"] > 0).all() and (c.reference()["out"] >= 0).all()
    assert (592 + 16 * refs + 16 <= 6144) == (refs == 346) and 592 + 16 * 348 > 6144


def test_c2_many_classes_input():
    c = I.c2_many_classes()
    assert len(c.plan.tables["n_tt"]) == 1500 and c.n == 1059 and (c.reference()["out"] >= 0).all()
