"""The general persistent kernels (ksim_pgen.hip: ksim_pgen_kernel, the single-hypothesis form, and
ksim_pgen2_kernel, the dual one; ksim_persistent.hip, C2) at plan, ring and tag-cycle edges, through the C
ABI, against the table-level C oracle on the same plan (tests/pgen_edge_inputs.py; the inputs and their
reference are checked alone in tests/test_pgen_edges_host.py).

Every case compares placements, the FitError histograms of the failed pods, lastNodeIndex, the node state
and (with volume tables) every node's mounts, exactly, and asserts ksim_last_plan: the kernel, its grid,
rows per workgroup and rows per thread, so that a case cannot silently move to another kernel.  The
canonical affinity counts have no read-back entry: every pgen case schedules its queue in at least two
calls, and the later calls stage the counts the earlier ones wrote back (a count lost or misplaced by the
write-back changes a later placement of these queues: anti-affinity and SelectorSpread read them).

The caps that select a plan are diagnostic environment variables: KSIM_MAX_GRID (read when the handle is
created), KSIM_PGEN_CHUNK, KSIM_PGEN_V1, KSIM_PGEN_NO_HDENSE, KSIM_PERSIST_GRID, KSIM_NO_STATIC_TABLE
(read per call)."""
import numpy as np
import pytest

import pgen_edge_inputs as I
from ksim import abi, scheduler

pytestmark = pytest.mark.gpu

ENV = ("KSIM_MAX_GRID", "KSIM_PGEN_CHUNK", "KSIM_PGEN_V1", "KSIM_PGEN_NO_HDENSE", "KSIM_PERSIST_GRID",
       "KSIM_NO_STATIC_TABLE", "KSIM_NO_PGEN", "KSIM_NO_PCACHE")
STATE = ("req_cpu", "req_mem", "req_gpu", "req_eph", "nz_cpu", "nz_mem", "pod_count", "port_count", "req_scalar")
DUAL, SINGLE, C2, NONE = abi.PLAN_PGEN_DUAL, abi.PLAN_PGEN_SINGLE, abi.PLAN_C2, abi.PLAN_NONE


def _mounts(slots, cnt):
    """Per node, the mounted words as a sorted tuple (slot order is not part of the state)."""
    return [tuple(sorted(int(slots[s, i]) for s in range(int(cnt[i])))) for i in range(len(cnt))]


def _run(case, env, monkeypatch, pieces=None, mode=abi.MODE_AUTO):
    """Schedule the case's queue under `env` in `pieces` (counts; None = the rest; default: all but the last
    20 pods, then those), compare everything with the reference, return every call's last_plan()."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    if pieces is None:
        pieces = (case.m - 20, None) if case.m > 40 else (case.m // 2, None)
    ref = case.reference(pieces)
    g = scheduler.GenericScheduler(case.cl, case.preds, case.prios, mode=mode, collect_reasons=True,
                                   custom_priorities=case.custom)
    try:
        outs, reas, plans, first = [], [], [], 0
        for cnt in pieces:
            cnt = case.m - first if cnt is None else cnt
            out, reasons, _ = g.schedule(first, cnt)
            outs.append(out)
            reas.append(reasons)
            plans.append(g.last_plan())
            first += cnt
        out, reasons = np.concatenate(outs), np.concatenate(reas)
        mism = np.flatnonzero(out != ref["out"])
        assert mism.size == 0, ("first mismatch at pod", int(mism[0]), int(out[mism[0]]), int(ref["out"][mism[0]]), mism.size,
                                plans[0])
        failed = out < 0
        assert np.array_equal(reasons[failed], ref["reasons"][failed])
        assert g.last_node_index == ref["ctr"]
        s = g.node_state()
        for k in STATE:
            assert np.array_equal(s[k], ref["state"][k]), k
        if g.volumes is not None:
            slots, cnt = g.volume_state()
            assert np.array_equal(cnt, ref["extra"]["vcount"])
            assert _mounts(slots, cnt) == _mounts(ref["extra"]["vslots"], ref["extra"]["vcount"])
    finally:
        g.close()
    return plans


def _is(plan, kernel, grid=None, rows=None, npt=None):
    assert plan["kernel"] == kernel, plan
    assert plan["finished"] == (0 if kernel == NONE else 1), plan
    for k, v in (("grid", grid), ("rows_per_wg", rows), ("rows_per_thread", npt)):
        assert v is None or plan[k] == v, (k, v, plan)
    if kernel in (DUAL, SINGLE):
        rt = 192 if kernel == DUAL else 256
        assert plan["rows_per_wg"] <= plan["rows_per_thread"] * rt and plan["rec_stride"] % 16 == 0
        assert 0 < plan["lds_bytes"] <= 154 * 1024 and plan["vslots"] == min(plan["vcap"], 8)


# ---------------------------------------------------------------------------------- plan geometry
@pytest.mark.parametrize("n,npt", [(1, 1), (191, 1), (192, 1), (193, 2), (384, 2), (385, 4), (768, 4)])
def test_dual_form_one_workgroup(n, npt, monkeypatch):
    """KSIM_MAX_GRID=1: every row in one workgroup, rows per thread 1 -> 2 -> 4 at 192 / 384 rows, the
    largest launch at 768; the queue saturates, so the last rows are chosen."""
    for p in _run(I.geometry(n, light=True), {"KSIM_MAX_GRID": 1}, monkeypatch):
        _is(p, DUAL, 1, n, npt)


@pytest.mark.parametrize("n,npt", [(255, 1), (256, 1), (257, 2), (512, 2), (513, 4), (1024, 4)])
def test_single_form_one_workgroup(n, npt, monkeypatch):
    for p in _run(I.geometry(n, light=True), {"KSIM_MAX_GRID": 1, "KSIM_PGEN_V1": 1}, monkeypatch):
        _is(p, SINGLE, 1, n, npt)


def test_769_rows_under_one_workgroup_take_the_single_form(monkeypatch):
    """More rows than the dual form launches in a workgroup (768) under a cap of one: the single form
    (1,024), where the plan used to hand the dual launcher a chunk it refuses (KSIM_E_DEVICE)."""
    for p in _run(I.geometry(769, light=True), {"KSIM_MAX_GRID": 1}, monkeypatch):
        _is(p, SINGLE, 1, 769, 4)


def test_1025_rows_under_one_workgroup_take_the_launch_form(monkeypatch):
    for p in _run(I.geometry(1025, light=True), {"KSIM_MAX_GRID": 1}, monkeypatch):
        _is(p, NONE)


def test_dual_form_short_last_workgroup(monkeypatch):
    """193 rows in chunks of 192: the second workgroup holds one row."""
    for p in _run(I.geometry(193), {"KSIM_PGEN_CHUNK": 192}, monkeypatch):
        _is(p, DUAL, 2, 192, 1)


def test_dual_form_64_workgroups_and_the_single_form_beyond(monkeypatch):
    """A chunk hint below ceil(n / 64) is held there: the dual form never exceeds 64 workgroups (one granule
    per lane in its sweeps); the single form takes the hint and runs its 65..256-workgroup instantiation."""
    for p in _run(I.geometry(1024), {"KSIM_PGEN_CHUNK": 1}, monkeypatch):
        _is(p, DUAL, 64, 16, 1)
    for p in _run(I.geometry(1040), {"KSIM_PGEN_CHUNK": 1}, monkeypatch):  # ceil(1040 / 64) = 17 rows: 62 workgroups
        _is(p, DUAL, 62, 17, 1)
    for p in _run(I.geometry(1040), {"KSIM_PGEN_CHUNK": 16, "KSIM_PGEN_V1": 1}, monkeypatch):
        _is(p, SINGLE, 65, 16, 1)


def test_static_words_staged_or_not(monkeypatch):
    """The static (pod class, row) words are staged when they fit beside the rows (192 rows a workgroup)
    and dropped when they do not (768 rows in one workgroup): the kernel then computes them from the tables."""
    c = I.geometry(768, light=True)
    small = _run(c, {"KSIM_PGEN_CHUNK": 192}, monkeypatch)
    for p in small:
        _is(p, DUAL, 4, 192, 1)
        assert p["n_st"] == len(c.plan.tables["n_tt"]) > 0, p
    for p in _run(c, {"KSIM_MAX_GRID": 1}, monkeypatch):
        _is(p, DUAL, 1, 768, 4)
        assert p["n_st"] == 0 and p["lds_bytes"] + 2 * 768 * small[0]["n_st"] > 154 * 1024, p


def test_dense_hypothesis_deltas_on_and_off(monkeypatch):
    """Counted pairs (SelectorSpread, anti-affinity matches) and carried terms with the dense deltas and,
    KSIM_PGEN_NO_HDENSE=1, with the per-entry lookups."""
    c = I.nohyp()
    for p in _run(c, {"KSIM_PGEN_CHUNK": 192}, monkeypatch):
        _is(p, DUAL, 3, 192, 1)
        assert p["hdense"] == 1
    for p in _run(c, {"KSIM_PGEN_CHUNK": 192, "KSIM_PGEN_NO_HDENSE": 1}, monkeypatch):
        _is(p, DUAL, 3, 192, 1)
        assert p["hdense"] == 0


@pytest.mark.parametrize("form", ["dual", "single"])
def test_volume_slots_beyond_lds(form, monkeypatch):
    """Nodes with up to 16 mounts: slots 8.. stay in HBM (a find, an add and the MaxPD count cross slot 8)."""
    env = {"KSIM_PGEN_CHUNK": 192}
    if form == "single":
        env["KSIM_PGEN_V1"] = 1
    for p in _run(I.volumes9(), env, monkeypatch, pieces=(100, 100, None)):
        _is(p, DUAL if form == "dual" else SINGLE, 2)
        assert p["vcap"] > 8 and p["vslots"] == 8


# ---------------------------------------------------------------------------------- ring and call edges
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
def test_short_calls(grid, count, monkeypatch):
    """Calls of 1..5 pods on a live handle (the two-record preload, wave 4's copy of pod p+2, the deferred
    commit of a call's last pod), twelve in a row, then the rest."""
    env = {"KSIM_MAX_GRID": 1} if grid == 1 else {"KSIM_PGEN_CHUNK": 134}
    c = I.geometry(300, light=True) if grid == 1 else I.ring()
    for p in _run(c, env, monkeypatch, pieces=(count,) * 12 + (None,)):
        _is(p, DUAL, grid)


@pytest.mark.parametrize("grid", [1, 3])
def test_one_queue_in_pieces(grid, monkeypatch):
    """schedule(first, count) with counts 1, 2, 3, 5, 250 and the rest: the state is written back and staged
    again on every piece (the host test pins that the reference in pieces equals the whole queue)."""
    env = {"KSIM_MAX_GRID": 1} if grid == 1 else {"KSIM_PGEN_CHUNK": 134}
    c = I.geometry(300, light=True) if grid == 1 else I.ring()
    for p in _run(c, env, monkeypatch, pieces=I.PIECES):
        _is(p, DUAL, grid)


# ---------------------------------------------------------------------------------- PGF_NOHYP and shared domains
@pytest.mark.parametrize("form", ["dual", "single"])
def test_commits_that_leave_the_lds_image(form, monkeypatch):
    """gpu / ephemeral-storage / extended-resource requests and zone-keyed required and preferred terms
    between node-keyed pods; consecutive shared-domain commits owned by different workgroups; such a pod
    first and last in a call (the queue's first and last pod, and the pieces cut at a zone-keyed run)."""
    env = {"KSIM_PGEN_CHUNK": 192}
    if form == "single":
        env["KSIM_PGEN_V1"] = 1
    c = I.nohyp()
    kinds = c.marks["kinds"]
    cut = next(k for k in range(100, c.m) if kinds[k] == "zone" and kinds[k + 1] == "zone")
    assert kinds[cut] == kinds[cut + 1] == "zone"
    for p in _run(c, env, monkeypatch, pieces=(cut + 1, None)):  # the first call ends, the second starts on one
        _is(p, DUAL if form == "dual" else SINGLE, 3, 192, 1)


# ---------------------------------------------------------------------------------- caps
def test_28_zones_against_29(monkeypatch):
    for p in _run(I.zones(28), {"KSIM_PGEN_CHUNK": 192}, monkeypatch):
        _is(p, DUAL, 2, 192, 1)
    for p in _run(I.zones(29), {"KSIM_PGEN_CHUNK": 192}, monkeypatch):
        _is(p, NONE)


@pytest.mark.parametrize("D,Z", [(57, 0), (53, 4)])
def test_pass_a_record_of_64_words_against_65(D, Z, monkeypatch):
    """The auxiliary priority's domains (with and without spread zones) up to the 64 words a workgroup
    publishes: 4 + Z + 3 + D = 64 runs the dual form, one domain more the launch form."""
    for p in _run(I.aux_domains(D, Z), {"KSIM_PGEN_CHUNK": 192}, monkeypatch):
        _is(p, DUAL, 2, 192, 1)
    for p in _run(I.aux_domains(D + 1, Z), {"KSIM_PGEN_CHUNK": 192}, monkeypatch):
        _is(p, NONE)


def test_record_just_under_the_bound_against_one_over(monkeypatch):
    """A pod with 346 volume refs (a record of at most 6,144 bytes) against one with 348."""
    for p in _run(I.record_bound(346), {}, monkeypatch):
        _is(p, DUAL, 1, 64, 1)
        assert 6128 <= p["rec_stride"] <= 6144, p
    for p in _run(I.record_bound(348), {}, monkeypatch):
        _is(p, NONE)


# ---------------------------------------------------------------------------------- tag cycle
TAG_ENV = {"dual": {"KSIM_PGEN_CHUNK": 192}, "single": {"KSIM_PGEN_CHUNK": 192, "KSIM_PGEN_V1": 1}}


def _tag_case(case, form, monkeypatch):
    """One call over the designed pods (the tag is the call index), then the last pods in a second call."""
    for p in _run(case, TAG_ENV[form], monkeypatch, pieces=(case.marks["second"] + 2, None)):
        _is(p, DUAL if form == "dual" else SINGLE, 3, 192, 1)


@pytest.mark.parametrize("form", ["dual", "single"])
@pytest.mark.parametrize("lead", [7, 255])
def test_pass_a_record_one_tag_cycle_later(lead, form, monkeypatch):
    """InterPodAffinity-priority pods at call index lead and lead + 256, no pass-A pod between: a record
    word left alone would carry the second pod's tag with the first one's minimum and maximum (lead = 255:
    the cleared word's zeros, a value of -2^55)."""
    _tag_case(I.tag_ipa(lead), form, monkeypatch)


@pytest.mark.parametrize("form", ["dual", "single"])
@pytest.mark.parametrize("lead", [7, 255])
def test_zone_words_one_tag_cycle_later_late_rows(lead, form, monkeypatch):
    """The same layout without the late rows' load: the designed pods land on late workgroups' rows."""
    _tag_case(I.tag_spread(lead, load=False), form, monkeypatch)


@pytest.mark.parametrize("form", ["dual", "single"])
@pytest.mark.parametrize("lead", [7, 255])
def test_zone_words_one_tag_cycle_later(lead, form, monkeypatch):
    """SelectorSpread pods 256 calls apart with InterPodAffinity-only pods of the same slot between: words
    0-3 are fresh, the zone words are the first pod's unless every call writes them."""
    _tag_case(I.tag_spread(lead), form, monkeypatch)


@pytest.mark.parametrize("form", ["dual", "single"])
@pytest.mark.parametrize("lead", [7, 255])
def test_class_words_one_tag_cycle_later(lead, form, monkeypatch):
    """A four-class decision, 255 one-class decisions, a four-class decision whose maxima sit in late
    workgroups: class words 1-3 of the slot."""
    _tag_case(I.tag_classes(lead), form, monkeypatch)


@pytest.mark.parametrize("form", ["dual", "single"])
@pytest.mark.parametrize("lead", [7, 255])
def test_commit_word_one_tag_cycle_later(lead, form, monkeypatch):
    """Shared-domain commits 256 calls apart owned by late workgroups: the first workgroup reads the commit
    word before its owner writes it, and an 8-bit tag would accept the node of the commit 256 calls back."""
    _tag_case(I.tag_commit(lead), form, monkeypatch)


# ---------------------------------------------------------------------------------- C2 (ksim_persistent.hip)
@pytest.mark.parametrize("n,grid,npt", [(448, 1, 1), (449, 1, 2), (896, 1, 2), (897, 1, 4), (1059, 1, 4)])
def test_c2_rows_per_thread(n, grid, npt, monkeypatch):
    """KSIM_PERSIST_GRID=1: 448 rows a thread slot, rows per thread 1 -> 2 -> 4; selector pods that tie on
    every fit node, two TaintToleration classes, decoys at the first, a middle and the last row.  1,059 rows
    of 116 bytes are the most a workgroup's 120 KiB row budget holds, so chunks of 1,792 / 1,793 and the
    eight-rows instantiation cannot be reached through ksim_persistent_config."""
    for p in _run(I.c2_uniform(n), {"KSIM_PERSIST_GRID": grid}, monkeypatch, mode=abi.MODE_PERSISTENT):
        _is(p, C2, grid, n, npt)


def test_c2_one_row_past_the_budget_takes_the_launch_form(monkeypatch):
    for p in _run(I.c2_uniform(1060), {"KSIM_PERSIST_GRID": 1}, monkeypatch):
        _is(p, NONE)


@pytest.mark.parametrize("n", [64 * 192, 64 * 192 + 1])
def test_c2_64_workgroups_and_wider(n, monkeypatch):
    """Up to 64 x 192 rows take 64 workgroups (one per sweep lane), one more row the wider instantiation."""
    c = I.c2_uniform(n, m=600)
    for p in _run(c, {}, monkeypatch, mode=abi.MODE_PERSISTENT):
        assert p["kernel"] == C2 and (p["grid"] == 64) == (n == 64 * 192) and p["grid"] * p["rows_per_wg"] >= n, p
        assert p["rows_per_thread"] == 1 and p["tables"] == 1


def test_c2_layout_with_and_without_ports(monkeypatch):
    """PLayout: host ports in LDS, none in the table, and too many slots for LDS (they stay in HBM)."""
    for p in _run(I.c2_ports(600, 1500), {"KSIM_PERSIST_GRID": 2}, monkeypatch, mode=abi.MODE_PERSISTENT):
        _is(p, C2, 2, 300, 1)
        assert p["ps"] == I.c2_ports(600, 1500).cl.port_slots > 0 and p["tables"] == 1
    for p in _run(I.c2_uniform(449), {"KSIM_PERSIST_GRID": 2}, monkeypatch, mode=abi.MODE_PERSISTENT):
        _is(p, C2, 2, 225, 1)
        assert p["ps"] == 0
    big = I.c2_ports(1000, 1500)  # 1,000 rows x (4 + 12 x 8) bytes of ports beside 1,000 x 116 of rows
    for p in _run(big, {"KSIM_PERSIST_GRID": 1}, monkeypatch, mode=abi.MODE_PERSISTENT):
        _is(p, C2, 1, 1000, 4)
        assert p["ps"] == 0 and big.cl.port_slots == 12


def test_c2_tables_and_static_words(monkeypatch):
    """The pod-class tables in LDS with and without the static words (KSIM_NO_STATIC_TABLE=1)."""
    c = I.c2_sixteen()
    for p in _run(c, {}, monkeypatch, mode=abi.MODE_PERSISTENT):
        assert p["kernel"] == C2 and p["tables"] == 1 and p["static_table"] == 1, p
    for p in _run(c, {"KSIM_NO_STATIC_TABLE": 1}, monkeypatch, mode=abi.MODE_PERSISTENT):
        assert p["kernel"] == C2 and p["tables"] == 1 and p["static_table"] == 0, p


def test_c2_tables_read_from_hbm(monkeypatch):
    """1,500 pod classes beside 1,059 rows: the class tables do not fit LDS and stay in HBM."""
    for p in _run(I.c2_many_classes(), {"KSIM_PERSIST_GRID": 1}, monkeypatch, mode=abi.MODE_PERSISTENT):
        _is(p, C2, 1, 1059, 4)
        assert p["tables"] == 0 and p["static_table"] == 0, p


@pytest.mark.parametrize("lead", [7, 255])
def test_c2_class_words_one_tag_cycle_later(lead, monkeypatch):
    """A sixteen-class pod, 255 one-class pods, a sixteen-class pod, in four workgroups."""
    for p in _run(I.c2_tag_classes(lead), {"KSIM_PERSIST_GRID": 4}, monkeypatch, mode=abi.MODE_PERSISTENT,
                  pieces=(lead + 258, None)):
        _is(p, C2, 4, 51, 1)
