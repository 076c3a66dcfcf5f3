"""The per-pod kernels (ksim_schedule_one and the cache events of include/ksim.h) at block, form
and table-growth edges, against the C oracle stepped one pod per call (tests/per_pod_inputs.py;
the reference and the inputs are checked alone in tests/test_per_pod_edges_host.py).

After every call the node, lastNodeIndex, the FitError histogram and (where the case restates it)
fit_nodes must equal the reference's, afterwards the node state: every comparison is exact.

Forms (csrc/ksim_cache.cpp, ksim_schedule_one): the single-workgroup kernel (KSIM_ONE_WG=1 up to
8,192 nodes), the resident kernel running the pick body (<= 64 blocks), the scan (KSIM_NO_PICK=1, or
more than 64 blocks), the pick launch kernel (KSIM_SERVE=0, read once per process: a worker).
KSIM_PICK_NPT reaches the pick / resident / scan kernels' 2, 4 and 8 nodes-per-thread instantiations.
Whether the resident kernel served is read from the KSIM_SERVE_STATS line a handle prints when it
is destroyed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import per_pod_inputs as I

pytestmark = pytest.mark.gpu

FORMS = {
    "one_wg": {"KSIM_ONE_WG": "1"},                            # the single-workgroup kernel wherever it fits
    "default": {},                                             # <= 1,024 nodes one workgroup, else by geometry
    "resident": {"KSIM_ONE_WG": "0"},                          # the pick body in the resident kernel (<= 64 blocks)
    "scan": {"KSIM_ONE_WG": "0", "KSIM_NO_PICK": "1"},         # the multi-block scan
}
GI = 1 << 30
_REF = {}


def _ref(key, build):
    """(case, recorded script, final state) of a workload, computed once and shared."""
    if key not in _REF:
        got = build()
        case, steps = got if isinstance(got, tuple) else (got, None)
        m = I.Mirror(case.cl, case.preds, case.prios)
        steps = I.assume_all(case) if steps is None else (steps(m, case) if callable(steps) else steps)
        rec, final = I.record(m, steps, case.fit)
        _REF[key] = (case, rec, final)
    return _REF[key]


def _stats(err):
    m = re.search(r"\[ksim serve\] launches (\d+) messages (\d+) stops (\d+) left-idle (\d+) untaken-relaunches (\d+)", err)
    return None if m is None else dict(zip(("launches", "messages", "stops", "left_idle", "untaken"), map(int, m.groups())))


def _run(ref, env, monkeypatch, capfd):
    """Replay a recorded script on a fresh handle under `env`; the resident kernel's statistics
    (None: it never ran)."""
    case, rec, final = ref
    for k in ("KSIM_ONE_WG", "KSIM_NO_PICK", "KSIM_PICK_NPT", "KSIM_FUSE_A"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("KSIM_SERVE_STATS", "1")
    capfd.readouterr()
    dut = I.Dut(case.cl, case.preds, case.prios)
    try:
        I.replay(dut, rec, final)
    finally:
        dut.close()
    return _stats(capfd.readouterr().err)


def _calls(ref):
    return sum(1 for s, _ in ref[1] if s[0] in ("one", "adapter"))


def _workloads(n, chunk):
    """rotation in full up to 1,025 nodes, probes above; saturate up to 1,100 nodes."""
    out = []
    if n <= 1025:
        out.append(_ref(("rotation", n), lambda: I.rotation(n)))
    else:
        out.append(_ref(("probes", n, chunk), lambda: I.probes(n, chunk, 8 if n > 100000 else 1)))
    if n <= 1100:
        out.append(_ref(("saturate", n), lambda: I.saturate(n)))
    return out


# ----------------------------------------------------------------------------- geometry x form
@pytest.mark.parametrize("n", [1, 63, 64, 65, 512, 513, 1024, 1025, 3073, 5121, 6145, 8192])
def test_one_workgroup(n, monkeypatch, capfd):
    """Every ksim_one_kernel instantiation (2, 4, 6, 8, 10, 12, 16 nodes per thread), both sides of
    each threshold."""
    for ref in _workloads(n, 512):
        assert _run(ref, FORMS["one_wg"], monkeypatch, capfd) is None


def test_one_workgroup_ends_at_8192(monkeypatch, capfd):
    ref = _workloads(8193, 256)[0]
    st = _run(ref, FORMS["one_wg"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 600, 1025, 16383, 16384])
def test_resident(n, monkeypatch, capfd):
    """1 to 64 blocks (16,384 nodes: the last pick geometry), every message served resident."""
    for ref in _workloads(n, 256):
        st = _run(ref, FORMS["resident"], monkeypatch, capfd)
        assert st is not None and st["messages"] == _calls(ref), st


@pytest.mark.parametrize("n,form", [(257, "scan"), (600, "scan"), (16385, "resident"), (262145, "resident")])
def test_scan(n, form, monkeypatch, capfd):
    """The scan by request (KSIM_NO_PICK=1) and by geometry alone (65 blocks; 262,145 nodes: the
    first table with 2 nodes per thread)."""
    for ref in _workloads(n, 512 if n > 262144 else 256):
        assert _run(ref, FORMS[form], monkeypatch, capfd) is None


@pytest.mark.parametrize("form", ["resident", "scan"])
@pytest.mark.parametrize("n", [600, 1030, 2049])
@pytest.mark.parametrize("npt", [2, 4, 8])
def test_nodes_per_thread(npt, n, form, monkeypatch, capfd):
    """KSIM_PICK_NPT: 1 to 5 fat blocks whose last one is partial; the probes aim at both sides of
    every block and every 256-node segment boundary (the owner block's segment walk)."""
    refs = [_ref(("probes", n, 256 * npt), lambda: I.probes(n, 256 * npt))]
    if n <= 1100:
        refs.append(_ref(("saturate", n), lambda: I.saturate(n)))
    for ref in refs:
        st = _run(ref, dict(FORMS[form], KSIM_PICK_NPT=str(npt)), monkeypatch, capfd)
        if form == "resident":
            assert st is not None and st["messages"] == _calls(ref), st
        else:
            assert st is None


# ----------------------------------------------------------------------------- records and tags
def test_record_width_and_tag_wrap(monkeypatch, capfd):
    """One resident handle, 3 blocks: the decision record's width (1 + 2K words) changes call by call
    over two cycles of the 8-bit tags, then 16-class pods exactly one tag cycle apart with one-class
    pods between them."""
    ref = _ref("selector", lambda: (I.selector(600), [("one", k, True) for k in I.selector_order()]))
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref) >= 520 + 3 * 254, st


def test_pass_a_after_pass_a_free_calls(monkeypatch, capfd):
    """A second handle: 300 pods without pass A, then SelectorSpread pods over 60 zones (the pass-A
    record's words were never needed before, more than one tag cycle long)."""
    ref = _ref("spread-after-plain", lambda: I.spread(600, 60, extra_pods=I.plain_pods(300)))
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref) == 500, st


def _revisit_steps(mirror, case):
    """257 nodes (2 blocks) -> 255 (1 block) for 253 calls -> 257: the second block's record slot
    is read again exactly one tag cycle after its last use.  (A saturate-style cluster: a block's
    record changes with every commit, so a stale one differs from the current one.)"""
    k = 0
    row = I.node_row(32000, 128 * GI, 8)
    for cycle in range(3):
        for _ in range(10 if cycle == 0 else 1):
            yield ("one", k, True)
            k += 1
        yield ("node_remove", mirror.n - 1)
        yield ("node_remove", 0)
        for _ in range(253):
            yield ("one", k, True)
            k += 1
        yield ("node_add", 0, row)
        yield ("node_add", mirror.n, row)
    for _ in range(10):
        yield ("one", k, True)
        k += 1


def test_block_slot_revisited_after_one_tag_cycle(monkeypatch, capfd):
    ref = _ref("revisit", lambda: (I.saturate(257, n_pods=800, allowed=8), _revisit_steps))
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref), st


def _cycle_steps(first, others, env=None):
    """`first`, 253 calls of `others`, `first` again — three times: what only `first` writes or
    reads in the records is met again exactly one cycle of the 8-bit tags (1..254) later, by the
    first call that needs it again.  env: (for `first`, for `others`), with runs of 10 `first`."""
    first, others = iter(first), iter(others)
    steps = [("one", next(first), True) for _ in range(10 if env else 1)]
    for _ in range(3):
        steps += [("env",) + env[1]] if env else []
        steps += [("one", next(others), True) for _ in range(253)]
        steps += [("env",) + env[0]] if env else []
        steps += [("one", next(first), True) for _ in range(10 if env else 1)]
    return steps


def test_64_block_slots_revisited_after_one_tag_cycle(monkeypatch, capfd):
    """16,384 nodes: 64 blocks, then 8 blocks of 8 nodes per thread (KSIM_PICK_NPT, read per call)
    until the tag of the last 64-block call comes round, then 64 blocks again: 56 record slots are
    read one tag cycle after their last use (the record clear on a geometry change), on a
    saturate-style cluster, whose blocks' records change with every commit."""
    env = (("KSIM_PICK_NPT", None), ("KSIM_PICK_NPT", "8"))
    ref = _ref("revisit64", lambda: (I.saturate(16384, n_pods=1200), _cycle_steps(range(0, 400), range(400, 1200), env)))
    assert _calls(ref) == 10 + 3 * (253 + 10)
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref) and st["launches"] >= 7, st


def test_late_block_slots_revisited_after_one_tag_cycle(monkeypatch, capfd):
    """2,048 nodes: 8 blocks, one block of 8 nodes per thread for 253 calls, 8 blocks again.  The
    blocks above the first are late by their data (per_pod_inputs.ports_late: their threads compare
    768 port pairs, the first block's none), so the first block reads their record slots — last
    written one tag cycle ago, with this call's tag — before they are written: without the record
    clear on a geometry change it takes the old fit counts for the new ones.  This is no stall test:
    no block is held, no spin bound is touched; the later blocks do microseconds of ordinary
    predicate work more, which the record exchange is built to wait for, and with the clear in
    place the first block simply polls until their records arrive."""
    env = (("KSIM_PICK_NPT", None), ("KSIM_PICK_NPT", "8"))
    ref = _ref("late", lambda: (I.ports_late(), _cycle_steps(range(0, 100), range(100, 900), env)))
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref) == 10 + 3 * (253 + 10), st


def test_pass_a_record_revisited_after_one_tag_cycle(monkeypatch, capfd):
    """64 blocks: a SelectorSpread pod (pass A: the zone sums in the second record), 253 pods
    without pass A, a SelectorSpread pod again — the pass-A record's words are read exactly one
    tag cycle after the last call that needed them."""
    def build():
        case = I.spread(16384, 60, n_pods=40, extra_pods=I.plain_pods(800))
        aff = [int(k) for k in (case.cl.pods["aff_class"] > 0).nonzero()[0]]
        assert len(aff) >= 4 and min(aff) >= 800
        return case, _cycle_steps(aff, range(800))
    ref = _ref("pass-a-revisit", build)
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref) == 1 + 3 * 254, st


@pytest.mark.parametrize("form", ["one_wg", "resident", "scan"])
def test_sixteen_reduce_classes(form, monkeypatch, capfd):
    """Exactly 16 reduce classes (the record's word 64 is the last reason) on 3 blocks, with
    FitErrors whose reasons cross that layout."""
    ref = _ref("sixteen", lambda: I.sixteen(600))
    assert sum(e[0] < 0 for _, e in ref[1]) >= 5
    st = _run(ref, FORMS[form], monkeypatch, capfd)
    assert (st is not None) == (form == "resident")
    assert st is None or st["messages"] == _calls(ref)


@pytest.mark.parametrize("Z,fuse", [(60, None), (61, None), (61, "0")])
def test_spread_zones(Z, fuse, monkeypatch, capfd):
    """60 zones are the last count the pick record holds (served resident); 61 fall to the scan
    with its own pass A, fused behind the grid barrier or (KSIM_FUSE_A=0) as a launch of its own."""
    ref = _ref(("spread", Z), lambda: I.spread(600, Z))
    env = dict(FORMS["resident"], **({"KSIM_FUSE_A": fuse} if fuse else {}))
    st = _run(ref, env, monkeypatch, capfd)
    assert (st is not None) == (Z == 60)
    assert st is None or st["messages"] == _calls(ref)


# ----------------------------------------------------------------------------- growth on a live handle
def _growth_steps(events):
    """20 saturate-style calls, then per node event: the event, a pod placed before it removed, 20
    more calls.  Every other call is the adapter's SCHEDULE_ONLY + ksim_pod_add, one per burst with
    a counter read in between; in the middle of every burst a pod is added onto a node of another
    block than the last commit."""
    def steps(mirror, case):
        k = [0]
        spare = len(case.cl.pods) - 1

        def other_block():
            """An empty node of the last commit's shape (so it ties at the top) in another block."""
            c, s = mirror.cl.cols, mirror.state
            last = mirror.placed[max(q for q in mirror.placed if q < k[0])]
            same = (c["alloc_cpu"] == c["alloc_cpu"][last]) & (c["alloc_mem"] == c["alloc_mem"][last]) & (s["pod_count"] == 0)
            same &= np.arange(mirror.n) // 256 != last // 256
            return int(same.nonzero()[0][0]) if same.any() else (last + mirror.n // 2) % mirror.n

        def burst():
            nonlocal spare
            for j in range(20):
                if j == 9:  # while the resident kernel is live: an ASSUME message onto another block's node
                    yield ("pod_add", other_block(), spare)
                    spare -= 1
                yield ("adapter", k[0], j == 5) if j % 2 else ("one", k[0], True)
                k[0] += 1
        yield from burst()
        for ev in events:
            yield (ev[0],) + tuple(mirror.n + x if isinstance(x, int) and x < 0 else (mirror.n if x == "end" else x)
                                   for x in ev[1:])
            victim = min(mirror.placed)
            yield ("pod_remove", mirror.placed[victim], victim)
            yield from burst()
    return steps


ROW = I.node_row(32000, 128 * GI, 2)
GROW3 = [("node_add", 0, ROW), ("node_add", "end", ROW), ("node_add", 500, ROW),
         ("node_remove", 0), ("node_remove", -1), ("node_remove", 500)]


@pytest.mark.parametrize("name,n,form,npt,events", [
    ("255-257-255", 255, "resident", None, [("node_add", 0, ROW), ("node_add", "end", ROW), ("node_remove", 0),
                                            ("node_remove", -1)]),
    ("1023-1026-1023", 1023, "default", None, GROW3),
    ("16383-16386-16383", 16383, "resident", None, GROW3),
    ("511-513", 511, "resident", "2", [("node_add", 0, ROW), ("node_add", "end", ROW)]),
])
def test_growth_across_boundaries(name, n, form, npt, events, monkeypatch, capfd):
    """Node add / remove at rank 0 (every row shifts), at the last rank and inside, across a block
    boundary, the one-workgroup / resident boundary and the resident / scan boundary (the resident
    kernel must stop), on one live handle."""
    ref = _ref(("growth", name), lambda: (I.saturate(n), _growth_steps(events)))
    assert {s[0] for s, _ in ref[1]} >= {"one", "adapter", "pod_add", "pod_remove", "node_add"}
    st = _run(ref, dict(FORMS[form], **({"KSIM_PICK_NPT": npt} if npt else {})), monkeypatch, capfd)
    # the form switch itself: the resident kernel takes a message for every Schedule, and for the
    # ksim_pod_add in the middle of a burst, exactly while the table has a pick geometry
    # (<= 64 blocks, and above 1,024 nodes where the one-workgroup kernel is not switched off)
    size, want, other = n, 0, 0
    for s, _ in ref[1]:
        size += (s[0] == "node_add") - (s[0] == "node_remove")
        pick = (1024 if form == "default" else 0) < size <= 16384 * int(npt or 1)
        if s[0] in ("one", "adapter") or (s[0] == "pod_add" and isinstance(s[2], int) and s[2] > len(ref[0].cl.pods) - 100):
            want, other = want + pick, other + (not pick)
    assert other >= 40 or name in ("255-257-255", "511-513")
    assert st is not None and st["messages"] == want and st["launches"] >= 2, (st, want)


# ----------------------------------------------------------------------------- form switches
def test_ports17_between_resident_pods(monkeypatch, capfd):
    """A pod with 17 host ports (one more than a message holds) goes through the pick launch
    between resident-served pods: the relaunched resident kernel's row cache must see its commit,
    and its ports refuse the second such pod on that node."""
    ref = _ref("ports17", lambda: I.ports17())
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == _calls(ref) - 2 and st["launches"] >= 2, st


def test_idle_leave(monkeypatch, capfd):
    """50 calls, a pause longer than the resident kernel's idle bound, 50 more: decisions and
    lastNodeIndex continue exactly."""
    ref = _ref("idle", lambda: (I.rotation(600, 100), [("one", k, True) for k in range(50)] + [("sleep", 0.35)] +
                                [("one", k, True) for k in range(50, 100)]))
    st = _run(ref, FORMS["resident"], monkeypatch, capfd)
    assert st is not None and st["messages"] == 100, st
    if "KSIM_SERVE_IDLE_MS" not in os.environ:
        assert st["left_idle"] >= 1, st


def test_pick_launch_form():
    """The pick launch kernel on 3 blocks, in a child process started with KSIM_SERVE=0."""
    env = dict(os.environ, KSIM_SERVE="0", KSIM_ONE_WG="0", KSIM_SERVE_STATS="1")
    for k in ("KSIM_NO_PICK", "KSIM_PICK_NPT", "KSIM_FUSE_A"):
        env.pop(k, None)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "per_pod_worker.py")
    p = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" ok (") == 4 and "[ksim serve]" not in p.stderr, p.stdout + p.stderr
