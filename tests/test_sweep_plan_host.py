"""CPU-only tests of the sweep's scratch planning (csrc/ksim_sweep_plan.h): tests/c/sweep_plan_check.cpp,
a stand-alone C++ program with its own main, is compiled against the header with the system compiler
and run.  It carves layouts shaped like the tree, scan and general forms — measured size against the
carving pass's end, alignment, bounds, overlap, and the empty cases (no scalar columns, no port slots,
count == 0, no prefix pods, no records, no node sets) — and checks the chunk rule.  Beside it: what the
sweep's host code must no longer hold; the rule that decides which per-scenario state a general sweep
owns (csrc/ksim_sweep_admit.h, tests/c/sweep_admit_check.cpp, also under the host sanitizers); the
shape the sweep's code keeps (a kernel header, one launch description, one plan, one entry prologue);
and the Python builder of a sweep call's buffers (scheduler.SweepBuffers), without a handle."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "c", "sweep_plan_check.cpp")


def test_plan_header_under_the_system_compiler(tmp_path):
    exe = tmp_path / "sweep_plan_check"
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, PROGRAM, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_plan_header_needs_no_device_header():
    src = open(os.path.join(CSRC, "ksim_sweep_plan.h")).read()
    assert not re.search(r'#include\s*[<"](hip/|ksim_)', src)


def test_inputs_of_the_gpu_scratch_test():
    """What tests/test_gpu_sweep_scratch.py relies on: the builder's own assertions (a resource-only
    range, a range that is not), ragged node-set words, and under the C oracle the first pod on the
    last node with every pod of both ranges placed."""
    import cpu_ref
    import sweep_scratch_inputs as I
    from ksim import scheduler
    cl = I.cluster()
    assert cl.n_nodes > 1024 and cl.n_nodes % 32 and [len(a) for a in I.node_sets()] == [0, 1, 1, 2, cl.n_nodes // 10]
    assert all(len(r) == 2 for r in I.requeue()) and len(I.requeue()) == len(I.node_sets())
    preds, prios = scheduler.provider("DefaultProvider")
    p = scheduler.plan(cl, preds, prios)
    for first, count in ((0, I.FAST), (I.FAST, I.GENERAL)):
        out, _, _, _ = cpu_ref.run(cl, p.cfg, first, count, threads=2, tables=p.tables, na_add=p.na_add)
        assert (out >= 0).all() and (first or out[0] == I.N - 1)


def _code(name):
    """The file without its // comments."""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_sweep_host_code_has_one_allocation_and_one_general_launcher():
    rt = _code("ksim_sweep_rt.cpp")
    assert "need_of" not in rt and len(re.findall(r"\bhipMalloc\(", rt)) == 1
    assert "ksim_sweep" not in _code("ksim_runtime.cpp")
    launchers = re.findall(r"hipError_t (ksim_sweep_\w*launch)\(", _code("ksim_handle.h"))
    assert launchers == ["ksim_sweep_launch", "ksim_sweep_general_launch"]
    assert "ksim_sweep_rt.cpp" in open(os.path.join(CSRC, "Makefile")).read()


# ---- which state a general sweep owns: csrc/ksim_sweep_admit.h
ADMIT_PROGRAM = os.path.join(ROOT, "tests", "c", "sweep_admit_check.cpp")


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_admit_rules_under_the_system_compiler(tmp_path, sanitize):
    """The whole truth table of ksim_sweep_admit_tables; the second build runs the same stand-alone program
    under the address and undefined-behaviour sanitizers (its own main: nothing is loaded into Python)."""
    exe = tmp_path / "sweep_admit_check"
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *sanitize, "-I" + CSRC, ADMIT_PROGRAM,
                    "-o", str(exe)], check=True)
    # (the program allocates nothing: the leak pass, which needs ptrace, is left out)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_admit_header_needs_no_device_header_and_keeps_no_message():
    src = open(os.path.join(CSRC, "ksim_sweep_admit.h")).read()
    assert not re.search(r'#include\s*[<"](hip/|ksim_)', src)
    assert "ksim_fail" not in src and "printf" not in src  # the texts stay in ksim_sweep_rt.cpp


# ---- the shape of the sweep's code
def _function(code, head):
    """The text of the function whose definition starts with `head`, through its closing brace in column 0."""
    a = code.index(head)
    return code[a:code.index("\n}\n", a) + 3]


def test_sweep_units_share_a_header_and_no_source_is_included():
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp")))
    for f in names:
        assert not re.search(r'#\s*include\s*[<"][^>"]*\.hip[>"]', _code(f)), f
        assert "KSIM_SWEEP_VOL_TU" not in open(os.path.join(CSRC, f)).read(), f
    assert "KSIM_SWEEP_VOL_TU" not in open(os.path.join(CSRC, "Makefile")).read()
    for unit in ("ksim_sweep.hip", "ksim_sweep_vol.hip"):
        assert '#include "ksim_sweep_kernels.h"' in _code(unit)
        assert "__global__ __launch_bounds__(SB) void ksim_sweep_general_kernel(" not in _code(unit)
    # each unit names the instantiations it had: the VOL ones (sixth argument) in the vol unit alone
    vol6 = re.compile(r"ksim_sweep_general_kernel<\s*true,\s*true,\s*PRE,\s*\w+,\s*\w+,\s*true\s*>")
    assert vol6.findall(_code("ksim_sweep_vol.hip")) and not vol6.findall(_code("ksim_sweep.hip"))
    assert "ksim_sweep_general_kernel<" in _code("ksim_sweep.hip")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = [ln for ln in mk.splitlines() if ln.endswith(": ksim_sweep_kernels.h")]
    assert len(rule) == 1 and all(o in rule[0] for o in ("build/ksim_sweep_vol.hip.o", "build/stamps/ksim_sweep_vol.hip.o",
                                                         "build/ksim_sweep.hip.o", "build/stamps/ksim_sweep.hip.o"))


def test_kernel_arguments_are_assembled_once_from_one_launch_description():
    both = "".join(_code(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".cpp")))
    # the SwgArgsSpr / SwgArgsIpa assembly: one slice of the queue's arguments into the fuller struct
    assert len(re.findall(r"\(SwgArgsPre&\)", both)) == 1 and "(SwgArgsPre&)" in _code("ksim_sweep_kernels.h")
    assert not re.search(r"\bSwgArgs(Spr|Ipa) \w+\{", _code("ksim_sweep.hip") + _code("ksim_sweep_vol.hip"))
    assert re.search(r"ksim_sweep_general_launch\(const SwgLaunch\* \w+\);", _code("ksim_handle.h"))
    # null-ness of a feature part is decided in one place of the host code: where swg_run fills the description
    rt = _code("ksim_sweep_rt.cpp")
    run = _function(rt, "int swg_run(")
    assert "SwgLaunch " in run and re.search(r"\? &m\.\w+ : nullptr", run)
    rest = rt.replace(run, "")
    assert "SwgLaunch" not in rest and not re.search(r"\? &m\.\w+ : nullptr", rest)


def test_sweep_is_built_in_one_place_and_the_general_form_runs_in_steps():
    rt = _code("ksim_sweep_rt.cpp")
    # a Sweep is declared in sweep_of alone and filled by name: no positional aggregate anywhere
    assert "Sweep sw;" in _function(rt, "Sweep sweep_of(") and not re.search(r"\bSweep \w+;", rt.replace(_function(rt, "Sweep sweep_of("), ""))
    assert not re.search(r"\bSweep( \w+)?\{|sweep_impl\(\{", rt) and "nullptr" not in _function(rt, "Sweep sweep_of(")
    for entry in ("ksim_sweep_drain", "ksim_sweep_affinity", "ksim_sweep_volumes", "ksim_sweep_policy"):
        body = _function(rt, "int %s(" % entry)
        assert "nullptr" not in body and not re.search(r"check_failures|check_queue|check_residents|std::fill|NO_NODES", body), entry
        order = [body.index(w) for w in ("sweep_of(", "queue_checks(sw, ", "hipSetDevice(", "return queue_sweep(sw, ")]
        assert order == sorted(order), entry
    checks = _function(rt, "int queue_checks(")
    order = [checks.index(w) for w in ("check_failures(", "check_queue(", "check_residents(")]
    assert order == sorted(order) and "hip" not in checks
    shared = _function(rt, "int queue_sweep(")
    order = [shared.index(w) for w in ("KSIM_E_NO_NODES", "ksim_rt_check_aff(", "std::fill(", "sweep_general(")]
    assert order == sorted(order)
    assert rt.index("int queue_sweep(") < rt.index("int ksim_sweep_drain(")  # defined before its callers, declared nowhere else
    general = _function(rt, "int sweep_general(Sweep& sw)")
    steps = [general.index(w) for w in ("swg_admit(", "sweep_scratch(", "swg_upload(", "swg_run(", "swg_verdict(", "sweep_done(")]
    assert steps == sorted(steps)
    # the per-scenario estimate is measured from the layout, and the features are read from the plan alone
    assert "ksim_sweep_measure(layout, 0)" in general and not re.search(r"sizeof\(Ksim(Aff|Vol|Ctx)\)", general)
    for step in ("void swg_layout(", "int swg_upload(", "int swg_run(", "int swg_verdict("):
        assert not re.search(r"sw\.(ipa|vol|pol)\b", _function(rt, step)), step
    # no function longer than the tree form's driver, which this file's refactor left as it was
    longest = max((len(m.group(0).splitlines()), m.group(0).splitlines()[0])
                  for m in re.finditer(r"^(?:template[^\n]*\n)?[A-Za-z][^;{}]*\) (?:const )?\{\n.*?^\}\n", open(
                      os.path.join(CSRC, "ksim_sweep_rt.cpp")).read(), re.M | re.S))
    assert longest[1].startswith("int sweep_tree(") or longest[0] <= 86, longest


# ---- the Python side: one builder of a sweep call's buffers, without a handle
def test_sweep_buffers_shapes_fills_and_structs():
    import ctypes

    import numpy as np

    from ksim import abi, scheduler
    B = scheduler.SweepBuffers
    b = B(3, 5)
    assert (b.out.shape, b.out.dtype) == ((3, 5), np.int32) and (b.ctr.shape, b.ctr.dtype) == ((3,), np.uint64)
    assert all((a.shape, a.dtype) == ((3,), np.int32) for a in (b.sched, b.rehosted)) and isinstance(b.st, abi.Stats)
    assert [b.weights, b.absent, b.rq, b.off, b.pod, b.pre, b.f, b.fails, b.rs, b.res, b.oc, b.rec] == [None] * 12
    w = B(2, 1, weights=[[1, 0, 1, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0]]).weights
    assert (w.shape, w.dtype) == ((2, abi.NW), np.int64) and w.flags["C_CONTIGUOUS"]
    # a range of no pods; width: the columns of out where they are not count
    assert B(2, 0).out.shape == (2, 0) and B(2, 0, requeue=[[1], []]).out.shape == (2, 0)
    assert B(2, -1, requeue=[[1], []], width=0).out.shape == (2, 0) and B(2, 3, width=1).out.shape == (2, 1)

    # re-queue lists: off the cumulative lengths from 0, pod back to back, pre parallel to pod
    b = B(4, 2, requeue=[[7, 3], (), iter([5]), np.array([9, 9, 1])])
    assert b.off.dtype == np.int64 and b.off.tolist() == [0, 2, 2, 3, 6] and b.off[0] == 0
    assert b.pod.dtype == np.int64 and b.pod.tolist() == [7, 3, 5, 9, 9, 1] and b.pod.flags["C_CONTIGUOUS"]
    assert (b.pre.shape, b.pre.dtype) == ((6,), np.int32) and [p.tolist() for p in b.prefix()] == [[0, 0], [], [0], [0, 0, 0]]
    b.pre[:] = np.arange(6)
    assert [p.tolist() for p in b.prefix()] == [[0, 1], [], [2], [3, 4, 5]]  # views of pre, by off
    assert ctypes.addressof(b._rq.off.contents) == b.off.ctypes.data and ctypes.addressof(b._rq.pod.contents) == b.pod.ctypes.data
    e = B(2, 0, requeue=[[], []])  # empty prefixes
    assert e.off.tolist() == [0, 0, 0] and e.pod.shape == (0,) and e.pre.shape == (0,) and e.rq is not None
    z = B(0, 3, requeue=[])
    assert z.off.tolist() == [0] and z.pod.shape == (0,) and z.out.shape == (0, 3) and z.prefix() == []

    # explain: True = every pod of the longest queue (longest prefix + count), an int = that cap; -1 fills
    for kw, cap in ((dict(explain=True), 5), (dict(explain=2), 2), (dict(explain=0), 0), (dict(explain=True, requeue=[[1, 2, 3], [4]]), 8),
                    (dict(explain=4, requeue=[[1, 2, 3], [4]]), 4)):
        b = B(2, 5, **kw)
        assert b._f.cap == cap and sorted(b.fails) == ["count", "hist", "listed", "pod"]
        assert b.fails["pod"].shape == (2, cap) and b.fails["hist"].shape == (2, cap, abi.NREASONS)
        assert all(b.fails[k].dtype == np.int32 for k in b.fails) and (b.fails["pod"] == -1).all() and (b.fails["hist"] == -1).all()
        assert b.fails["count"].tolist() == [0, 0] and b.fails["listed"].tolist() == [0, 0] and b.f is not None
    assert B(2, 0, explain=True, requeue=[[], []])._f.cap == 0 and B(0, 3, explain=True, requeue=[])._f.cap == 3
    assert B(2, 5, explain=False).f is None and B(2, 5, explain=None).fails is None
    neg = B(1, 5, explain=-2)  # the C entry refuses the negative cap; the arrays are empty
    assert neg._f.cap == -2 and neg.fails["pod"].shape == (1, 0)

    # residents: the cluster's rows, then exactly the bound pods with an affinity identity or class
    pods = np.zeros(4, abi.POD_DTYPE)
    pods["aff_ident"] = [0, 2, 0, 0]
    pods["aff_class"] = [0, 0, 3, 0]
    b = B(1, 1, residents=[(4, 1, 1), (6, 0, 2)], bound=[(0, 10), (1, 11), (2, 12), (3, 13), (1, 14)], pods=pods)
    assert b.res.dtype == np.int32 and b.res.tolist() == [[4, 1, 1], [6, 0, 2], [11, 2, 0], [12, 0, 3], [14, 2, 0]]
    assert b.rs.n == 5 and [b.rs.node[k] for k in range(5)] == [4, 6, 11, 12, 14]
    assert [b.rs.aff_ident[k] for k in range(5)] == [1, 0, 2, 0, 2] and [b.rs.aff_class[k] for k in range(5)] == [1, 2, 0, 3, 0]
    b = B(1, 1, residents=np.zeros((0, 3), np.int32))
    assert b.res.shape == (0, 3) and b.rs.n == 0

    # outcome records
    b = B(3, 1, outcome=True)
    assert sorted(b.rec) == ["free_cpu", "free_mem", "listed", "used"] and all(a.dtype == np.int32 for a in b.rec.values())
    assert b.rec["listed"].shape == b.rec["used"].shape == (3,)
    assert b.rec["free_cpu"].shape == b.rec["free_mem"].shape == (3, abi.OUTCOME_BUCKETS) and b.oc is not None
    assert ctypes.addressof(b._oc.free_mem.contents) == b.rec["free_mem"].ctypes.data


def test_every_sweep_method_builds_its_buffers_through_the_builder():
    import inspect

    from ksim import scheduler
    G = scheduler.GenericScheduler
    for m in (G.sweep, G._sweep_sets, G.sweep_drain, G._sweep_owned):
        src = inspect.getsource(m)
        src = src[src.index('"""', src.index('"""') + 3) + 3:] if '"""' in src else src
        if m is G.sweep_drain:  # the owned sweep without residents
            assert "self._sweep_owned(" in src and "SweepBuffers(" not in src
        else:
            assert src.count("SweepBuffers(") == 1, m
        assert "np.zeros" not in src and "np.full" not in src and "abi.Sweep" not in src and "abi.Stats" not in src, m
    assert "_sweep_weights(scenarios)" in inspect.getsource(G.sweep)
