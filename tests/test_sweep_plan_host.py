"""CPU-only tests of the sweep's scratch planning (csrc/ksim_sweep_plan.h): tests/c/sweep_plan_check.cpp,
a stand-alone C++ program with its own main, is compiled against the header with the system compiler
and run.  It carves layouts shaped like the tree, scan and general forms — measured size against the
carving pass's end, alignment, bounds, overlap, and the empty cases (no scalar columns, no port slots,
count == 0, no prefix pods, no records, no node sets) — and checks the chunk rule.  Beside it: what the
sweep's host code must no longer hold."""
import os
import re
import subprocess

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
