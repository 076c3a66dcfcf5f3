"""CPU-only test of the general persistent kernels' launch geometry (csrc/ksim_pgen_plan.h):
tests/c/pgen_plan_check.cpp, a stand-alone C++ program with its own main, is compiled against the header
with the system compiler and run, once more under the address and undefined-behaviour sanitizers.  It
plans every node count from 1 to 49,153 under the workgroup caps 0, 1, 2, 27, 40, 64, 65 and 256, with
the dual form allowed and not, against LDS byte models on either side of the budget, and holds every
accepted plan to the conditions ksim_launch_pgen / ksim_launch_pgen2 check before they launch and every
refusal to a table that no form holds.  (Before the header existed the plan took the dual form for 769
rows under a cap of one workgroup, which its launcher refuses.)  Nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "c", "pgen_plan_check.cpp")


@pytest.mark.parametrize("sanitize", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_plan_geometry_against_the_launchers_conditions(tmp_path, sanitize):
    exe = tmp_path / "pgen_plan_check"
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *sanitize, "-I" + CSRC, PROGRAM,
                    "-o", str(exe)], check=True)
    # (the program allocates nothing: the leak pass, which needs ptrace, is left out)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_plan_header_needs_no_device_header():
    src = open(os.path.join(CSRC, "ksim_pgen_plan.h")).read()
    assert not re.search(r'#include\s*[<"](hip/|ksim_)', src)


def test_last_plan_is_bound_beside_an_unchanged_function_list():
    """ksim_last_plan lives in include/ksim_plan.h: ksim.h's function list and abi.EXPORTS keep their length."""
    from ksim import abi
    assert "ksim_last_plan" not in abi.EXPORTS and "ksim_last_plan" not in open(os.path.join(ROOT, "include", "ksim.h")).read()
    hdr = open(os.path.join(ROOT, "include", "ksim_plan.h")).read()
    fields = re.search(r"typedef struct ksim_plan_info \{(.*?)\} ksim_plan_info;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n for decl in re.findall(r"int(?:32|64)_t ([^;]+);", fields) for n in re.split(r",\s*", decl)]
    assert names == [k for k, _ in abi.PlanInfo._fields_]
    for k, v in (("NONE", 0), ("C2", 1), ("PGEN_SINGLE", 2), ("PGEN_DUAL", 3)):
        assert re.search(r"#define KSIM_PLAN_%s %d\b" % (k, v), hdr) and getattr(abi, "PLAN_" + k) == v
