"""CPU-only test of the histogram sub-form's bookkeeping (csrc/ksim_phist.h): tests/c/phist_check.cpp,
a stand-alone C++ program with its own main, is compiled against the header with the system compiler
(under AddressSanitizer and UBSan where the compiler links them) and run.  It builds histograms from
cache columns, moves rows one commit at a time and takes (F, M, C) with two adjusted buckets, each
against a recount of the column: random build / commit sequences, a bucket emptied to the next one
and across a gap, a row turning unfit, a row entering above the top, score 63, a workgroup's 1,568
rows in one bucket.  Nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "c", "phist_check.cpp")
BASE = ["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, PROGRAM]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _compile(exe, extra):
    return subprocess.run(BASE + extra + ["-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_histogram_bookkeeping_against_a_recount(tmp_path):
    exe = tmp_path / "phist_check"
    r = _compile(exe, SANITIZE)
    if r.returncode != 0:  # a compiler without the sanitizer runtimes: the same program without them
        r = _compile(exe, [])
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_histogram_header_needs_no_device_header_on_the_host():
    """Outside hipcc the header includes nothing of HIP or of the project."""
    src = open(os.path.join(CSRC, "ksim_phist.h")).read()
    host = re.sub(r"#ifdef __HIPCC__.*?#else", "", src, flags=re.S)
    assert not re.search(r'#include\s*[<"](hip/|ksim_)', host)
