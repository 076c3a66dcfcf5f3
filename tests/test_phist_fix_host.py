"""CPU-only test of the owner's fix as a function of the class's top two buckets (khist::fix in
csrc/ksim_phist.h): tests/c/phist_fix_check.cpp, a stand-alone C++ program with its own main, is
compiled against the header with the system compiler (under AddressSanitizer and UBSan where the
compiler links them) and run.  It drives the function against khist::stats on the histogram row and
against a recount of the column: every (e_old, e_new) in {-1, 0..63}^2 over histograms with 0 to 3
non-empty buckets and top counts 1 and 2, random columns of up to 1,568 rows under random commit
sequences, F0 = 1 going to no fit row, a top bucket of one row emptied across a gap, e_new below, on,
between and above the old top two, score 63.  The program counts every case of the arithmetic and
fails if one was never taken.  Nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "c", "phist_fix_check.cpp")
BASE = ["c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, PROGRAM]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _compile(exe, extra):
    return subprocess.run(BASE + extra + ["-o", str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_fix_from_the_top_two_buckets_against_stats_and_a_recount(tmp_path):
    exe = tmp_path / "phist_fix_check"
    r = _compile(exe, SANITIZE)
    if r.returncode != 0:  # a compiler without the sanitizer runtimes: the same program without them
        r = _compile(exe, [])
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
