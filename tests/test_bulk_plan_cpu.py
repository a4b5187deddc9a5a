"""No GPU: the plan of a grouped bulk update (csrc/bulk_plan.hpp), checked by a stand-alone C++ program (tests/bulk_plan_check.cpp, its own main) that is built
with the host compiler under -fsanitize=address,undefined and run once over a grid of sides 256 … 61 440, thresholds 256 … 16 384, with and without carried rows,
remainder strips included.  Nothing is loaded into python.  The program prints one "FAIL <check> <case>: <what>" line per violation; each test below owns a check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = tmp_path_factory.mktemp("bulk_plan") / "bulk_plan_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
           os.path.join(ROOT, "tests", "bulk_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    lines = run.stdout.splitlines()
    assert lines and lines[-1].startswith("cases "), run.stdout[-2000:] + run.stderr[-4000:]  # a sanitizer report ends the program before its last line
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    return dict(rc=run.returncode, lines=lines)


def _fails(report, check):
    return [ln for ln in report["lines"] if ln.startswith(f"FAIL {check} ")]


def test_the_grid_ran(report):
    n, fails = int(report["lines"][-1].split()[1]), int(report["lines"][-1].split()[3])
    assert n >= 250
    assert (report["rc"] == 0) == (fails == 0)


@pytest.mark.parametrize("check", ["disjoint", "order", "coverage", "workspace", "tiles", "sequence"])
def test_plan_property_holds_on_every_case(report, check):
    """disjoint: targets within a launch;  order: products per quadrant;  coverage: every lower / carried cell over exactly K (Strassen identities expanded on
    2×2 blocks from the entries' offsets);  workspace: slices disjoint and inside the size;  tiles: prefix sums and grid sizes;  sequence: ungrouped launch count and flops"""
    assert _fails(report, check) == []


def test_ungrouped_launch_counts_are_the_pinned_ones(report):
    """K = 256, threshold 256, 128 carried rows: 17 launches at m = 1 024 and 22 at m = 1 280 (tests/test_gpu_strassen.py pins the same on the device)"""
    counts = {ln.split()[1]: ln.split()[3] for ln in report["lines"] if ln.startswith("COUNT ")}
    assert counts == {"1024": "17", "1280": "22"}
