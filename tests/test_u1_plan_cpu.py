"""No GPU: the plan of U1 — the update of the next panel's columns — in the Strassen form (csrc/bulk_plan.hpp u1_plan_build / u1_block_rows), checked by a
stand-alone C++ program (tests/u1_plan_check.cpp, its own main) that is built with the host compiler under -fsanitize=address,undefined and run once over a grid:
panel widths 256 … 4 096, K 256 … 4 096, rectangles of 256 … 61 440 rows (heights that are no multiple of 256 included), with and without carried rows.
Nothing is loaded into python.  The program prints one "FAIL <check> <case>: <what>" line per violation; each test below owns a check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = tmp_path_factory.mktemp("u1_plan") / "u1_plan_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
           os.path.join(ROOT, "tests", "u1_plan_check.cpp")]
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
    """4 widths × 3 depths × 19 heights × {0, 128} carried rows at floor 256 are all planned; the cases at floor 8 192 are planned from 8 192 rows on"""
    w = report["lines"][-1].split()
    n, planned, fails = int(w[1]), int(w[3]), int(w[5])
    assert n >= 4 * 3 * 19 * 2 and planned >= 4 * 3 * 19 * 2
    assert planned < n  # the gate refused some: below the floor, floor 0, K or the width off the shape, no whole quadrant row
    assert (report["rc"] == 0) == (fails == 0)


@pytest.mark.parametrize("check", ["disjoint", "order", "coverage", "workspace", "tiles", "shape"])
def test_u1_plan_property_holds_on_every_case(report, check):
    """disjoint: targets within a launch;  order: products per quadrant;  coverage: every cell of the trapezoid and of the carried rows over exactly K (Strassen
    identities expanded on 2×2 blocks from the entries' offsets);  workspace: the slice inside the size, every panel read is written;  tiles: prefix sums and grid
    sizes;  shape: one block of the rectangle's whole quadrants, the square / strip / carried rows classical, and the gate"""
    assert _fails(report, check) == []
