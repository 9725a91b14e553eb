"""The exact path's synthetic-list layout on the CPU (cause_amd/csrc/xplan.h,
x_plan).

Both of exact_weave_flagged's layouts -- n + 1 slots a document for phase 1,
2n + 1 for phase 2's anchor rounds -- come from one planner.  tests/xplan.cpp
holds the two grouping loops as the function wrote them before and compares
the planner with them field for field: per-document bases (their 32-bit
truncation included), groups and the total, for one document, documents that
do not take part, all or no early documents, sizes on both sides of giant_min,
of the document limit and of a multiple of 32, totals past 2^32, and 4,000
seeded random size lists."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_matches_both_layouts(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not present")
    exe = tmp_path / "xplan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cause_amd", "csrc"),
                    os.path.join(ROOT, "tests", "xplan.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
