"""The look-back epoch rule on the CPU (cause_amd/csrc/lookback.h, lb_step).

The words that k_map_pack, k_map_union and k_list_union number their output
with carry a 16-bit epoch and are cleared only when it would wrap, when the
buffer moved or when a call needs more words than were cleared.  No GPU test
makes 65,535 calls, so tests/lookback_epoch.cpp drives the rule itself: first
use, a moved buffer, more words than ever cleared, and 65,600 consecutive calls
across the wrap, against the rule as the three stages wrote it before they
shared it.  Every epoch lies in 1 .. 0xFFFE, no two calls between two clears
share one, and a clear happens exactly when that rule says."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_epoch_rule(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not present")
    exe = tmp_path / "lookback_epoch"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cause_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lookback_epoch.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
