"""The host half of cw_version / cw_delta on the CPU (cause_amd/csrc/sync_plan.h).

tests/sync_plan.cpp, a stand-alone program, runs every check of a
cw_sync_batch (each refusal of include/causeweave_sync.h that needs no device,
with nothing written), the NULL pairing of the gathered columns and the route
at every size where it changes.  It is built with the address and
undefined-behaviour sanitizers: the checks read host arrays of the caller's,
and a read past n_docs + 1 offsets must not pass unseen."""
import os
import shutil
import subprocess

import pytest

from cause_amd import abi_sync  # noqa: F401  (the header under test is the one it binds)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sync_plan_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not present")
    exe = tmp_path / "sync_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cause_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sync_plan.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
