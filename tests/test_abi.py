"""The C-ABI library loads on a CPU-only host and exports exactly what
include/causeweave.h declares (no compute calls here)."""
import ctypes
import subprocess

import pytest

from cause_amd import abi


def test_header_declares_the_entry_points():
    names = abi.header_functions()
    for must in ("cw_abi_version", "cw_ctx_create", "cw_ctx_destroy", "cw_last_error",
                 "cw_ctx_set_stream", "cw_ctx_set_async", "cw_ctx_set_profiling",
                 "cw_ctx_set_option",
                 "cw_get_kernel_stats", "cw_reset_kernel_stats", "cw_weave_lists"):
        assert must in names


def test_library_exports_every_header_symbol():
    L = abi.lib()
    for name in abi.header_functions():
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(abi.header_functions()) <= exported


def test_abi_version():
    assert abi.lib().cw_abi_version() == 1


# the environment variables that chose the library's paths until cw_ctx_set_option
FORMER_VARIABLES = [
    "CW_FRONT", "CW_FRONT_FUSED", "CW_FRONT_SLOT", "CW_FRONT_MIN_AVG", "CW_FUSED", "CW_TOUR",
    "CW_TOUR_LOG2K", "CW_TREE_L", "CW_TREE_PROF", "CW_PACK_SORT", "CW_GDIR", "CW_GJOIN",
    "CW_GLOCAL_MIN", "CW_GIANT_MIN", "CW_GIANT_DOCS", "CW_GIANT_LOG2K", "CW_GIANT_LOG2CAP",
    "CW_MAP_SMALL", "CW_MAP_FUSED", "CW_XFOLD", "CW_X_ROUND_CAP"]


def test_library_reads_no_environment_variable():
    """Options come through cw_ctx_set_option: none of the 21 former variable
    names is in the built library, and its sources never call getenv."""
    import glob
    import os

    assert len(set(FORMER_VARIABLES)) == 21
    blob = open(abi.LIB_PATH, "rb").read()
    assert [v for v in FORMER_VARIABLES if v.encode() in blob] == []
    csrc = os.path.join(os.path.dirname(abi.LIB_PATH), "csrc")
    sources = glob.glob(os.path.join(csrc, "*"))
    assert len(sources) >= 8
    assert [p for p in sources if "getenv" in open(p, errors="replace").read()] == []


def test_struct_layout_matches_header():
    # 4 pointers-or-u64 + 4 u32 fields, naturally aligned on x86-64
    assert ctypes.sizeof(abi.CwListBatch) == 8 * 5 + 4 * 4
    assert ctypes.sizeof(abi.CwListResult) == 8 * 6
    assert ctypes.sizeof(abi.CwKernelStat) == 48 + 8 * 3
    assert ctypes.sizeof(abi.CwListBatchK128) == 8 * 5


def test_status_bits_match_header():
    import re

    src = open(abi.HEADER).read()
    bits = {m.group(1): 1 << int(m.group(2))
            for m in re.finditer(r"CW_STATUS_(\w+)\s*=\s*1u\s*<<\s*(\d+)", src)}
    for name, v in bits.items():
        assert getattr(abi, "STATUS_" + name) == v, name
    assert "KEY_RANGE" in bits


def test_no_gpu_means_a_loud_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(abi.WeaveError):
        abi.Weaver(0)
