"""cw_weft_lists_dev through the layers that need no GPU: the built library
exports it, cause_amd/abi.py declares it, include/causeweave.h declares it."""
import ctypes as C
import os
import re

from cause_amd import abi


def test_library_exports_the_device_call():
    assert os.path.exists(abi.LIB_PATH), "libcauseweave.so is not built"
    assert hasattr(C.CDLL(abi.LIB_PATH), "cw_weft_lists_dev")


def test_abi_declares_three_arguments():
    fn = abi.lib().cw_weft_lists_dev
    assert fn.argtypes == [C.c_void_p, C.POINTER(abi.CwWeftBatch), C.POINTER(abi.CwWeftResult)]
    assert fn.restype is C.c_int
    assert callable(abi.Weaver.weft_lists_device)


def test_header_declares_it():
    assert "cw_weft_lists_dev" in abi.header_functions()
    src = open(abi.HEADER).read()
    m = re.search(r"int\s+cw_weft_lists_dev\s*\(([^)]*)\)\s*;", src)
    assert m and len(m.group(1).split(",")) == 3
