"""ctypes binding of include/causeweave_sync.h: cw_version (the per-site heads
of every document, (peek yarn) of s/spin) and cw_delta (the nodes above a
peer's heads, the complement of what s/weft keeps).

The signatures are applied to the library abi.lib() loads.  ``version`` and
``delta`` (host arrays in, dataclasses out) and ``version_device`` /
``delta_device`` (raw device pointers) take an abi.Weaver.  There is no
fallback: a library without the symbols raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import abi

HEADER = os.path.join(os.path.dirname(abi.HEADER), "causeweave_sync.h")
_U64P = C.POINTER(C.c_uint64)
WAVE_CAP = 256  # CW_SYNC_WAVE_CAP


class CwSyncBatch(C.Structure):
    _fields_ = [("n_docs", C.c_uint64), ("doc_offsets", _U64P), ("id_key", C.c_void_p), ("cause", C.c_void_p),
                ("kind", C.c_void_p), ("cause_is_id", C.c_void_p), ("ts_shift", C.c_uint32),
                ("site_shift", C.c_uint32), ("site_bits", C.c_uint32), ("reserved", C.c_uint32)]


class CwVersionResult(C.Structure):
    _fields_ = [("ver", C.c_void_p), ("yarn_len", C.c_void_p), ("max_ts", C.c_void_p)]


class CwDeltaResult(C.Structure):
    _fields_ = [("delta_offsets", _U64P), ("delta_src", C.c_void_p), ("delta_id", C.c_void_p),
                ("delta_cause", C.c_void_p), ("delta_kind", C.c_void_p), ("delta_cause_is_id", C.c_void_p),
                ("ahead", C.c_void_p)]


# every function include/causeweave_sync.h declares -> (restype, argtypes)
SIGNATURES = {"cw_version": abi._batch_call(CwSyncBatch, CwVersionResult),
              "cw_delta": abi._sig("I", "P", CwSyncBatch, "P", CwDeltaResult, "I")}


def bind(L):
    """Apply SIGNATURES to a loaded library (once); WeaveError when it lacks a symbol."""
    if isinstance(L, C.CDLL) and not getattr(L, "_cw_sync_bound", False):
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(L, name):
                raise abi.WeaveError(f"{abi.LIB_PATH} has no {name}: rebuild it")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        L._cw_sync_bound = True
    return L


def lib():
    """abi.lib() with this header's signatures applied."""
    return bind(abi.lib())


@dataclass
class VersionResult:
    """The version vectors of a batch (cw_version)."""
    ver: np.ndarray       # uint64[D << site_bits]: the largest id of each site rank, 0 = none
    yarn_len: np.ndarray  # uint32[D << site_bits]: the nodes of each site rank
    max_ts: np.ndarray    # uint64[D]


@dataclass
class DeltaResult:
    """The nodes above a peer's heads (cw_delta)."""
    delta_offsets: np.ndarray             # uint64[D+1]
    delta_src: np.ndarray                 # uint32[P] doc-local input index, per document in input order
    delta_id: np.ndarray                  # uint64[P]
    delta_cause: np.ndarray | None        # uint64[P], None when the input column was None
    delta_kind: np.ndarray | None         # uint8[P]
    delta_cause_is_id: np.ndarray | None  # uint8[P]
    ahead: np.ndarray                     # uint32[D]: site ranks of which the peer holds more


def _host_batch(doc_offsets, id_key, cause, kind, cause_is_id, layout):
    off = abi._u64(doc_offsets)
    if len(off) < 1:
        raise ValueError("offsets arrays must hold at least one entry")
    ids = abi._u64(id_key)
    cols = [None if x is None else np.ascontiguousarray(x, dt)
            for x, dt in zip((cause, kind, cause_is_id), (np.uint64, np.uint8, np.uint8))]
    N = len(ids)
    if int(off[-1]) != N or any(x is not None and len(x) != N for x in cols):
        raise ValueError("offsets[-1] != number of nodes")
    b = CwSyncBatch(len(off) - 1, abi._u64p(off), abi._ptr(ids), *map(abi._ptr, cols), layout.ts_shift,
                    layout.site_shift, layout.site_bits, 0)
    return b, (off, ids, cols)


def version(w, doc_offsets, id_key, layout) -> VersionResult:
    """Host-memory call."""
    b, keep = _host_batch(doc_offsets, id_key, None, None, None, layout)
    D = b.n_docs
    words = D << layout.site_bits
    ver, yl, mts = np.zeros(max(words, 1), np.uint64), np.zeros(max(words, 1), np.uint32), np.zeros(max(D, 1), np.uint64)
    r = CwVersionResult(abi._ptr(ver), abi._ptr(yl), abi._ptr(mts))
    bind(w._L)
    w._check(w._L.cw_version(w._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST), "cw_version")
    return VersionResult(ver[:words], yl[:words], mts[:D])


def delta(w, doc_offsets, id_key, cause, kind, cause_is_id, layout, have) -> DeltaResult:
    """Host-memory call.  cause / kind / cause_is_id None: that column is not
    gathered.  have: uint64[D << layout.site_bits]."""
    b, keep = _host_batch(doc_offsets, id_key, cause, kind, cause_is_id, layout)
    D, N = b.n_docs, len(keep[1])
    hv = abi._u64(have)
    if len(hv) != D << layout.site_bits:
        raise ValueError("have: one word a document and site rank")
    M = max(N, 1)
    do = np.zeros(D + 1, np.uint64)
    osrc, oid = np.zeros(M, np.uint32), np.zeros(M, np.uint64)
    oca, okd, oci = (None if x is None else np.zeros(M, x.dtype) for x in keep[2])
    ahead = np.zeros(max(D, 1), np.uint32)
    hv1 = hv if len(hv) else np.zeros(1, np.uint64)
    r = CwDeltaResult(abi._u64p(do), abi._ptr(osrc), abi._ptr(oid), abi._ptr(oca), abi._ptr(okd), abi._ptr(oci),
                      abi._ptr(ahead))
    bind(w._L)
    w._check(w._L.cw_delta(w._h, C.byref(b), abi._ptr(hv1), C.byref(r), abi.CW_MEM_HOST), "cw_delta")
    P = int(do[-1])
    cut = lambda x: None if x is None else x[:P]
    return DeltaResult(do, osrc[:P], oid[:P], cut(oca), cut(okd), cut(oci), ahead[:D])


def _device_batch(doc_offsets, ptrs, layout):
    off = abi._u64(doc_offsets)
    if len(off) < 1:
        raise ValueError("offsets arrays must hold at least one entry")
    ptrs = tuple(ptrs) + (None,) * (4 - len(ptrs))
    return CwSyncBatch(len(off) - 1, abi._u64p(off), *map(abi._vp, ptrs[:4]), layout.ts_shift, layout.site_shift,
                       layout.site_bits, 0), off


def version_device(w, doc_offsets, id_ptr, layout, out_ptrs):
    """Device-memory call: raw device pointers.  out_ptrs: a dict of the
    cw_version_result arrays (yarn_len, max_ts optional)."""
    b, off = _device_batch(doc_offsets, (id_ptr,), layout)
    r = CwVersionResult(*[abi._vp(out_ptrs.get(f)) for f, _ in CwVersionResult._fields_])
    bind(w._L)
    w._check(w._L.cw_version(w._h, C.byref(b), C.byref(r), abi.CW_MEM_DEVICE), "cw_version")


def delta_device(w, doc_offsets, ptrs, layout, have_ptr, out_ptrs):
    """Device-memory call: raw device pointers (None = NULL).  ptrs = (id_key,
    cause, kind, cause_is_id), the last three optional; out_ptrs: a dict of the
    cw_delta_result arrays but delta_offsets, every per-node array sized for N.
    Returns the delta offsets (uint64[D+1])."""
    b, off = _device_batch(doc_offsets, ptrs, layout)
    do = np.zeros(len(off), np.uint64)
    r = CwDeltaResult(abi._u64p(do), *[abi._vp(out_ptrs.get(f)) for f, _ in CwDeltaResult._fields_[1:]])
    bind(w._L)
    w._check(w._L.cw_delta(w._h, C.byref(b), abi._vp(have_ptr), C.byref(r), abi.CW_MEM_DEVICE), "cw_delta")
    return do
