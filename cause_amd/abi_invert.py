"""ctypes binding of include/causeweave_invert.h: cw_invert, the inverting
transaction of a slice of history (invert-, base/core.cljc:313-343; what undo-,
redo- and reset- end in).

The signature is applied to the library abi.lib() loads.  ``invert`` (host
arrays in, an InvertResult out) and ``invert_device`` (raw device pointers)
take an abi.Weaver.  There is no fallback: a library without the symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import abi

HEADER = os.path.join(os.path.dirname(abi.HEADER), "causeweave_invert.h")
_U64P = C.POINTER(C.c_uint64)
U32_MAX = 0xFFFFFFFF


class CwInvertBatch(C.Structure):
    _fields_ = [("n_docs", C.c_uint64), ("doc_offsets", _U64P), ("id_key", C.c_void_p), ("cause", C.c_void_p),
                ("kind", C.c_void_p), ("cause_is_id", C.c_void_p), ("ref_doc", C.c_void_p),
                ("ts_shift", C.c_uint32), ("site_shift", C.c_uint32), ("site_bits", C.c_uint32),
                ("reserved", C.c_uint32), ("n_bases", C.c_uint64), ("base_offsets", _U64P),
                ("sel_lo", C.c_void_p), ("sel_hi", C.c_void_p), ("sel_sites", C.c_void_p),
                ("new_tx", C.c_void_p)]


class CwInvertResult(C.Structure):
    _fields_ = [("part_offsets", _U64P), ("inv_id", C.c_void_p), ("inv_cause", C.c_void_p),
                ("inv_cause_is_id", C.c_void_p), ("inv_kind", C.c_void_p), ("inv_src", C.c_void_p),
                ("base_parts", C.c_void_p), ("status", C.c_void_p)]


# every function include/causeweave_invert.h declares -> (restype, argtypes)
SIGNATURES = {"cw_invert": abi._batch_call(CwInvertBatch, CwInvertResult)}


def bind(L):
    """Apply SIGNATURES to a loaded library (once); WeaveError when it lacks a symbol."""
    if isinstance(L, C.CDLL) and not getattr(L, "_cw_invert_bound", False):
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(L, name):
                raise abi.WeaveError(f"{abi.LIB_PATH} has no {name}: rebuild it")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        L._cw_invert_bound = True
    return L


def lib():
    """abi.lib() with this header's signatures applied."""
    return bind(abi.lib())


def mask_words(site_bits: int) -> int:
    """64-bit words of sel_sites per base."""
    return ((1 << site_bits) + 63) // 64


@dataclass
class InvertResult:
    """The inverting transaction of every base (cw_invert)."""
    part_offsets: np.ndarray            # uint64[D+1]: the parts of document d, ascending tx-index
    inv_id: np.ndarray                  # uint64[P]
    inv_cause: np.ndarray               # uint64[P]
    inv_cause_is_id: np.ndarray | None  # uint8[P], None when the input column was None
    inv_kind: np.ndarray                # uint8[P] h.hide (2) / h.show (3)
    inv_src: np.ndarray                 # uint32[P] doc-local input index of the node the part was made from
    base_parts: np.ndarray              # uint32[G]
    status: np.ndarray                  # uint32[D] 0 or STATUS_KEY_RANGE


def invert(w, doc_offsets, id_key, cause, kind, cause_is_id, ref_doc, layout, base_offsets, sel_lo, sel_hi,
           sel_sites, new_tx) -> InvertResult:
    """Host-memory call.  cause_is_id None: a batch of lists; ref_doc None: no
    references.  sel_sites: uint64[G * mask_words(layout.site_bits)]."""
    off, boff = abi._u64(doc_offsets), abi._u64(base_offsets)
    cols = [np.ascontiguousarray(x, dt) for x, dt in zip((id_key, cause, kind), abi._LIST_DT)]
    cii = None if cause_is_id is None else np.ascontiguousarray(cause_is_id, np.uint8)
    ref = None if ref_doc is None else np.ascontiguousarray(ref_doc, np.uint32)
    sel = [abi._u64(x) for x in (sel_lo, sel_hi, sel_sites, new_tx)]
    if len(off) < 1 or len(boff) < 1:
        raise ValueError("offsets arrays must hold at least one entry")
    D, G, N = len(off) - 1, len(boff) - 1, len(cols[0])
    if int(off[-1]) != N or any(x is not None and len(x) != N for x in (cols[1], cols[2], cii, ref)):
        raise ValueError("offsets[-1] != number of nodes")
    W = mask_words(layout.site_bits)
    if len(sel[0]) != G or len(sel[1]) != G or len(sel[3]) != G or len(sel[2]) != G * W:
        raise ValueError("sel_lo, sel_hi, new_tx: one entry a base; sel_sites: mask_words(site_bits) a base")
    b = CwInvertBatch(D, abi._u64p(off), *map(abi._ptr, cols), abi._ptr(cii), abi._ptr(ref), layout.ts_shift,
                      layout.site_shift, layout.site_bits, 0, G, abi._u64p(boff), *map(abi._ptr, sel))
    M = max(N, 1)
    po = np.zeros(D + 1, np.uint64)
    oid, oca, okd = np.zeros(M, np.uint64), np.zeros(M, np.uint64), np.zeros(M, np.uint8)
    oci = None if cii is None else np.zeros(M, np.uint8)
    osrc, obp, ost = np.zeros(M, np.uint32), np.zeros(max(G, 1), np.uint32), np.zeros(max(D, 1), np.uint32)
    r = CwInvertResult(abi._u64p(po), abi._ptr(oid), abi._ptr(oca), abi._ptr(oci), abi._ptr(okd), abi._ptr(osrc),
                       abi._ptr(obp), abi._ptr(ost))
    bind(w._L)
    w._check(w._L.cw_invert(w._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST), "cw_invert")
    P = int(po[-1])
    return InvertResult(po, oid[:P], oca[:P], None if oci is None else oci[:P], okd[:P], osrc[:P], obp[:G],
                        ost[:D])


def invert_device(w, doc_offsets, ptrs, layout, base_offsets, sel_ptrs, out_ptrs, cause_is_id_ptr=None,
                  ref_doc_ptr=None):
    """Device-memory call: raw device pointers (None = NULL).  ptrs = (id_key,
    cause, kind); sel_ptrs = (sel_lo, sel_hi, sel_sites, new_tx); out_ptrs: a
    dict of the cw_invert_result arrays but part_offsets, every per-node array
    sized for N.  Returns the part offsets (uint64[D+1])."""
    off, boff = abi._u64(doc_offsets), abi._u64(base_offsets)
    if len(off) < 1 or len(boff) < 1:
        raise ValueError("offsets arrays must hold at least one entry")
    b = CwInvertBatch(len(off) - 1, abi._u64p(off), *map(abi._vp, ptrs[:3]), abi._vp(cause_is_id_ptr),
                      abi._vp(ref_doc_ptr), layout.ts_shift, layout.site_shift, layout.site_bits, 0,
                      len(boff) - 1, abi._u64p(boff), *map(abi._vp, sel_ptrs[:4]))
    po = np.zeros(len(off), np.uint64)
    r = CwInvertResult(abi._u64p(po), *[abi._vp(out_ptrs.get(f)) for f, _ in CwInvertResult._fields_[1:]])
    bind(w._L)
    w._check(w._L.cw_invert(w._h, C.byref(b), C.byref(r), abi.CW_MEM_DEVICE), "cw_invert")
    return po
