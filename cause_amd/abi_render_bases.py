"""ctypes binding of include/causeweave_render_bases.h: cw_render_bases, cb->edn
(base/core.cljc:83-96) of a batch of bases as depth-first token streams over
the entry table that cw_render_lists / cw_render_maps make.

The signature is applied to the library abi.lib() loads.  ``render_bases``
(host arrays in, a RenderBasesResult out) and ``render_bases_device`` (raw
device pointers) take an abi.Weaver.  There is no fallback: a library without
the symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import abi

HEADER = os.path.join(os.path.dirname(abi.HEADER), "causeweave_render_bases.h")
_U64P = C.POINTER(C.c_uint64)
U32_MAX = 0xFFFFFFFF
STATUS_REF_SHARED = 1 << 9
TOK_OPEN, TOK_CLOSE, TOK_LEAF, TOK_NIL = 0, 1, 2, 3


class CwRenderBasesBatch(C.Structure):
    _fields_ = [("n_docs", C.c_uint64), ("ent_offsets", _U64P), ("ent_ref", C.c_void_p),
                ("n_bases", C.c_uint64), ("root_doc", C.c_void_p)]


class CwRenderBasesResult(C.Structure):
    _fields_ = [("base_tok_offsets", _U64P), ("tok_kind", C.c_void_p), ("tok_doc", C.c_void_p),
                ("tok_entry", C.c_void_p), ("base_status", C.c_void_p), ("doc_base", C.c_void_p),
                ("doc_open", C.c_void_p)]


# every function include/causeweave_render_bases.h declares -> (restype, argtypes)
SIGNATURES = {"cw_render_bases": abi._batch_call(CwRenderBasesBatch, CwRenderBasesResult)}


def bind(L):
    """Apply SIGNATURES to a loaded library (once); WeaveError when it lacks a symbol."""
    if isinstance(L, C.CDLL) and not getattr(L, "_cw_render_bases_bound", False):
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(L, name):
                raise abi.WeaveError(f"{abi.LIB_PATH} has no {name}: rebuild it")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        L._cw_render_bases_bound = True
    return L


def lib():
    """abi.lib() with this header's signatures applied."""
    return bind(abi.lib())


@dataclass
class RenderBasesResult:
    """The token stream of every base (cw_render_bases)."""
    base_tok_offsets: np.ndarray   # uint64[G+1]: the tokens of base g
    tok_kind: np.ndarray | None    # uint8[T] TOK_*; None after the count-only call
    tok_doc: np.ndarray | None     # uint32[T]
    tok_entry: np.ndarray | None   # uint32[T] LEAF / NIL: the entry; OPEN / CLOSE: the referring entry, U32_MAX for a root
    base_status: np.ndarray        # uint32[G] 0 or STATUS_REF_SHARED
    doc_base: np.ndarray           # uint32[D] the base that reaches d, U32_MAX if none or flagged
    doc_open: np.ndarray           # uint32[D] d's OPEN; unspecified where doc_base is U32_MAX


def render_bases(w, ent_offsets, ent_ref, root_doc, tokens=True) -> RenderBasesResult:
    """Host-memory call.  tokens False: the count-only call."""
    off = abi._u64(ent_offsets)
    ref, root = np.ascontiguousarray(ent_ref, np.uint32), np.ascontiguousarray(root_doc, np.uint32)
    if len(off) < 1:
        raise ValueError("ent_offsets must hold at least one entry")
    D, G, E = len(off) - 1, len(root), len(ref)
    if int(off[-1]) != E:
        raise ValueError("ent_offsets[-1] != number of entries")
    b = CwRenderBasesBatch(D, abi._u64p(off), abi._ptr(ref), G, abi._ptr(root))
    cap = max(E + 2 * D, 1)
    bo = np.zeros(G + 1, np.uint64)
    kind = doc = ent = None
    if tokens:
        kind, doc, ent = np.zeros(cap, np.uint8), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    st, db, do = np.zeros(max(G, 1), np.uint32), np.zeros(max(D, 1), np.uint32), np.zeros(max(D, 1), np.uint32)
    r = CwRenderBasesResult(abi._u64p(bo), abi._ptr(kind), abi._ptr(doc), abi._ptr(ent), abi._ptr(st), abi._ptr(db),
                            abi._ptr(do))
    bind(w._L)
    w._check(w._L.cw_render_bases(w._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST), "cw_render_bases")
    T = int(bo[-1])
    cut = (lambda x: x[:T]) if tokens else (lambda x: None)
    return RenderBasesResult(bo, cut(kind), cut(doc), cut(ent), st[:G], db[:D], do[:D])


def render_bases_device(w, ent_offsets, ent_ref_ptr, n_bases, root_doc_ptr, out_ptrs):
    """Device-memory call: raw device pointers (None = NULL).  out_ptrs: a dict of
    the cw_render_bases_result arrays but base_tok_offsets, the token arrays
    sized for E + 2 * n_docs.  Returns the base token offsets (uint64[G+1])."""
    off = abi._u64(ent_offsets)
    if len(off) < 1:
        raise ValueError("ent_offsets must hold at least one entry")
    b = CwRenderBasesBatch(len(off) - 1, abi._u64p(off), abi._vp(ent_ref_ptr), n_bases, abi._vp(root_doc_ptr))
    bo = np.zeros(n_bases + 1, np.uint64)
    r = CwRenderBasesResult(abi._u64p(bo), *[abi._vp(out_ptrs.get(f)) for f, _ in CwRenderBasesResult._fields_[1:]])
    bind(w._L)
    w._check(w._L.cw_render_bases(w._h, C.byref(b), C.byref(r), abi.CW_MEM_DEVICE), "cw_render_bases")
    return bo
