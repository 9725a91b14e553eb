"""ctypes binding of include/causeweave_insert.h: cw_insert_lists, the
incremental list insert (c.list/weave's 2/3-arity over s/weave-node).

The structs nest abi.CwListBatch and abi.CwListResult; the signature is applied
to the library abi.lib() loads.  ``insert_lists`` (host arrays in, an
InsertResult out) and ``insert_lists_device`` (raw device pointers) take an
abi.Weaver.  There is no fallback: a library without the symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import abi

HEADER = os.path.join(os.path.dirname(abi.HEADER), "causeweave_insert.h")
_U64P = C.POINTER(C.c_uint64)


class CwInsertBatch(C.Structure):
    _fields_ = [("docs", abi.CwListBatch), ("weave_perm", C.c_void_p), ("visible_bits", C.c_void_p),
                ("yarn_perm", C.c_void_p), ("doc_value", C.c_void_p), ("tx_offsets", _U64P),
                ("tx_id", C.c_void_p), ("tx_cause", C.c_void_p), ("tx_kind", C.c_void_p),
                ("tx_value", C.c_void_p)]


class CwInsertResult(C.Structure):
    _fields_ = [("new_offsets", _U64P), ("insert_pos", C.c_void_p), ("weave", abi.CwListResult),
                ("id_key", C.c_void_p), ("cause_key", C.c_void_p), ("kind", C.c_void_p),
                ("value", C.c_void_p)]


# every function include/causeweave_insert.h declares -> (restype, argtypes)
SIGNATURES = {"cw_insert_lists": abi._batch_call(CwInsertBatch, CwInsertResult)}


def bind(L):
    """Apply SIGNATURES to a loaded library (once); WeaveError when it lacks a symbol."""
    if isinstance(L, C.CDLL) and not getattr(L, "_cw_insert_bound", False):
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(L, name):
                raise abi.WeaveError(f"{abi.LIB_PATH} has no {name}: rebuild it")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        L._cw_insert_bound = True
    return L


def lib():
    """abi.lib() with this header's signatures applied."""
    return bind(abi.lib())


@dataclass
class InsertResult:
    """The documents after one tx each (cw_insert_lists)."""
    offsets: np.ndarray            # uint64[D+1] the new documents
    insert_pos: np.ndarray         # uint32[D] doc-local weave position of the tx, UINT32_MAX = none
    weave: abi.ListResult          # indices: s < n_d old input index, s >= n_d tx node s - n_d
    id_key: np.ndarray | None      # uint64[M] the new documents' columns: old nodes, then the tx
    cause_key: np.ndarray | None
    kind: np.ndarray | None
    value: np.ndarray | None


def insert_lists(w, docs, weave_perm, visible_bits, tx, layout, yarn_perm=None, doc_value=None,
                 columns=True) -> InsertResult:
    """Host-memory call.  docs = (offsets, id_key, cause_key, kind) of the woven
    documents, weave_perm / visible_bits / yarn_perm their cw_list_result
    arrays; tx = (tx_offsets, tx_id, tx_cause, tx_kind[, tx_value]) with
    tx_value exactly when doc_value is given.  yarn_perm None: no yarn output.
    columns: also return the new documents' node columns."""
    what = "offsets[-1] != number of nodes"
    off, cols = abi._host_nodes(docs[0], docs[1:4], abi._LIST_DT, what)
    toff, tcols = abi._host_nodes(tx[0], tx[1:4], abi._LIST_DT, what)
    if len(off) != len(toff):
        raise ValueError("docs and tx must have the same number of documents")
    D, N, T = len(off) - 1, len(cols[0]), len(tcols[0])
    perm = np.ascontiguousarray(weave_perm, np.uint32)
    bits = np.ascontiguousarray(visible_bits, np.uint32)
    yarn = None if yarn_perm is None else np.ascontiguousarray(yarn_perm, np.uint32)
    val = None if doc_value is None else abi._u64(doc_value)
    tval = abi._u64(tx[4]) if len(tx) > 4 and tx[4] is not None else None
    if (val is None) != (tval is None):
        raise ValueError("doc_value and tx_value go together")
    if len(perm) != N or len(bits) < (N + 31) // 32 or (yarn is not None and len(yarn) != N) or \
            (val is not None and (len(val) != N or len(tval) != T)):
        raise ValueError("weave_perm / visible_bits / yarn_perm / value sizes differ from the nodes")
    lb, off = w._batch(off, *map(abi._ptr, cols), layout)
    b = CwInsertBatch(lb, abi._ptr(perm), abi._ptr(bits), abi._ptr(yarn), abi._ptr(val),
                      abi._u64p(toff), *map(abi._ptr, tcols), abi._ptr(tval))
    M = max(N + T, 1)
    offs, pos = np.zeros(D + 1, np.uint64), np.zeros(max(D, 1), np.uint32)
    out, wr = abi._new_list_result(M, (M + 31) // 32, max(D, 1), yarn is not None)
    oc = [np.zeros(M, dt) if columns else None for dt in abi._LIST_DT]
    oval = np.zeros(M, np.uint64) if columns and val is not None else None
    r = CwInsertResult(abi._u64p(offs), abi._ptr(pos), wr, *map(abi._ptr, oc), abi._ptr(oval))
    bind(w._L)
    w._check(w._L.cw_insert_lists(w._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST), "cw_insert_lists")
    m = int(offs[-1])
    cut = lambda a: None if a is None else a[:m]
    return InsertResult(offs, pos[:D], abi._trim_list_result(out, m, D), cut(oc[0]), cut(oc[1]),
                        cut(oc[2]), cut(oval))


def insert_lists_device(w, offsets, ptrs, perm_ptr, bits_ptr, tx_offsets, tx_ptrs, layout, out_ptrs,
                        pos_ptr=None, yarn_ptr=None, value_ptr=None, col_ptrs=None):
    """Device-memory call: raw device pointers (None = NULL).  ptrs = (id_key,
    cause_key, kind) of the documents; tx_ptrs = (tx_id, tx_cause, tx_kind[,
    tx_value]); out_ptrs as Weaver.weave_lists_device, every per-node array
    sized for N + T; pos_ptr: insert_pos; col_ptrs = (id_key, cause_key, kind[,
    value]) outputs.  Returns the new offsets (uint64[D+1])."""
    off, toff = abi._u64(offsets), abi._u64(tx_offsets)
    if len(off) != len(toff):
        raise ValueError("docs and tx must have the same number of documents")
    lb, off = w._batch(off, *map(abi._vp, ptrs[:3]), layout)
    txp = list(tx_ptrs) + [None] * (4 - len(tx_ptrs))
    b = CwInsertBatch(lb, abi._vp(perm_ptr), abi._vp(bits_ptr), abi._vp(yarn_ptr), abi._vp(value_ptr),
                      abi._u64p(toff), *map(abi._vp, txp))
    offs = np.zeros(len(off), np.uint64)
    cp = list(col_ptrs or ()) + [None] * (4 - len(col_ptrs or ()))
    r = CwInsertResult(abi._u64p(offs), abi._vp(pos_ptr), abi._list_result(out_ptrs), *map(abi._vp, cp))
    bind(w._L)
    w._check(w._L.cw_insert_lists(w._h, C.byref(b), C.byref(r), abi.CW_MEM_DEVICE), "cw_insert_lists")
    return offs
