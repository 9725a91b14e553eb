"""ctypes binding of include/causeweave_map_insert.h: cw_insert_maps, the
incremental map insert (c.map/weave's 2/3-arity over s/weave-node).

The structs nest abi.CwMapBatch and abi.CwMapResult; the signature is applied
to the library abi.lib() loads.  ``insert_maps`` (host arrays in, a
MapInsertResult out) and ``insert_maps_device`` (raw device pointers) take an
abi.Weaver.  There is no fallback: a library without the symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import abi

HEADER = os.path.join(os.path.dirname(abi.HEADER), "causeweave_map_insert.h")
_U64P = C.POINTER(C.c_uint64)
_SEG_DT = (np.uint64, np.uint32, np.uint64, np.int64, np.uint32)  # seg_offsets .. seg_perm


class CwMapInsertBatch(C.Structure):
    _fields_ = [("colls", abi.CwMapBatch), ("n_segs", C.c_uint64), ("seg_offsets", C.c_void_p),
                ("seg_coll", C.c_void_p), ("seg_key", C.c_void_p), ("seg_active", C.c_void_p),
                ("seg_perm", C.c_void_p), ("coll_value", C.c_void_p), ("tx_offsets", _U64P),
                ("tx_id", C.c_void_p), ("tx_cause", C.c_void_p), ("tx_cause_is_id", C.c_void_p),
                ("tx_kind", C.c_void_p), ("tx_value", C.c_void_p)]


class CwMapInsertResult(C.Structure):
    _fields_ = [("new_offsets", _U64P), ("tx_seg", C.c_void_p), ("tx_pos", C.c_void_p),
                ("maps", abi.CwMapResult), ("id_key", C.c_void_p), ("cause", C.c_void_p),
                ("cause_is_id", C.c_void_p), ("kind", C.c_void_p), ("value", C.c_void_p)]


# every function include/causeweave_map_insert.h declares -> (restype, argtypes)
SIGNATURES = {"cw_insert_maps": abi._batch_call(CwMapInsertBatch, CwMapInsertResult)}


def bind(L):
    """Apply SIGNATURES to a loaded library (once); WeaveError when it lacks a symbol."""
    if isinstance(L, C.CDLL) and not getattr(L, "_cw_map_insert_bound", False):
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(L, name):
                raise abi.WeaveError(f"{abi.LIB_PATH} has no {name}: rebuild it")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        L._cw_map_insert_bound = True
    return L


def lib():
    """abi.lib() with this header's signatures applied."""
    return bind(abi.lib())


@dataclass
class MapInsertResult:
    """The collections after one tx each (cw_insert_maps)."""
    offsets: np.ndarray            # uint64[D+1] the new collections
    tx_seg: np.ndarray             # uint32[T] key weave of each tx node, UINT32_MAX = not inserted
    tx_pos: np.ndarray             # uint32[T] its position there (root = 0)
    maps: abi.MapResult            # indices: s < n_d old input index, s >= n_d tx node s - n_d
    id_key: np.ndarray | None      # uint64[M] the new collections' columns: old nodes, then the tx
    cause: np.ndarray | None
    cause_is_id: np.ndarray | None
    kind: np.ndarray | None
    value: np.ndarray | None


def insert_maps(w, colls, segs, tx, coll_value=None, columns=True) -> MapInsertResult:
    """Host-memory call.  colls = (offsets, id_key, cause, cause_is_id, kind) of the
    woven collections; segs = (seg_offsets, seg_coll, seg_key, seg_active,
    seg_perm), their cw_map_result (an abi.MapResult does too); tx = (tx_offsets,
    tx_id, tx_cause, tx_cause_is_id, tx_kind[, tx_value]) with tx_value exactly
    when coll_value is given.  columns: also return the new collections' node
    columns."""
    what = "offsets[-1] != number of nodes"
    off, cols = abi._host_nodes(colls[0], colls[1:5], abi._MAP_DT, what)
    toff, tcols = abi._host_nodes(tx[0], tx[1:5], abi._MAP_DT, what)
    if len(off) != len(toff):
        raise ValueError("colls and tx must have the same number of collections")
    if isinstance(segs, abi.MapResult):
        segs = (segs.seg_offsets, segs.seg_coll, segs.seg_key, segs.seg_active, segs.seg_perm)
    sg = [np.ascontiguousarray(x, dt) for x, dt in zip(segs, _SEG_DT)]
    D, N, T, S = len(off) - 1, len(cols[0]), len(tcols[0]), len(sg[1])
    val = None if coll_value is None else abi._u64(coll_value)
    tval = abi._u64(tx[5]) if len(tx) > 5 and tx[5] is not None else None
    if (val is None) != (tval is None):
        raise ValueError("coll_value and tx_value go together")
    if len(sg[0]) != S + 1 or len(sg[2]) != S or len(sg[3]) != S or len(sg[4]) != N + S or \
            (val is not None and (len(val) != N or len(tval) != T)):
        raise ValueError("seg / value array sizes differ from the nodes and key weaves")
    mb = w._map_batch(off, [abi._ptr(x) for x in cols], 0, 0)
    b = CwMapInsertBatch(mb, S, *map(abi._ptr, sg), abi._ptr(val), abi._u64p(toff),
                         *map(abi._ptr, tcols), abi._ptr(tval))
    M = max(N + T, 1)
    offs = np.zeros(D + 1, np.uint64)
    seg, pos = np.zeros(max(T, 1), np.uint32), np.zeros(max(T, 1), np.uint32)
    out, mr = abi._new_map_result(max(S + T, 1), N + T, D)
    oc = [np.zeros(M, dt) if columns else None for dt in abi._MAP_DT]
    oval = np.zeros(M, np.uint64) if columns and val is not None else None
    r = CwMapInsertResult(abi._u64p(offs), abi._ptr(seg), abi._ptr(pos), mr, *map(abi._ptr, oc),
                          abi._ptr(oval))
    bind(w._L)
    w._check(w._L.cw_insert_maps(w._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST), "cw_insert_maps")
    m = int(offs[-1])
    cut = lambda a: None if a is None else a[:m]
    return MapInsertResult(offs, seg[:T], pos[:T], abi._trim_map_result(out, int(r.maps.n_segs), m, D),
                           cut(oc[0]), cut(oc[1]), cut(oc[2]), cut(oc[3]), cut(oval))


def insert_maps_device(w, offsets, ptrs, n_segs, seg_ptrs, tx_offsets, tx_ptrs, out_ptrs, cap_segs,
                       tx_seg_ptr=None, tx_pos_ptr=None, value_ptr=None, col_ptrs=None):
    """Device-memory call: raw device pointers (None = NULL).  ptrs = (id_key,
    cause, cause_is_id, kind) of the collections; seg_ptrs = (seg_offsets,
    seg_coll, seg_key, seg_active, seg_perm); tx_ptrs = (tx_id, tx_cause,
    tx_cause_is_id, tx_kind[, tx_value]); out_ptrs as Weaver.weave_maps_device
    (seg_perm sized N + T + cap_segs); col_ptrs = (id_key, cause, cause_is_id,
    kind[, value]) outputs.  Returns (the new offsets uint64[D+1], n_segs)."""
    off, toff = abi._u64(offsets), abi._u64(tx_offsets)
    if len(off) != len(toff):
        raise ValueError("colls and tx must have the same number of collections")
    mb = w._map_batch(off, [abi._vp(p) for p in ptrs[:4]], 0, 0)
    txp = list(tx_ptrs) + [None] * (5 - len(tx_ptrs))
    b = CwMapInsertBatch(mb, n_segs, *map(abi._vp, seg_ptrs), abi._vp(value_ptr), abi._u64p(toff),
                         *map(abi._vp, txp))
    offs = np.zeros(len(off), np.uint64)
    cp = list(col_ptrs or ()) + [None] * (5 - len(col_ptrs or ()))
    r = CwMapInsertResult(abi._u64p(offs), abi._vp(tx_seg_ptr), abi._vp(tx_pos_ptr),
                          abi._map_result(out_ptrs, cap_segs), *map(abi._vp, cp))
    bind(w._L)
    w._check(w._L.cw_insert_maps(w._h, C.byref(b), C.byref(r), abi.CW_MEM_DEVICE), "cw_insert_maps")
    return offs, int(r.maps.n_segs)
