"""ctypes binding of include/causeweave_transact.h: cw_transact, transact-
(base/core.cljc:100-252) of a batch of bases: depth-first token streams in, the
nodes of every collection out, in the column layout that cw_insert_*, cw_weave_*,
cw_invert and cw_render_* read.

The signature is applied to the library abi.lib() loads.  ``transact`` (host
arrays in, a TransactResult out) and ``transact_device`` (raw device pointers)
take an abi.Weaver.  There is no fallback: a library without the symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import abi

HEADER = os.path.join(os.path.dirname(abi.HEADER), "causeweave_transact.h")
_U64P = C.POINTER(C.c_uint64)
U32_MAX = 0xFFFFFFFF
STATUS_TX_MALFORMED = 1 << 10
TX_LEAF, TX_STR, TX_OPEN_LIST, TX_OPEN_MAP, TX_CLOSE, TX_PART, TX_ROOT_LIST, TX_ROOT_MAP = range(8)


class CwTransactBatch(C.Structure):
    _fields_ = [("n_docs", C.c_uint64), ("base_doc_offsets", _U64P), ("doc_is_map", C.c_void_p),
                ("ts_shift", C.c_uint32), ("site_shift", C.c_uint32), ("site_bits", C.c_uint32),
                ("reserved", C.c_uint32), ("n_bases", C.c_uint64), ("new_tx", C.c_void_p),
                ("tok_offsets", _U64P), ("tok_kind", C.c_void_p), ("tok_arg", C.c_void_p),
                ("tok_cause", C.c_void_p), ("tok_cause_is_id", C.c_void_p), ("tok_vkind", C.c_void_p)]


class CwTransactResult(C.Structure):
    _fields_ = [("new_cap", C.c_uint64), ("node_cap", C.c_uint64), ("base_new_offsets", _U64P),
                ("base_node_offsets", _U64P), ("node_offsets", _U64P), ("node_id", C.c_void_p),
                ("node_cause", C.c_void_p), ("node_cause_is_id", C.c_void_p), ("node_kind", C.c_void_p),
                ("node_src", C.c_void_p), ("node_sub", C.c_void_p), ("node_ref", C.c_void_p),
                ("node_run", C.c_void_p), ("new_is_map", C.c_void_p), ("new_open", C.c_void_p),
                ("root_doc", C.c_void_p), ("base_status", C.c_void_p)]


# the per-node and per-collection arrays of cw_transact_result and their element types
NODE_COLUMNS = (("node_id", np.uint64), ("node_cause", np.uint64), ("node_cause_is_id", np.uint8),
                ("node_kind", np.uint8), ("node_src", np.uint32), ("node_sub", np.uint32), ("node_ref", np.uint32),
                ("node_run", np.uint8))
NEW_COLUMNS = (("new_is_map", np.uint8), ("new_open", np.uint32))

# every function include/causeweave_transact.h declares -> (restype, argtypes)
SIGNATURES = {"cw_transact": abi._batch_call(CwTransactBatch, CwTransactResult)}


def bind(L):
    """Apply SIGNATURES to a loaded library (once); WeaveError when it lacks a symbol."""
    if isinstance(L, C.CDLL) and not getattr(L, "_cw_transact_bound", False):
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(L, name):
                raise abi.WeaveError(f"{abi.LIB_PATH} has no {name}: rebuild it")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        L._cw_transact_bound = True
    return L


def lib():
    """abi.lib() with this header's signatures applied."""
    return bind(abi.lib())


@dataclass
class TransactResult:
    """The nodes that the transactions of every base make (cw_transact)."""
    base_new_offsets: np.ndarray        # uint64[G+1]: the new collections of base g
    base_node_offsets: np.ndarray       # uint64[G+1]: the nodes of base g counted, roots included
    node_offsets: np.ndarray            # uint64[D+C+1] (count-only with C > new_cap: D+new_cap+1)
    node_id: np.ndarray | None          # uint64[M]; the node and collection arrays are None after the count-only call
    node_cause: np.ndarray | None       # uint64[M]
    node_cause_is_id: np.ndarray | None  # uint8[M]
    node_kind: np.ndarray | None        # uint8[M]
    node_src: np.ndarray | None         # uint32[M] the token that made the node
    node_sub: np.ndarray | None         # uint32[M] the character within its STR
    node_ref: np.ndarray | None         # uint32[M] the document a ref node names, else U32_MAX
    node_run: np.ndarray | None         # uint8[M] 1 on the first node of each insert
    new_is_map: np.ndarray | None       # uint8[C]
    new_open: np.ndarray | None         # uint32[C] the token that opens the collection
    root_doc: np.ndarray                # uint32[G] the document of the base's last ROOT_*, else U32_MAX
    base_status: np.ndarray             # uint32[G] 0, STATUS_TX_MALFORMED or abi.STATUS_KEY_RANGE


def _token_columns(tok_kind, tok_arg, tok_cause, tok_cause_is_id, tok_vkind):
    cols = [np.ascontiguousarray(x, dt) for x, dt in
            zip((tok_kind, tok_arg, tok_cause, tok_cause_is_id), (np.uint8, np.uint32, np.uint64, np.uint8))]
    cols.append(None if tok_vkind is None else np.ascontiguousarray(tok_vkind, np.uint8))
    return cols


def transact(w, base_doc_offsets, doc_is_map, layout, new_tx, tok_offsets, tok_kind, tok_arg, tok_cause,
             tok_cause_is_id, tok_vkind=None, new_cap=None, node_cap=None, nodes=True) -> TransactResult:
    """Host-memory call.  nodes False: the count-only call.  new_cap / node_cap
    None: the counts are taken first (a count-only call) and the arrays sized
    from them."""
    doff, toff = abi._u64(base_doc_offsets), abi._u64(tok_offsets)
    if len(doff) < 1 or len(doff) != len(toff):
        raise ValueError("base_doc_offsets and tok_offsets: one entry a base and one more")
    ism, ntx = np.ascontiguousarray(doc_is_map, np.uint8), abi._u64(new_tx)
    cols = _token_columns(tok_kind, tok_arg, tok_cause, tok_cause_is_id, tok_vkind)
    G, D, T = len(doff) - 1, len(ism), len(cols[0])
    if int(doff[-1]) != D or int(toff[-1]) != T or any(x is not None and len(x) != T for x in cols) or len(ntx) != G:
        raise ValueError("offsets[-1] != number of documents / tokens, or new_tx is not one entry a base")
    if nodes and (new_cap is None or node_cap is None):
        counts = transact(w, doff, ism, layout, ntx, toff, *cols, new_cap=T, nodes=False)
        new_cap = int(counts.base_new_offsets[-1]) if new_cap is None else new_cap
        node_cap = int(counts.base_node_offsets[-1]) if node_cap is None else node_cap
    new_cap, node_cap = int(new_cap or 0), int(node_cap or 0)
    b = CwTransactBatch(D, abi._u64p(doff), abi._ptr(ism), layout.ts_shift, layout.site_shift, layout.site_bits, 0,
                        G, abi._ptr(ntx), abi._u64p(toff), *map(abi._ptr, cols))
    bn, bm = np.zeros(G + 1, np.uint64), np.zeros(G + 1, np.uint64)
    no = np.zeros(D + new_cap + 1, np.uint64)
    ncol = [np.zeros(max(node_cap, 1), dt) if nodes else None for _, dt in NODE_COLUMNS]
    ccol = [np.zeros(max(new_cap, 1), dt) if nodes else None for _, dt in NEW_COLUMNS]
    root, st = np.zeros(max(G, 1), np.uint32), np.zeros(max(G, 1), np.uint32)
    r = CwTransactResult(new_cap, node_cap, abi._u64p(bn), abi._u64p(bm), abi._u64p(no), *map(abi._ptr, ncol),
                         *map(abi._ptr, ccol), abi._ptr(root), abi._ptr(st))
    bind(w._L)
    w._check(w._L.cw_transact(w._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST), "cw_transact")
    Cn, M = int(bn[-1]), int(bm[-1])
    cut = lambda xs, n: [x[:n] if nodes else None for x in xs]
    return TransactResult(bn, bm, no[:D + min(Cn, new_cap) + 1], *cut(ncol, M), *cut(ccol, Cn), root[:G], st[:G])


def transact_device(w, base_doc_offsets, doc_is_map_ptr, layout, new_tx_ptr, tok_offsets, tok_ptrs, new_cap,
                    node_cap, out_ptrs):
    """Device-memory call: raw device pointers (None = NULL).  tok_ptrs =
    (tok_kind, tok_arg, tok_cause, tok_cause_is_id, tok_vkind); out_ptrs: a dict
    of the cw_transact_result arrays but the three offset arrays, the node arrays
    sized for node_cap, the collection arrays for new_cap.  Returns
    (base_new_offsets, base_node_offsets, node_offsets), the last with
    n_docs + min(new_cap, T) + 1 entries."""
    doff, toff = abi._u64(base_doc_offsets), abi._u64(tok_offsets)
    if len(doff) < 1 or len(doff) != len(toff):
        raise ValueError("base_doc_offsets and tok_offsets: one entry a base and one more")
    G, D, T = len(doff) - 1, int(doff[-1]), int(toff[-1])
    b = CwTransactBatch(D, abi._u64p(doff), abi._vp(doc_is_map_ptr), layout.ts_shift, layout.site_shift,
                        layout.site_bits, 0, G, abi._vp(new_tx_ptr), abi._u64p(toff), *map(abi._vp, tok_ptrs[:5]))
    bn, bm = np.zeros(G + 1, np.uint64), np.zeros(G + 1, np.uint64)
    no = np.zeros(D + min(int(new_cap), T) + 1, np.uint64)
    r = CwTransactResult(int(new_cap), int(node_cap), abi._u64p(bn), abi._u64p(bm), abi._u64p(no),
                         *[abi._vp(out_ptrs.get(f)) for f, _ in CwTransactResult._fields_[5:]])
    bind(w._L)
    w._check(w._L.cw_transact(w._h, C.byref(b), C.byref(r), abi.CW_MEM_DEVICE), "cw_transact")
    return bn, bm, no
