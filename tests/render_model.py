"""numpy model of cw_render_lists / cw_render_maps (include/causeweave.h): the
reference's filter over a weave's result arrays, nothing else.

Lists: the rendered nodes are the weave positions whose visible bit is set,
in weave order; a document's offset is the number of set bits below its first
position; values come by fancy indexing, 0 where weave_perm points outside the
document.  Maps: the same over seg_active >= 0.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class Rendered:
    offsets: np.ndarray        # uint64[D+1]
    src: np.ndarray            # uint32[R]
    value: np.ndarray | None   # [R], the value column's dtype
    key: np.ndarray | None = None  # maps: uint64[R]


def flags(visible_bits, n):
    """uint8[n]: bit g of the bitmap (bits at positions >= n are ignored)."""
    b = np.ascontiguousarray(visible_bits, np.uint32)
    return np.unpackbits(b.view(np.uint8), bitorder="little")[:n]


def pack_bits(vis, ones_above=False):
    """uint32[(n+31)//32] bitmap of the flags; ones_above: the bits past n set."""
    vis = np.asarray(vis, np.uint8)
    n = len(vis)
    pad = np.full((-n) % 32, 1 if ones_above else 0, np.uint8)
    return np.packbits(np.concatenate([vis, pad]), bitorder="little").view(np.uint32).copy()


def _gather(value, base, size, src):
    ok = src.astype(np.int64) < size
    idx = np.where(ok, base + src.astype(np.int64), 0)
    out = value[idx] if len(value) else np.zeros(len(idx), value.dtype)
    return np.where(ok, out, 0).astype(value.dtype)


def render_lists(offsets, weave_perm, visible_bits, value=None) -> Rendered:
    off = np.asarray(offsets, np.int64)
    perm = np.asarray(weave_perm).astype(np.uint32)
    n = int(off[-1])
    on = flags(visible_bits, n) == 1
    below = np.concatenate([[0], np.cumsum(on)])
    val = None
    if value is not None:
        value = np.asarray(value)
        doc = np.repeat(np.arange(len(off) - 1), np.diff(off))
        val = _gather(value, off[doc], np.diff(off)[doc], perm)[on]
    return Rendered(below[off].astype(np.uint64), perm[on], val)


def render_maps(n_colls, seg_coll, seg_key, seg_active, coll_offsets=None, value=None) -> Rendered:
    coll = np.asarray(seg_coll, np.int64)
    act = np.asarray(seg_active, np.int64)
    on = act >= 0
    counts = np.bincount(coll[on], minlength=n_colls)
    src = np.minimum(np.where(on, act, 0), 0xFFFFFFFF).astype(np.uint32)  # (UINT32_MAX: no index)
    val = None
    if value is not None:
        value = np.asarray(value)
        co = np.asarray(coll_offsets, np.int64)
        val = _gather(value, co[coll], np.diff(co)[coll], src)[on]
    return Rendered(np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), src[on], val,
                    np.asarray(seg_key, np.uint64)[on])
