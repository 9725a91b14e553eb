"""invert- (base/core.cljc:313-343) restated twice, as the checker of cw_invert.

``invert_tx`` / ``transact_parts`` work on node tuples and follow the reference
step by step (paths newest first, the soon-to-be-hidden uuids, invert-path, one
part per [uuid cause] in an insertion-ordered map, one node a part).
``invert_columns`` is the same function over the packed columns of
include/causeweave_invert.h and returns every array the call returns.
``pack_bases`` / ``unpack_parts`` go from one form to the other.  Nothing here
imports cause_amd.base.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from cause_amd import causal as C, pack

REF_NS = "causal.collection.ref"
U32_MAX = 0xFFFFFFFF
STATUS_KEY_RANGE = 1 << 7


def ref(uuid):
    return C.Keyword(REF_NS, uuid)


def is_ref(v):
    return isinstance(v, C.Keyword) and v.ns == REF_NS


def id_key(i):
    """Sort key of an id: the vector compare of util.cljc:4-10."""
    return (i[0], pack.java_str_key(i[1]), i[2])


# ------------------------------------------------------------ node tuples ----
def invert_path(uuid, node):
    """:313-320"""
    nid, cause, value = node
    if value == C.HIDE or value == C.H_HIDE:
        return (uuid, cause, C.H_SHOW)
    if value == C.H_SHOW:
        return (uuid, cause, C.H_HIDE)
    return (uuid, nid, C.H_HIDE)


def invert_tx(collections, history_slice):
    """:322-342 up to the transact-: collections = {uuid: {id: (cause, value)}},
    history_slice = [(id, uuid)] ascending by id -> the tx [(uuid, cause, value)].
    A Python dict keeps a key where it first appeared and takes the last value,
    as the reference's array map does (up to 8 keys; beyond, this order is the
    library's choice)."""
    paths = [(u, (i,) + tuple(collections[u][i])) for i, u in reversed(history_slice)]
    hidden = {n[2].name for _, n in paths if is_ref(n[2])}
    acc = {}
    for u, n in paths:
        if u in hidden:
            continue
        part = invert_path(u, n)
        acc[(u, part[1])] = part
    return list(acc.values())


def transact_parts(tx, lamport_ts, site_id):
    """:232-252 for keyword values: part k becomes the node [lamport-ts site k]."""
    return [(u, ((lamport_ts, site_id, k), cause, value)) for k, (u, cause, value) in enumerate(tx)]


def slice_of(collections, lo, hi, sites):
    """The reverse paths of every non-root node with lo <= id <= hi (None: open)
    and a site in ``sites`` (None: any), ascending."""
    out = []
    for u, nodes in collections.items():
        for i in nodes:
            if i == C.ROOT_ID:
                continue
            k = id_key(i)
            if (lo is None or id_key(lo) <= k) and (hi is None or k <= id_key(hi)) and \
                    (sites is None or i[1] in sites):
                out.append((i, u))
    return sorted(out, key=lambda p: id_key(p[0]))


# ---------------------------------------------------------- packed columns ----
@dataclass
class Packed:
    doc_offsets: np.ndarray
    id_key: np.ndarray
    cause: np.ndarray
    kind: np.ndarray
    cause_is_id: np.ndarray | None
    ref_doc: np.ndarray | None
    layout: pack.KeyLayout
    base_offsets: np.ndarray
    sel_lo: np.ndarray
    sel_hi: np.ndarray
    sel_sites: np.ndarray
    new_tx: np.ndarray
    sites: list           # rank -> site-id
    tokens: list          # token -> map key
    uuids: list           # document -> uuid
    types: list           # document -> "list" / "map"

    def args(self):
        return (self.doc_offsets, self.id_key, self.cause, self.kind, self.cause_is_id, self.ref_doc,
                self.layout, self.base_offsets, self.sel_lo, self.sel_hi, self.sel_sites, self.new_tx)


def mask_words(site_bits):
    return ((1 << site_bits) + 63) // 64


def pack_bases(bases, slices, new_tx, tx_bits=None, site_bits=None, lists_only=False, refs=True):
    """bases: [[(uuid, "list" | "map", [node, ...]), ...], ...]; slices[g] = (lo id
    or None, hi id or None, set of sites or None); new_tx[g] = (lamport-ts, site).
    One layout and one site ranking for the whole batch."""
    ids = [C.ROOT_ID]
    for b in bases:
        for _, _, nodes in b:
            for n in nodes:
                ids.append(n[0])
                if pack.valid_id(n[1]):
                    ids.append(n[1])
    for lo, hi, _ in slices:
        ids += [i for i in (lo, hi) if i is not None]
    ids += [(ts, s, 0) for ts, s in new_tx]
    sites = sorted({i[1] for i in ids}, key=pack.java_str_key)
    rank = {s: r for r, s in enumerate(sites)}
    sb = max(1, (len(sites) - 1).bit_length(), site_bits or 0)
    tb = tx_bits if tx_bits is not None else max(1, max(i[2] for i in ids).bit_length())
    lay = pack.KeyLayout(max(1, max(i[0] for i in ids).bit_length()), sb, tb)
    assert lay.key_bits <= 63
    assert all(i[2] < 1 << tb for i in ids)
    pk = lambda i: 0 if i == C.ROOT_ID else lay.pack(i[0], rank[i[1]], i[2])
    tok = {}
    off, boff = [0], [0]
    idk, ca, ci, kd, rf, uuids, types = [], [], [], [], [], [], []
    for b in bases:
        index = {u: len(uuids) + k for k, (u, _, _) in enumerate(b)}
        for u, typ, nodes in b:
            uuids.append(u)
            types.append(typ)
            for nid, cause, value in nodes:
                idk.append(pk(nid))
                k = pack.kind_of(value)
                if typ == "list":
                    if nid == C.ROOT_ID and cause is None:
                        k |= pack.KIND_ROOT
                    ca.append(pack.NIL if cause is None else pk(cause) if pack.is_id(cause) else pack.NON_ID_CAUSE)
                    ci.append(1)
                elif pack.valid_id(cause):
                    ca.append(pk(cause))
                    ci.append(1)
                elif cause is None:
                    ca.append(0)
                    ci.append(2)
                else:
                    ca.append(tok.setdefault(cause, len(tok)))
                    ci.append(0)
                kd.append(k)
                rf.append(index.get(value.name, U32_MAX) if is_ref(value) else U32_MAX)
            off.append(len(idk))
        boff.append(len(uuids))
    W = mask_words(sb)
    G = len(bases)
    lo_a, hi_a = np.zeros(G, np.uint64), np.zeros(G, np.uint64)
    masks, ntx = np.zeros(G * W, np.uint64), np.zeros(G, np.uint64)
    for g, (lo, hi, ss) in enumerate(slices):
        lo_a[g] = 0 if lo is None else pk(lo)
        hi_a[g] = (1 << 63) - 1 if hi is None else pk(hi)
        for r, s in enumerate(sites):
            if ss is None or s in ss:
                masks[g * W + r // 64] |= np.uint64(1 << (r % 64))
        if ss is None:
            masks[g * W:(g + 1) * W] = np.uint64(2 ** 64 - 1)
        ntx[g] = lay.pack(new_tx[g][0], rank[new_tx[g][1]], 0)
    return Packed(np.array(off, np.uint64), np.array(idk, np.uint64), np.array(ca, np.uint64),
                  np.array(kd, np.uint8), None if lists_only else np.array(ci, np.uint8),
                  np.array(rf, np.uint32) if refs else None, lay, np.array(boff, np.uint64), lo_a, hi_a, masks,
                  ntx, sites, list(tok), uuids, types)


@dataclass
class Parts:
    part_offsets: np.ndarray        # uint64[D+1]
    inv_id: np.ndarray              # uint64[P]
    inv_cause: np.ndarray           # uint64[P]
    inv_cause_is_id: np.ndarray | None
    inv_kind: np.ndarray            # uint8[P]
    inv_src: np.ndarray             # uint32[P]
    base_parts: np.ndarray          # uint32[G]
    status: np.ndarray              # uint32[D]


def invert_columns(doc_offsets, id_key, cause, kind, cause_is_id, ref_doc, layout, base_offsets, sel_lo,
                   sel_hi, sel_sites, new_tx) -> Parts:
    """include/causeweave_invert.h, steps 1-5 per base."""
    off = [int(x) for x in doc_offsets]
    boff = [int(x) for x in base_offsets]
    D, G = len(off) - 1, len(boff) - 1
    W = mask_words(layout.site_bits)
    smask = (1 << layout.site_bits) - 1
    per_doc = [[] for _ in range(D)]
    base_parts, status = np.zeros(G, np.uint32), np.zeros(D, np.uint32)
    idl, cal, kdl = id_key.tolist(), cause.tolist(), kind.tolist()
    cil = None if cause_is_id is None else cause_is_id.tolist()
    rfl = None if ref_doc is None else ref_doc.tolist()
    for g in range(G):
        lo, hi = int(sel_lo[g]), int(sel_hi[g])
        mask = [int(w) for w in sel_sites[g * W:(g + 1) * W]]
        selected, hidden = [], set()
        for d in range(boff[g], boff[g + 1]):
            for p in range(off[d], off[d + 1]):
                i = idl[p]
                r = (i >> layout.site_shift) & smask
                if kdl[p] & pack.KIND_ROOT or not lo <= i <= hi or not (mask[r // 64] >> (r % 64)) & 1:
                    continue
                selected.append((d, p))
                if rfl is not None and boff[g] <= rfl[p] < boff[g + 1]:
                    hidden.add(rfl[p])
        keys = {}   # (document, cause_is_id, cause) -> [oldest id, its part, newest id]
        for d, p in selected:
            if d in hidden:
                continue
            k = kdl[p] & 3
            if k == 0:
                ci, ca, ki = 1, idl[p], pack.KIND_HHIDE
            else:
                ci = 1 if cil is None else cil[p]
                ca = 0 if ci == 2 else cal[p]
                ki = pack.KIND_HHIDE if k == pack.KIND_HSHOW else pack.KIND_HSHOW
            part = (d, ci, ca, ki, p - off[d])
            e = keys.setdefault((d, ci, ca), [idl[p], part, idl[p]])
            if idl[p] < e[0]:
                e[0], e[1] = idl[p], part
            e[2] = max(e[2], idl[p])
        order = sorted(keys.values(), key=lambda e: -e[2])
        if len(order) > 1 << layout.site_shift:
            status[boff[g]:boff[g + 1]] = STATUS_KEY_RANGE
            continue
        base_parts[g] = len(order)
        for tx, (_, (d, ci, ca, ki, src), _) in enumerate(order):
            per_doc[d].append((int(new_tx[g]) + tx, ca, ci, ki, src))
    flat = [x for parts in per_doc for x in parts]
    po = np.zeros(D + 1, np.uint64)
    po[1:] = np.cumsum([len(p) for p in per_doc], dtype=np.uint64)
    col = lambda k, dt: np.array([x[k] for x in flat], dt)
    return Parts(po, col(0, np.uint64), col(1, np.uint64), None if cause_is_id is None else col(2, np.uint8),
                 col(3, np.uint8), col(4, np.uint32), base_parts, status)


_KW = {pack.KIND_HHIDE: C.H_HIDE, pack.KIND_HSHOW: C.H_SHOW}


def unpack_parts(pk: Packed, parts: Parts):
    """Per base the nodes [(uuid, node)] in tx-index order."""
    lay = pk.layout
    smask, txmask = (1 << lay.site_bits) - 1, (1 << lay.site_shift) - 1

    def unid(k):
        k = int(k)
        return C.ROOT_ID if k == 0 else (k >> lay.ts_shift, pk.sites[(k >> lay.site_shift) & smask], k & txmask)

    out = [[] for _ in range(len(pk.base_offsets) - 1)]
    for g in range(len(out)):
        nodes = []
        for d in range(int(pk.base_offsets[g]), int(pk.base_offsets[g + 1])):
            for j in range(int(parts.part_offsets[d]), int(parts.part_offsets[d + 1])):
                ci = 1 if parts.inv_cause_is_id is None else int(parts.inv_cause_is_id[j])
                cause = unid(parts.inv_cause[j]) if ci == 1 else None if ci == 2 else \
                    pk.tokens[int(parts.inv_cause[j])]
                nodes.append((pk.uuids[d], (unid(parts.inv_id[j]), cause, _KW[int(parts.inv_kind[j])])))
        out[g] = sorted(nodes, key=lambda x: x[1][0][2])
    return out


def same(a: Parts, b: Parts):
    """Every array of two results, bit for bit."""
    for f in ("part_offsets", "inv_id", "inv_cause", "inv_cause_is_id", "inv_kind", "inv_src", "base_parts",
              "status"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert x.dtype == y.dtype and np.array_equal(x, y), (f, x, y)
