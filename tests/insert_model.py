"""numpy / Python statement of cw_insert_lists (include/causeweave_insert.h).

``insert_lists`` takes the arrays of a cw_insert_batch and returns every array
of a cw_insert_result: the formula of the header (weave-node as two
min-reductions), s/insert's validations on the first tx node, the index
convention (s < n_d old, s >= n_d tx node s - n_d), the rendered bits and
counts, max_ts, the yarns and the compacted offsets.  It never looks at the
library; tests/test_insert_model.py holds it against oracle.causal_ref step by
step, and the GPU tests hold the library against it.

``batch_of`` builds the arrays from reference cts (dicts of oracle.causal_ref)
and their transactions; ``apply_result`` turns a result back into cts.
"""
from __future__ import annotations

from bisect import bisect_left
from types import SimpleNamespace as NS

import numpy as np

from cause_amd import pack
from oracle import causal_ref as R

NIL = np.uint64((1 << 64) - 1)
NONE = 0xFFFFFFFF
STATUS_DUP, STATUS_ORPHAN = 2, 4
KIND_ROOT = 4

U8, U32, U64 = np.uint8, np.uint32, np.uint64


def special(kind):
    return (kind & 3) != 0


def is_hide(kind):
    return (kind & 3 == 1) | (kind & 3 == 2)


def place(wid, wca, wkd, nid, nca, nkd):
    """(a, p) of the header's formula for a weave given as id / cause / kind
    arrays in weave order and the node (nid, nca, nkd); a is None when the
    cause is no node of the weave (s/insert refuses it, shared.cljc:175-178,
    even where an orphan of the weave names nid and so gives an asap position)."""
    n = len(wid)
    sr, sm = special(wkd), bool(special(nkd))
    lt = nid < wid
    later = (sr & (nid != wca) & ((not sm) | lt)) | (lt & ((not sm) | sr))
    if not (wid == nca).any():
        return None, n
    cand = np.concatenate([np.flatnonzero(wid == nca) + 1, np.flatnonzero(wca == nid)])
    a = int(cand.min())
    stop = np.flatnonzero(~later[a:])
    return a, (a + int(stop[0]) if len(stop) else n)


def hidden(nid, nkd, xca, xkd):
    """hide? (list.cljc:48-55) of a node given the node after it (xkd None: the last)."""
    if special(nkd) or nkd & KIND_ROOT:
        return True
    return xkd is not None and bool(is_hide(xkd)) and nid == xca


def insert_lists(off, idk, ck, kd, perm, bits, toff, tid, tca, tkd, ts_shift, site_shift=0,
                 site_bits=0, yarn=None, val=None, tval=None):
    """Every array of a cw_insert_result, as a namespace (yarn_perm / value None
    when their inputs are)."""
    off, toff = np.asarray(off, np.int64), np.asarray(toff, np.int64)
    D = len(off) - 1
    vis_old = np.unpackbits(np.ascontiguousarray(bits, U32).view(U8), bitorder="little")
    new_off = np.zeros(D + 1, U64)
    pos = np.full(D, NONE, U32)
    status, count, max_ts = np.zeros(D, U32), np.zeros(D, U32), np.zeros(D, U64)
    o_perm, o_vis, o_yarn = [], [], []
    o_id, o_ca, o_kd, o_val = [], [], [], []
    smask = (1 << site_bits) - 1
    ykey = lambda i: ((int(i) >> site_shift) & smask, int(i))
    for d in range(D):
        o, n = int(off[d]), int(off[d + 1] - off[d])
        t0, k = int(toff[d]), int(toff[d + 1] - toff[d])
        did, dca, dkd = idk[o:o + n], ck[o:o + n], kd[o:o + n]
        w = np.asarray(perm[o:o + n], np.int64)
        vis = vis_old[o:o + n].astype(bool)
        p = None
        if k:
            hit = np.flatnonzero(did == tid[t0])
            if len(hit):
                same = (dca[hit] == tca[t0]) & (dkd[hit] == tkd[t0])
                if val is not None:
                    same &= val[o:o + n][hit] == tval[t0]
                if not same.any():
                    status[d] = STATUS_DUP
            else:
                a, pp = place(did[w], dca[w], dkd[w], tid[t0], tca[t0], tkd[t0])
                if a is None:
                    status[d] = STATUS_ORPHAN
                else:
                    p = pp
        kk = k if p is not None else 0
        nid = np.concatenate([did, tid[t0:t0 + kk]])
        nca = np.concatenate([dca, tca[t0:t0 + kk]])
        nkd = np.concatenate([dkd, tkd[t0:t0 + kk]])
        if p is not None:
            pos[d] = p
            w = np.concatenate([w[:p], n + np.arange(k), w[p:]])
            vis = np.concatenate([vis[:p], np.zeros(k, bool), vis[p:]])
            for j in range(max(p - 1, 0), p + k):
                s, x = w[j], (w[j + 1] if j + 1 < n + k else None)
                vis[j] = not hidden(nid[s], nkd[s], None if x is None else nca[x],
                                    None if x is None else nkd[x])
        new_off[d + 1] = new_off[d] + U64(n + kk)
        count[d] = int(vis.sum())
        max_ts[d] = (int(nid.max()) >> ts_shift) if len(nid) else 0
        o_perm.append(w.astype(U32))
        o_vis.append(vis)
        o_id.append(nid), o_ca.append(nca), o_kd.append(nkd)
        if val is not None:
            o_val.append(np.concatenate([val[o:o + n], tval[t0:t0 + kk]]))
        if yarn is not None:
            y = np.asarray(yarn[o:o + n], np.int64)
            keys = [ykey(did[e]) for e in y]
            out = np.full(n + kk, -1, np.int64)
            for m in range(kk):  # tx node m behind the old entries below it
                out[bisect_left(keys, ykey(tid[t0 + m])) + m] = n + m
            out[out < 0] = y
            o_yarn.append(out.astype(U32))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    M = int(new_off[-1])
    v = np.zeros((M + 31) // 32 * 32, U8)
    v[:M] = cat(o_vis, U8)
    return NS(new_offsets=new_off, insert_pos=pos, weave_perm=cat(o_perm, U32),
              visible_bits=np.packbits(v, bitorder="little").view(U32), visible=v[:M],
              visible_count=count, max_ts=max_ts, status=status,
              yarn_perm=None if yarn is None else cat(o_yarn, U32),
              id_key=cat(o_id, U64), cause_key=cat(o_ca, U64), kind=cat(o_kd, U8),
              value=None if val is None else cat(o_val, U64))


# --------------------------------------------------------------- reference cts
def batch_of(items, tokens=None):
    """The arrays of a cw_insert_batch from [(ct, tx nodes)] -- cts of
    oracle.causal_ref with their ::weave and ::yarns as they stand.  Each
    document is packed with its tx (one site ranking for both).  Returns a
    namespace: the arrays, the layout, and per document its nodes in input order
    (old, then tx)."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct, _ in items]
    pk = pack.pack_lists([d + list(tx) for d, (_, tx) in zip(docs, items)], min_site_bits=1)
    lay = pk.layout
    tok = tokens or (lambda v: hash(repr(v)) & ((1 << 62) - 1))
    sel, tsel, off, toff = [], [], [0], [0]
    perm, vis, yarn = [], [], []
    for d, ((ct, tx), nodes) in enumerate(zip(items, docs)):
        lo, n = int(pk.offsets[d]), len(nodes)
        sel.append(np.arange(lo, lo + n))
        tsel.append(np.arange(lo + n, lo + n + len(tx)))
        off.append(off[-1] + n)
        toff.append(toff[-1] + len(tx))
        at = {nd[0]: s for s, nd in enumerate(nodes)}
        w = ct["weave"]
        perm += [at[nd[0]] for nd in w]
        vis += [not R.hide_q(nd, w[j + 1] if j + 1 < len(w) else None) for j, nd in enumerate(w)]
        for site in sorted(ct["yarns"], key=R.java_str_key):
            yarn += [at[nd[0]] for nd in ct["yarns"][site]]
    sel = np.concatenate(sel) if sel else np.zeros(0, np.int64)
    tsel = np.concatenate(tsel) if tsel else np.zeros(0, np.int64)
    N = len(sel)
    v = np.zeros((N + 31) // 32 * 32, U8)
    v[:N] = vis
    vals = np.array([tok(nd[2]) for pd in pk.docs for nd in pd.nodes], U64)
    return NS(off=np.array(off, U64), toff=np.array(toff, U64), idk=pk.id_key[sel],
              ck=pk.cause_key[sel], kd=pk.kind[sel], val=vals[sel],
              perm=np.array(perm, U32), bits=np.packbits(v, bitorder="little").view(U32),
              yarn=np.array(yarn, U32), tid=pk.id_key[tsel], tca=pk.cause_key[tsel],
              tkd=pk.kind[tsel], tval=vals[tsel], layout=lay,
              nodes=[d + list(tx) for d, (_, tx) in zip(docs, items)])


def run(b, values=True):
    """insert_lists on a batch_of namespace."""
    return insert_lists(b.off, b.idk, b.ck, b.kd, b.perm, b.bits, b.toff, b.tid, b.tca, b.tkd,
                        b.layout.ts_shift, b.layout.site_shift, b.layout.site_bits, b.yarn,
                        b.val if values else None, b.tval if values else None)


def doc_view(b, res, d):
    """Document d of a result as reference values: (weave nodes, rendered flags,
    yarns {site: nodes}, max_ts)."""
    lo, hi = int(res.new_offsets[d]), int(res.new_offsets[d + 1])
    nodes = b.nodes[d]
    weave = [nodes[s] for s in res.weave_perm[lo:hi]]
    yarns = {}
    for s in res.yarn_perm[lo:hi]:
        yarns.setdefault(nodes[s][0][1], []).append(nodes[s])
    return weave, [bool(x) for x in res.visible[lo:hi]], yarns, int(res.max_ts[d])
