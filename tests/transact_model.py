"""The rules of include/causeweave_transact.h stated twice on the CPU.

``transact_recursive`` consumes a base's tokens the way base.py:124-199 consumes
a value: a function per group that calls itself for a nested group, the tx-index
and the chain carried along.  ``transact_columns`` does what the call does:
depths from a scan, one stable sort by (base, depth, target of the part), the
groups from the ranks of openers and CLOSEs, the nodes expanded from the scanned
shares.  Both take abi_transact.transact's arguments after the Weaver and return
its TransactResult, so either stands in for the GPU (``transact_fn``).
"""
import sys

import numpy as np

from cause_amd import abi, abi_transact as A

U8, U32, U64, I64 = np.uint8, np.uint32, np.uint64, np.int64
NIL = 0xFFFFFFFFFFFFFFFF
KIND_ROOT = 4
LEAF, STR, OPEN_LIST, OPEN_MAP, CLOSE, PART, ROOT_LIST, ROOT_MAP = range(8)


class Malformed(Exception):
    pass


def _args(base_doc_offsets, doc_is_map, new_tx, tok_offsets, tok_kind, tok_arg, tok_cause, tok_cause_is_id,
          tok_vkind):
    doff, toff = np.asarray(base_doc_offsets, U64).astype(I64), np.asarray(tok_offsets, U64).astype(I64)
    T = int(toff[-1])
    vk = np.zeros(T, U8) if tok_vkind is None else np.asarray(tok_vkind, U8)
    return (doff, np.asarray(doc_is_map, U8), np.asarray(new_tx, U64), toff, np.asarray(tok_kind, U8).astype(I64),
            np.asarray(tok_arg, U32).astype(I64), np.asarray(tok_cause, U64), np.asarray(tok_cause_is_id, U8), vk)


def _result(G, D, status, news, docs, root, new_cap, nodes):
    """news[g]: [(is_map, opening token)]; docs[g]: {document: [node]}, a new
    collection's document ("n", k); node = (id, cause, cii, kind, src, sub, ref,
    run), ref None or the local number of a new collection; root[g]: local or None."""
    bn, bm = np.zeros(G + 1, U64), np.zeros(G + 1, U64)
    for g in range(G):
        bn[g + 1] = bn[g] + U64(len(news[g]))
        bm[g + 1] = bm[g] + U64(sum(len(v) for v in docs[g].values()))
    C, M = int(bn[-1]), int(bm[-1])
    per_doc = [[] for _ in range(D + C)]
    for g in range(G):
        for d, ns in docs[g].items():
            doc = D + int(bn[g]) + d[1] if isinstance(d, tuple) else d
            per_doc[doc] = [n[:6] + (A.U32_MAX if n[6] is None else D + int(bn[g]) + n[6], n[7]) for n in ns]
    no = np.zeros(D + C + 1, U64)
    no[1:] = np.cumsum([len(x) for x in per_doc], dtype=U64) if D + C else []
    flat = [n for x in per_doc for n in x]
    ncols = [np.array([n[k] for n in flat], dt) for k, (_, dt) in enumerate(A.NODE_COLUMNS)]
    flat_new = [x for g in range(G) for x in news[g]]
    ccols = [np.array([x[k] for x in flat_new], dt) for k, (_, dt) in enumerate(A.NEW_COLUMNS)]
    rd = np.array([A.U32_MAX if root[g] is None else D + int(bn[g]) + root[g] for g in range(G)], U32)
    cap = C if new_cap is None else min(C, int(new_cap))
    if not nodes:
        ncols, ccols = [None] * len(ncols), [None] * len(ccols)
    return A.TransactResult(bn, bm, no[:D + cap + 1], *ncols, *ccols, rd, np.array(status, U32))


# --------------------------------------------------------------- recursively ----
def transact_recursive(base_doc_offsets, doc_is_map, layout, new_tx, tok_offsets, tok_kind, tok_arg, tok_cause,
                       tok_cause_is_id, tok_vkind=None, new_cap=None, node_cap=None, nodes=True):
    doff, ism, ntx, toff, kind, arg, cause, cii, vk = _args(base_doc_offsets, doc_is_map, new_tx, tok_offsets, tok_kind,
                                                            tok_arg, tok_cause, tok_cause_is_id, tok_vkind)
    G, D = len(toff) - 1, int(doff[-1])
    status, news, docs, root = [], [], [], []
    for g in range(G):
        t1, tx0 = int(toff[g + 1]), int(ntx[g])
        cols, made, tx = [], {}, [0]
        last_root = [None]

        def new_node(doc, cs, ci, kd, src, sub, ref, run):     # new-node (:100-105)
            made.setdefault(doc, []).append((tx0 + tx[0], cs, ci, kd, src, sub, ref, run))
            tx[0] += 1
            return tx0 + tx[0] - 1

        def add_collection(i, is_map):                          # :117-126
            cols.append((1 if is_map else 0, i))
            doc = ("n", len(cols) - 1)
            made[doc] = [] if is_map else [(0, NIL, 1, KIND_ROOT, i, 0, None, 0)]
            return doc

        def group(i, doc, is_map, init):
            """The children from token i up to the group's CLOSE -> its position."""
            chain, run = init, 1
            while True:
                if i >= t1:
                    raise Malformed("a group still open at the end")
                k = int(kind[i])
                cs, ci = (int(cause[i]), int(cii[i])) if is_map else (None, 1)
                if k == CLOSE:
                    return i
                if k == LEAF:                                   # a scalar
                    chain = new_node(doc, chain if cs is None else cs, ci, int(vk[i]), i, 0, None, run)
                elif k == STR and is_map:                       # preserve-strings? (:134)
                    chain = new_node(doc, cs, ci, 0, i, 0, None, run)
                elif k == STR:                                  # spliced, char by char (:145-151)
                    for j in range(int(arg[i])):
                        chain = new_node(doc, chain, 1, 0, i, j, None, run)
                        run = 0
                    i += 1
                    continue
                elif k in (OPEN_LIST, OPEN_MAP):                # flatten-collection (:158-164)
                    inner = add_collection(i, k == OPEN_MAP)
                    end = group(i + 1, inner, k == OPEN_MAP, 0)
                    chain = new_node(doc, chain if cs is None else cs, ci, 0, end, 0, inner[1], run)
                    i = end
                else:
                    raise Malformed("a part inside a group, or no such kind")
                run = 0
                i += 1

        try:
            if any(int(k) > ROOT_MAP for k in kind[int(toff[g]):t1]):
                raise Malformed("no such kind")
            i = int(toff[g])
            while i < t1:
                k = int(kind[i])
                if k == PART:
                    doc = int(arg[i])
                    if not int(doff[g]) <= doc < int(doff[g + 1]):
                        raise Malformed("a target outside the base")
                    is_map = bool(ism[doc])
                elif k in (ROOT_LIST, ROOT_MAP):                # :203-208
                    doc, is_map = add_collection(i, k == ROOT_MAP), k == ROOT_MAP
                    last_root[0] = doc[1]
                else:
                    raise Malformed("outside any group")
                i = group(i + 1, doc, is_map, int(cause[i])) + 1
            st = abi.STATUS_KEY_RANGE if tx[0] > (1 << layout.site_shift) else 0
        except Malformed:
            st = A.STATUS_TX_MALFORMED
        status.append(st)
        news.append([] if st else cols)
        docs.append({} if st else {d: v for d, v in made.items() if v})
        root.append(None if st else last_root[0])
    return _result(G, D, status, news, docs, root, new_cap, nodes)


# ---------------------------------------------------------------- in columns ----
def _excl(x):
    out = np.zeros(len(x) + 1, I64)
    np.cumsum(x, out=out[1:])
    return out


def transact_columns(base_doc_offsets, doc_is_map, layout, new_tx, tok_offsets, tok_kind, tok_arg, tok_cause,
                     tok_cause_is_id, tok_vkind=None, new_cap=None, node_cap=None, nodes=True):
    doff, ism, ntx, toff, kind, arg, cause, cii, vk = _args(base_doc_offsets, doc_is_map, new_tx, tok_offsets, tok_kind,
                                                            tok_arg, tok_cause, tok_cause_is_id, tok_vkind)
    G, D, T = len(toff) - 1, int(doff[-1]), int(toff[-1])
    ntok = np.diff(toff)
    base = np.repeat(np.arange(G, dtype=I64), ntok)
    t0, d0, d1 = toff[base], doff[base], doff[base + 1]
    opener, close = np.isin(kind, (OPEN_LIST, OPEN_MAP, PART, ROOT_LIST, ROOT_MAP)), kind == CLOSE
    part, new = (kind >= PART) & (kind <= ROOT_MAP), np.isin(kind, (OPEN_LIST, OPEN_MAP, ROOT_LIST, ROOT_MAP))
    newlist = np.isin(kind, (OPEN_LIST, ROOT_LIST))
    # 1. the depth, the malformed streams
    inc = opener.astype(I64) - close
    lvl_p = _excl(inc)
    level = lvl_p[:T] - lvl_p[t0]
    bad = (kind > ROOT_MAP) | (close & (level <= 0)) | (part & (level != 0)) | ((kind <= OPEN_MAP) & (level <= 0))
    bad |= (kind == PART) & ((arg < d0) | (arg >= d1))
    last = np.zeros(T, bool)
    last[toff[1:][ntok > 0] - 1] = True
    bad |= last & (level + inc != 0)
    flag = np.zeros(G, bool)
    flag[base[bad]] = True
    nlist = np.bincount(base[newlist], minlength=G).astype(I64)
    root_tok = np.zeros(G, I64)
    isroot = (kind == ROOT_LIST) | (kind == ROOT_MAP)
    np.maximum.at(root_tok, base[isroot], np.nonzero(isroot)[0] + 1)
    # 2. the target of each token's part; the stable sort
    part_p, new_p = _excl(part), _excl(new)
    part_tok = np.concatenate([np.nonzero(part)[0], [0]])
    pidx = part_p[:T] + part
    has = pidx > part_p[t0]
    pt = part_tok[np.where(has, pidx - 1, 0)]
    tg = np.where(kind[pt] == PART, np.where((arg[pt] >= d0) & (arg[pt] < d1), arg[pt] - d0, 0),
                  (d1 - d0) + new_p[pt] - new_p[t0]) if T else np.zeros(0, I64)
    tg = np.where(has, tg, 0)
    lk = np.maximum(level, 0)
    order = np.lexsort((tg, lk, base))           # (stable)
    sk, sb, slv, s = kind[order], base[order], lk[order], np.arange(T, dtype=I64)
    st0, st1 = toff[sb], toff[sb + 1]
    change = np.ones(T + 1, bool)                # the key differs from the one before
    if T:
        change[1:T] = (sb[1:] != sb[:-1]) | (slv[1:] != slv[:-1]) | (tg[order][1:] != tg[order][:-1])
    # 3. the k-th CLOSE of a base in sorted order closes its k-th opener
    o_rank, c_rank = _excl(opener[order]), _excl(close[order])
    op = np.concatenate([order[opener[order]], [0]])
    own = np.full(T, -1, I64)
    own[op[:-1]] = np.arange(len(op) - 1)
    r = o_rank[st0] + c_rank[:T] - c_rank[st0]
    valid = (slv > 0) & (r < o_rank[st1])
    o = op[np.where(valid, r, 0)]
    ok = kind[o]
    gmap = (ok == OPEN_MAP) | (ok == ROOT_MAP) | ((ok == PART) & (arg[o] < D) & (ism[np.minimum(arg[o], max(D - 1, 0))] != 0
                                                                         if D else False))
    close_tok = np.full(T, -1, I64)
    close_tok[r[valid & (sk == CLOSE)]] = order[valid & (sk == CLOSE)]
    # 4. the counts (token order) and what a child adds to its group (sorted order)
    is_open = (sk == OPEN_LIST) | (sk == OPEN_MAP)
    scnt = np.select([sk == CLOSE, sk == LEAF, sk == STR], [(ok == OPEN_LIST) | (ok == OPEN_MAP), 1,
                                                             np.where(gmap, 1, arg[order])], 0) * valid
    e = np.select([sk == LEAF, sk == STR, is_open], [1, np.where(gmap, 1, arg[order]), 1], 0) * valid
    cnt = np.zeros(T, I64)
    cnt[order] = scnt
    gr = np.full(T, -1, I64)
    gr[order] = np.where(valid, r, -1)
    cnt_p = _excl(cnt)
    tot = cnt_p[toff[1:]] - cnt_p[toff[:-1]]
    status = np.where(flag, A.STATUS_TX_MALFORMED, np.where(tot > (1 << layout.site_shift), abi.STATUS_KEY_RANGE, 0))
    good = status == 0
    bnew = _excl(np.where(good, new_p[toff[1:]] - new_p[toff[:-1]], 0))
    bnode = _excl(np.where(good, tot + nlist, 0))
    C, M = int(bnew[-1]), int(bnode[-1])
    root_doc = np.where(good & (root_tok > 0), D + bnew[:-1] + new_p[np.maximum(root_tok - 1, 0)] - new_p[toff[:-1]],
                        A.U32_MAX)
    # 5. the virtual nodes; the marks of the groups and documents
    live = good[sb] if T else np.zeros(0, bool)
    e = e * live
    W = _excl(e)
    in_grp = live & valid
    head = in_grp & (change[:T] | np.concatenate([[False], sk[:-1] == CLOSE]))
    w_start, w_close = np.zeros(T + 1, I64), np.zeros(T + 1, I64)
    w_start[r[head]] = W[:T][head]
    w_close[r[in_grp & (sk == CLOSE)]] = W[:T][in_grp & (sk == CLOSE)]
    doc_w0, doc_w1 = np.zeros(D, I64), np.zeros(D, I64)
    to_doc = in_grp & (ok == PART)
    m = to_doc & change[:T]
    doc_w0[arg[o][m]] = W[:T][m]
    m = to_doc & ((s + 1 == st1) | change[1:])
    doc_w1[arg[o][m]] = (W[:T] + e)[m]
    new_tok = np.zeros(C, I64)
    m = live & new[order]
    new_tok[(bnew[sb] + new_p[order] - new_p[st0])[m]] = order[m]
    counts = np.concatenate([doc_w1 - doc_w0, w_close[own[new_tok]] - w_start[own[new_tok]] + newlist[new_tok]])
    noff = _excl(counts)
    assert int(noff[-1]) == M, (int(noff[-1]), M)
    cap = C if new_cap is None else min(C, int(new_cap))
    res = dict(base_new_offsets=bnew.astype(U64), base_node_offsets=bnode.astype(U64),
               node_offsets=noff[:D + cap + 1].astype(U64), root_doc=root_doc.astype(U32),
               base_status=status.astype(U32))
    if not nodes:
        return A.TransactResult(**res, **{f: None for f, _ in A.NODE_COLUMNS + A.NEW_COLUMNS})
    # 6. every node from its virtual number
    kids = np.nonzero(e)[0]
    sv = np.repeat(kids, e[kids])                # the child that makes virtual node v
    V = len(sv)
    v = np.arange(V, dtype=I64)
    i, j, g = order[sv], v - W[sv], sb[sv]
    rr, oo = r[sv], o[sv]
    kd, okd, q, b0 = kind[i], kind[oo], v - w_start[rr], toff[g]
    to_part = okd == PART
    c_grp = bnew[g] + new_p[oo] - new_p[b0]
    g_map = np.where(to_part, ism[np.where(to_part, arg[oo], 0)] != 0 if D else False,
                     (okd == OPEN_MAP) | (okd == ROOT_MAP))
    pos = np.where(to_part, noff[np.where(to_part, arg[oo], 0)] + v - (doc_w0[np.where(to_part, arg[oo], 0)] if D else 0),
                   noff[D + np.where(to_part, 0, c_grp)] + (~g_map) + q)
    is_ref = (kd == OPEN_LIST) | (kd == OPEN_MAP)
    mk = np.where(is_ref, close_tok[own[i]], i)
    txi = np.where(is_ref, cnt_p[mk] - cnt_p[b0], cnt_p[i] - cnt_p[b0] + j)
    ref = np.where(is_ref, D + bnew[g] + new_p[i] - new_p[b0], A.U32_MAX)
    tx0 = ntx[g]
    nid = tx0 + txi.astype(U64)
    # the last node of the child before: virtual node v - 1
    s2 = sv[np.maximum(v - 1, 0)]
    i2 = order[s2]
    ref2 = (kind[i2] == OPEN_LIST) | (kind[i2] == OPEN_MAP)
    last2 = np.where(ref2, cnt_p[close_tok[own[i2]]] - cnt_p[b0], cnt_p[i2] - cnt_p[b0] + e[s2] - 1)
    init = np.where(okd == OPEN_LIST, U64(0), cause[oo])
    ca = np.where(g_map, cause[i], np.where(q == 0, init, np.where(j > 0, nid - U64(1), tx0 + last2.astype(U64))))
    ci = np.where(g_map, cii[i], 1)
    cols = {"node_id": np.zeros(M, U64), "node_cause": np.zeros(M, U64), "node_cause_is_id": np.zeros(M, U8),
            "node_kind": np.zeros(M, U8), "node_src": np.zeros(M, U32), "node_sub": np.zeros(M, U32),
            "node_ref": np.zeros(M, U32), "node_run": np.zeros(M, U8)}
    for f, x in (("node_id", nid), ("node_cause", ca), ("node_cause_is_id", ci), ("node_kind", np.where(kd == LEAF, vk[i], 0)),
                 ("node_src", mk), ("node_sub", np.where(kd == STR, j, 0)), ("node_ref", ref), ("node_run", q == 0)):
        cols[f][pos] = x
    # the new collections and the roots of the lists
    lists = np.nonzero(newlist[new_tok])[0]
    p = noff[D + lists]
    cols["node_id"][p], cols["node_cause"][p], cols["node_cause_is_id"][p] = 0, NIL, 1
    cols["node_kind"][p], cols["node_src"][p], cols["node_sub"][p] = KIND_ROOT, new_tok[lists], 0
    cols["node_ref"][p], cols["node_run"][p] = A.U32_MAX, 0
    return A.TransactResult(**res, **cols, new_is_map=(~newlist[new_tok]).astype(U8), new_open=new_tok.astype(U32))


def same(x, y):
    """Two TransactResults, array by array, bit for bit (a list of differences)."""
    out = []
    for f in A.TransactResult.__dataclass_fields__:
        p, q = getattr(x, f), getattr(y, f)
        if (p is None) != (q is None):
            out.append(f"{f}: one is None")
        elif p is not None and (p.dtype != q.dtype or p.shape != q.shape or not np.array_equal(p, q)):
            out.append(f"{f}: {p[:12]} ({p.dtype}{p.shape}) != {q[:12]} ({q.dtype}{q.shape})")
    return out


# ------------------------------------------------------------------ streams ----
def random_stream(rng, n_docs, doc0, is_map, budget=40, depth=5, p_bad=0.0):
    """One base's tokens: parts into its documents [doc0, doc0 + n_docs) and new
    roots, nested up to `depth`, about `budget` tokens -> [(kind, arg, cause, cii, vkind)]."""
    toks = []

    def cause_of(in_map):
        if not in_map:
            return 0, 1
        c = rng.randrange(3)
        return (rng.randrange(1, 50), 0) if c == 0 else (rng.randrange(1, 1 << 20), 1) if c == 1 else (0, 2)

    def contents(in_map, left, d):
        for _ in range(rng.randrange(0, 5)):
            if left[0] <= 0:
                break
            left[0] -= 1
            c = rng.random()
            ca, ci = cause_of(in_map)
            if c < 0.45:
                toks.append((LEAF, 0, ca, ci, rng.choice((0, 0, 0, 1, 2, 3))))
            elif c < 0.65:
                toks.append((STR, rng.choice((0, 1, 2, 5)), ca, ci, 0))
            elif d < depth:
                m = rng.random() < 0.5
                toks.append((OPEN_MAP if m else OPEN_LIST, 0, ca, ci, 0))
                contents(m, left, d + 1)
                toks.append((CLOSE, 0, 0, 0, 0))

    left = [budget]
    for _ in range(rng.randrange(0, 4)):
        if n_docs and rng.random() < 0.7:
            d = doc0 + rng.randrange(n_docs)
            m = bool(is_map[d])
            toks.append((PART, d, 0 if m else rng.choice((0, NIL, rng.randrange(1, 1 << 20))), 1, 0))
        else:
            m = rng.random() < 0.5
            toks.append((ROOT_MAP if m else ROOT_LIST, 0, 0 if m else rng.choice((0, NIL)), 1, 0))
        contents(m, left, 1)
        toks.append((CLOSE, 0, 0, 0, 0))
    if toks and rng.random() < p_bad:
        k = rng.randrange(len(toks))
        c = rng.randrange(6)
        if c == 0:
            del toks[k]
        elif c == 1:
            toks.insert(k, (CLOSE, 0, 0, 0, 0))
        elif c == 2:
            toks.insert(k, (rng.choice((PART, ROOT_LIST, OPEN_MAP, LEAF, STR)), doc0, 0, 1, 0))
        elif c == 3:
            toks[k] = (rng.choice((8, 9, 200, 255)),) + toks[k][1:]
        elif c == 4:
            toks[k] = (toks[k][0], doc0 + n_docs + rng.randrange(3)) + toks[k][2:]
        else:
            toks = toks[:k]
    return toks


def random_batch(rng, n_bases, budget=40, depth=5, p_bad=0.0, site_shift=12):
    """-> transact's arguments after the Weaver (a dict)."""
    from cause_amd import pack
    doff, toff, ism, toks = [0], [0], [], []
    for _ in range(n_bases):
        n = rng.randrange(0, 4)
        ism += [rng.randrange(2) for _ in range(n)]
        toks += random_stream(rng, n, doff[-1], ism, budget, depth, p_bad)
        doff.append(doff[-1] + n)
        toff.append(len(toks))
    lay = pack.KeyLayout(20, 4, site_shift)
    ntx = np.array([lay.pack(rng.randrange(1, 1000), rng.randrange(16), 0) for _ in range(n_bases)], U64)
    col = lambda k, dt: np.array([t[k] for t in toks], dt)
    return dict(base_doc_offsets=np.array(doff, U64), doc_is_map=np.array(ism, U8), layout=lay, new_tx=ntx,
                tok_offsets=np.array(toff, U64), tok_kind=col(0, U8), tok_arg=col(1, U32), tok_cause=col(2, U64),
                tok_cause_is_id=col(3, U8), tok_vkind=col(4, U8))
