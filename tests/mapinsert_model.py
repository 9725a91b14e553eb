"""numpy / Python statement of cw_insert_maps (include/causeweave_map_insert.h).

``insert_maps`` takes the arrays of a cw_map_insert_batch and returns every
array of a cw_map_insert_result: s/insert's validations on the first tx node,
the key word and cause-in-weave of every tx node, the header's formula run on
one key weave per tx node in order, active-node of the touched key weaves, the
index convention (s < n_d old, s >= n_d tx node s - n_d) and the compacted
offsets.  It never looks at the library; tests/test_mapinsert_model.py holds it
against oracle.causal_ref step by step, and the GPU tests hold the library
against it.

``batch_of`` builds the arrays from reference map cts (dicts of
oracle.causal_ref) and their transactions; ``doc_view`` turns a result back
into a ct's ``nodes`` / ``weave`` / active nodes.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

from cause_amd import pack
from oracle import causal_ref as R

NIL = (1 << 64) - 1
ID_KEY = 1 << 63
NONE = 0xFFFFFFFF
STATUS_DUP, STATUS_ORPHAN, STATUS_MAP_KEY = 2, 4, 16

U8, U32, U64, I64 = np.uint8, np.uint32, np.uint64, np.int64


def special(kind):
    return (kind & 3) != 0


def is_hide(kind):
    return (kind & 3) in (1, 2)


def place(wid, wciw, wkd, nid, nciw, nkd):
    """p of the header's formula: the key weave as lists of ids, causes-in-weave
    (None for the root) and kinds, root first; nm = (nid, nciw, nkd)."""
    n = len(wid)
    sm = special(nkd)
    cand = [i + 1 for i in range(n) if wid[i] == nciw] + [i for i in range(n) if wciw[i] == nid]
    if not cand:
        return n
    for i in range(min(cand), n):
        sr, lt = special(wkd[i]), nid < wid[i]
        later = (sr and nid != wciw[i] and (not sm or lt)) or (lt and (not sm or sr))
        if not later:
            return i
    return n


def active(kinds):
    """active-node (map.cljc:47-59) of a key weave given its kinds, root first:
    the position, or -1 for blank."""
    if len(kinds) > 1 and is_hide(kinds[1]):
        return -1
    for i in range(1, len(kinds)):
        if special(kinds[i]):
            continue
        if i + 1 < len(kinds) and is_hide(kinds[i + 1]):
            continue
        return i
    return -1


def insert_maps(off, idk, ca, ci, kd, seg_off, seg_coll, seg_key, seg_active, seg_perm, toff, tid, tca,
                tci, tkd, val=None, tval=None):
    """Every array of a cw_map_insert_result, as a namespace."""
    off, toff = [int(x) for x in off], [int(x) for x in toff]
    D = len(off) - 1
    segs_of = [[] for _ in range(D)]
    for s, d in enumerate(np.asarray(seg_coll).tolist()):
        segs_of[d].append(s)
    new_off, status = [0], np.zeros(D, U32)
    T = toff[-1]
    tx_seg, tx_pos = np.full(T, NONE, U32), np.full(T, NONE, U32)
    o_so, o_sc, o_sk, o_sa, o_sp = [], [], [], [], []
    o_id, o_ca, o_ci, o_kd, o_val = [], [], [], [], []
    for d in range(D):
        o, n, t0, k = off[d], off[d + 1] - off[d], toff[d], toff[d + 1] - toff[d]
        did, dca = [int(x) for x in idk[o:o + n]], [int(x) for x in ca[o:o + n]]
        dci, dkd = [int(x) for x in ci[o:o + n]], [int(x) for x in kd[o:o + n]]
        xid, xca = [int(x) for x in tid[t0:t0 + k]], [int(x) for x in tca[t0:t0 + k]]
        xci, xkd = [int(x) for x in tci[t0:t0 + k]], [int(x) for x in tkd[t0:t0 + k]]
        weaves, act = {}, {}
        for s in segs_of[d]:
            lo, hi = int(seg_off[s]), int(seg_off[s + 1])
            weaves[int(seg_key[s])] = [int(x) for x in seg_perm[lo + 1:hi]]
            act[int(seg_key[s])] = int(seg_active[s])
        accept = k > 0
        if k:
            if xid[0] in did:
                accept = False
                s = did.index(xid[0])
                same = dci[s] == xci[0] and dkd[s] == xkd[0] and (xci[0] == 2 or dca[s] == xca[0])
                if val is not None and int(val[o + s]) != int(tval[t0]):
                    same = False
                if not same:
                    status[d] = STATUS_DUP
            elif xci[0] == 2 or (xci[0] == 1 and xca[0] not in did):
                accept, status[d] = False, STATUS_ORPHAN
            elif any(c == 0 and x >= 1 << 62 for c, x in zip(xci, xca)):
                accept, status[d] = False, STATUS_MAP_KEY
        kk = k if accept else 0
        aid, aca, aci, akd = did + xid[:kk], dca + xca[:kk], dci + xci[:kk], dkd + xkd[:kk]
        at = {}
        for s in range(n + kk - 1, -1, -1):  # (old nodes win, then the first tx node of an id)
            at[aid[s]] = s
        ciw = lambda s: aca[s] if aci[s] == 1 else 0
        touched, where = set(), {}
        for j in range(kk):
            s = n + j
            if aci[s] == 0:
                key = aca[s]
            elif aci[s] == 2 or aca[s] not in at:
                key = NIL
            else:
                c = at[aca[s]]
                key = aca[c] if aci[c] == 0 else (ID_KEY | aca[c]) if aci[c] == 1 else NIL
            w = weaves.setdefault(key, [])
            p = place([0] + [aid[x] for x in w], [None] + [ciw(x) for x in w], [4] + [akd[x] for x in w],
                      aid[s], ciw(s), akd[s])
            w.insert(p - 1, s)
            touched.add(key)
            where[j] = key
        S0 = len(o_sk)
        for key in sorted(weaves):
            w = weaves[key]
            if key in touched:
                a = active([4] + [akd[x] for x in w])
                act[key] = -1 if a < 0 else w[a - 1]
            o_so.append(len(o_sp))
            o_sc.append(d)
            o_sk.append(key)
            o_sa.append(act[key])
            o_sp += [NONE] + w
        keys = sorted(weaves)
        for j in range(kk):
            tx_seg[t0 + j] = S0 + keys.index(where[j])
            tx_pos[t0 + j] = weaves[where[j]].index(n + j) + 1
        new_off.append(new_off[-1] + n + kk)
        o_id += aid
        o_ca += aca
        o_ci += aci
        o_kd += akd
        if val is not None:
            o_val += [int(x) for x in val[o:o + n]] + [int(x) for x in tval[t0:t0 + kk]]
    o_so.append(len(o_sp))
    return NS(new_offsets=np.array(new_off, U64), tx_seg=tx_seg, tx_pos=tx_pos, n_segs=len(o_sk),
              seg_offsets=np.array(o_so, U64), seg_coll=np.array(o_sc, U32), seg_key=np.array(o_sk, U64),
              seg_active=np.array(o_sa, I64), seg_perm=np.array(o_sp, U32), status=status,
              id_key=np.array(o_id, U64), cause=np.array(o_ca, U64), cause_is_id=np.array(o_ci, U8),
              kind=np.array(o_kd, U8), value=None if val is None else np.array(o_val, U64))


ARRAYS = ("new_offsets", "tx_seg", "tx_pos", "seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm",
          "status", "id_key", "cause", "cause_is_id", "kind", "value")


def weave_maps(off, idk, ca, ci, kd):
    """The cw_map_result of collections given as columns, by inserting every
    node as a tx of its own in the given order into empty collections -- the
    model's own full weave (collections whose nodes arrive in id order: the
    reference's fold)."""
    D = len(off) - 1
    z64, z8 = np.zeros(0, U64), np.zeros(0, U8)
    segs = NS(seg_offsets=np.zeros(1, U64), seg_coll=np.zeros(0, U32), seg_key=z64,
              seg_active=np.zeros(0, I64), seg_perm=np.zeros(0, U32))
    cur = NS(off=np.zeros(D + 1, U64), idk=z64, ca=z64, ci=z8, kd=z8)
    most = max([int(off[d + 1] - off[d]) for d in range(D)] + [0])
    for step in range(most):
        pick = [int(off[d]) + step for d in range(D) if step < int(off[d + 1] - off[d])]
        toff = np.cumsum([0] + [int(step < int(off[d + 1] - off[d])) for d in range(D)]).astype(U64)
        r = insert_maps(cur.off, cur.idk, cur.ca, cur.ci, cur.kd, segs.seg_offsets, segs.seg_coll,
                        segs.seg_key, segs.seg_active, segs.seg_perm, toff, idk[pick], ca[pick], ci[pick],
                        kd[pick])
        assert not r.status.any()
        cur = NS(off=r.new_offsets, idk=r.id_key, ca=r.cause, ci=r.cause_is_id, kd=r.kind)
        segs = r
    return segs


# --------------------------------------------------------------- reference cts
def batch_of(items, tokens=None):
    """The arrays of a cw_map_insert_batch from [(map ct, tx nodes)] -- cts of
    oracle.causal_ref with their ::weave as it stands.  Each collection is
    packed with its tx (one site ranking, one key-token table).  Returns a
    namespace: the arrays, and per collection its nodes in input order (old,
    then tx), the packing and the key of each old key weave."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct, _ in items]
    pm = pack.pack_maps([d + list(tx) for d, (_, tx) in zip(docs, items)])
    tok = tokens or (lambda v: hash(repr(v)) & ((1 << 62) - 1))
    ktok = {k: t for t, k in enumerate(pm.keys)}
    sel, tsel, off, toff = [], [], [0], [0]
    so, sc, sk, sa, sp = [0], [], [], [], []
    for d, ((ct, tx), nodes) in enumerate(zip(items, docs)):
        lo, n = int(pm.offsets[d]), len(nodes)
        sel += range(lo, lo + n)
        tsel += range(lo + n, lo + n + len(tx))
        off.append(off[-1] + n)
        toff.append(toff[-1] + len(tx))
        at = {nd[0]: s for s, nd in enumerate(nodes)}
        rank = pm.ranks[d]
        words = {}
        for key in ct["weave"]:
            if key is None:
                words[NIL] = key
            elif pack.valid_id(key):
                words[ID_KEY | (0 if key == R.ROOT_ID else pm.layout.pack(key[0], rank[key[1]], key[2]))] = key
            else:
                words[ktok[key]] = key
        for word in sorted(words):
            w = ct["weave"][words[word]]
            a = R.active_node(words[word], w)
            sc.append(d)
            sk.append(word)
            sa.append(-1 if a is R.BLANK else at[a[0]])
            sp += [NONE] + [at[nd[0]] for nd in w[1:]]
            so.append(len(sp))
    sel, tsel = np.array(sel, np.int64), np.array(tsel, np.int64)
    vals = np.array([tok(nd[2]) for pd in pm.docs for nd in pd], U64)
    return NS(off=np.array(off, U64), toff=np.array(toff, U64), idk=pm.id_key[sel], ca=pm.cause[sel],
              ci=pm.cause_is_id[sel], kd=pm.kind[sel], val=vals[sel], seg_off=np.array(so, U64),
              seg_coll=np.array(sc, U32), seg_key=np.array(sk, U64), seg_active=np.array(sa, I64),
              seg_perm=np.array(sp, U32), tid=pm.id_key[tsel], tca=pm.cause[tsel], tci=pm.cause_is_id[tsel],
              tkd=pm.kind[tsel], tval=vals[tsel], pm=pm,
              nodes=[d + list(tx) for d, (_, tx) in zip(docs, items)])


def run(b, values=True):
    """insert_maps on a batch_of namespace."""
    return insert_maps(b.off, b.idk, b.ca, b.ci, b.kd, b.seg_off, b.seg_coll, b.seg_key, b.seg_active,
                       b.seg_perm, b.toff, b.tid, b.tca, b.tci, b.tkd, b.val if values else None,
                       b.tval if values else None)


def key_of(b, d, word):
    """The map key a seg_key word of collection d stands for."""
    if word == NIL:
        return None
    if word >> 63:
        w = word & (ID_KEY - 1)
        if w == 0:
            return R.ROOT_ID
        lay, rank = b.pm.layout, b.pm.ranks[d]
        site = {r: s for s, r in rank.items()}
        return (w >> lay.ts_shift, site[(w >> lay.site_shift) & ((1 << lay.site_bits) - 1)],
                w & ((1 << lay.tx_bits) - 1) if lay.tx_bits else 0)
    return b.pm.keys[word]


def doc_view(b, res, d):
    """Collection d of a result as reference values: (nodes {id: body}, weave
    {key: key weave}, {key: active node or BLANK})."""
    lo, hi = int(res.new_offsets[d]), int(res.new_offsets[d + 1])
    nodes = b.nodes[d][:hi - lo]
    weave, act = {}, {}
    for s in np.flatnonzero(np.asarray(res.seg_coll) == d).tolist():
        key = key_of(b, d, int(res.seg_key[s]))
        run_ = res.seg_perm[int(res.seg_offsets[s]):int(res.seg_offsets[s + 1])].tolist()
        assert run_[0] == NONE
        weave[key] = [R.ROOT_NODE] + [
            (nodes[p][0], nodes[p][1] if pack.valid_id(nodes[p][1]) else R.ROOT_ID, nodes[p][2])
            for p in run_[1:]]
        a = int(res.seg_active[s])
        act[key] = R.BLANK if a < 0 else (nodes[a][0], key, nodes[a][2])
    return {nd[0]: (nd[1], nd[2]) for nd in nodes}, weave, act
