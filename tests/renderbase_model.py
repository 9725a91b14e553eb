"""CPU model of cw_render_bases (include/causeweave_render_bases.h), twice:

``render_recursive``  the contract as the header states it: claims, then
                      go(root, UINT32_MAX) per base with an explicit stack.
``render_columns``    the path renderbase.hip takes, in numpy columns: claims,
                      the tree refs compacted in entry order, the two events of
                      every document with successor and weight, pointer jumping
                      for ceil(log2(2 * n_docs)) rounds, sizes and starts from
                      the distances, flags, the scan of the base sizes, and
                      every token's position computed on its own.

Both return an abi_render_bases.RenderBasesResult; ``same`` compares two of
them (doc_open only where doc_base names a base: it is unspecified elsewhere).
"""
import numpy as np

from cause_amd.abi_render_bases import (RenderBasesResult, STATUS_REF_SHARED, TOK_CLOSE, TOK_LEAF, TOK_NIL,
                                        TOK_OPEN, U32_MAX)

U8, U32, U64, I64 = np.uint8, np.uint32, np.uint64, np.int64
NONE = U32_MAX
SHARED = STATUS_REF_SHARED
# (ent_offsets, ent_ref, root_doc, base_status): every way a collection is claimed twice, and a cycle nobody reaches
SHARED_CASES = [
    ([0, 2, 3], [1, 1, NONE], [0], [SHARED]),                      # referred to twice in one base
    ([0, 1, 2, 3], [2, 2, NONE], [0, 1], [SHARED] * 2),            # ... from two bases
    ([0, 1, 2, 3], [1, NONE, 1], [0], [SHARED]),                   # ... and from an unreachable document
    ([0, 1, 2], [1, 0], [0], [SHARED]),                            # a root referred to by its descendant
    ([0, 1], [NONE], [0, 0], [SHARED] * 2),                        # two bases with one root
    ([0, 1, 2, 3], [NONE, 2, 1], [0], [0]),                        # an isolated cycle nobody reaches
    ([0, 1, 2, 3], [NONE, 0, NONE], [0, 2], [SHARED, 0]),          # a root referred to from outside
]


def _inputs(ent_offsets, ent_ref, root_doc):
    off = np.asarray(ent_offsets, I64)
    ref = np.asarray(ent_ref, U32).astype(I64)
    root = np.asarray(root_doc, U32).astype(I64)
    assert len(off) >= 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(ref)
    return off, ref, root, len(off) - 1, len(root), len(ref)


def claims_of(off, ref, root, D):
    """claims[d]: the entries that refer to d plus the bases rooted at d."""
    return np.bincount(ref[ref < D], minlength=D)[:D] + np.bincount(root[root < D], minlength=D)[:D]


def render_recursive(ent_offsets, ent_ref, root_doc) -> RenderBasesResult:
    off, ref, root, D, G, E = _inputs(ent_offsets, ent_ref, root_doc)
    claims = claims_of(off, ref, root, D)
    kind, doc, ent = [], [], []
    bo, status = [0], []
    doc_base, doc_open = np.full(D, NONE, U32), np.full(D, NONE, U32)
    for g in range(G):
        r = int(root[g])
        if r >= D:
            status.append(0)
            bo.append(bo[-1])
            continue
        toks, reached = [], []
        flagged = claims[r] >= 2
        stack = [] if flagged else [(r, NONE, int(off[r]))]
        if stack:
            toks.append((TOK_OPEN, r, NONE))
            reached.append((r, 0))
        while stack and not flagged:
            d, via, e = stack.pop()
            end = int(off[d + 1])
            while e < end:
                t = int(ref[e])
                if t == NONE:
                    toks.append((TOK_LEAF, d, e))
                elif t >= D:
                    toks.append((TOK_NIL, d, e))
                elif claims[t] >= 2:
                    flagged = True
                    break
                else:       # a tree ref: d goes on after the child
                    stack.append((d, via, e + 1))
                    stack.append((t, e, int(off[t])))
                    reached.append((t, len(toks)))
                    toks.append((TOK_OPEN, t, e))
                    break
                e += 1
            else:
                toks.append((TOK_CLOSE, d, via))
        if flagged:
            status.append(STATUS_REF_SHARED)
            bo.append(bo[-1])
            continue
        status.append(0)
        for d, at in reached:
            doc_base[d], doc_open[d] = g, bo[-1] + at
        kind += [t[0] for t in toks]
        doc += [t[1] for t in toks]
        ent += [t[2] for t in toks]
        bo.append(bo[-1] + len(toks))
    return RenderBasesResult(np.array(bo, U64), np.array(kind, U8), np.array(doc, U32), np.array(ent, U32),
                             np.array(status, U32), doc_base, doc_open)


def rounds_for(D):
    """The host-known bound of jumping rounds: 2^rounds >= 2 * n_docs."""
    return max(1, int(2 * D - 1).bit_length())


def render_columns(ent_offsets, ent_ref, root_doc) -> RenderBasesResult:
    off, ref, root, D, G, E = _inputs(ent_offsets, ent_ref, root_doc)
    if D == 0 or G == 0:
        z = np.zeros
        return RenderBasesResult(z(G + 1, U64), z(0, U8), z(0, U32), z(0, U32), z(G, U32), np.full(D, NONE, U32),
                                 np.full(D, NONE, U32))
    # 1. link
    claims = claims_of(off, ref, root, D)
    rootbase = np.full(D, -1, I64)
    rootbase[root[root < D]] = np.nonzero(root < D)[0]
    # 2. compact: the tree refs in entry order
    isref = ref < D
    tgt = np.where(isref, ref, 0)
    tree = isref & (claims[tgt] == 1)
    cref = np.nonzero(tree)[0]                          # item k -> its entry
    child = ref[cref]                                   # item k -> the document it opens
    ent_doc = np.searchsorted(off, np.arange(E), side="right") - 1
    ent_doc = np.minimum(ent_doc, D - 1)
    kidx = np.full(D, -1, I64)
    kidx[child] = np.arange(len(cref))
    par = np.full(D, -1, I64)
    par[child] = ent_doc[cref]
    crank = np.searchsorted(cref, off, side="left")     # the tree refs before each boundary
    shared = np.zeros(D, bool)
    shared[ent_doc[isref & (claims[tgt] >= 2)]] = True
    # 3. tour: events 2d = OPEN, 2d + 1 = CLOSE
    d = np.arange(D)
    succ, wt = np.zeros(2 * D, I64), np.zeros(2 * D, I64)
    has = crank[:-1] < crank[1:]
    first = np.where(has, crank[:-1], 0)
    fe = cref[first] if len(cref) else np.zeros(D, I64)
    fc = child[first] if len(cref) else np.zeros(D, I64)
    succ[0::2] = np.where(has, 2 * fc, 2 * d + 1)
    wt[0::2] = np.where(has, 1 + fe - off[:-1], 1 + off[1:] - off[:-1])
    isch = (claims == 1) & (kidx >= 0)
    k = np.where(isch, kidx, 0)
    p = np.where(isch, par, 0)
    pe = cref[k] if len(cref) else np.zeros(D, I64)
    sib = isch & (k + 1 < crank[p + 1])
    k2 = np.where(sib, k + 1, 0)
    e2 = cref[k2] if len(cref) else np.zeros(D, I64)
    c2 = child[k2] if len(cref) else np.zeros(D, I64)
    succ[1::2] = np.where(sib, 2 * c2, np.where(isch, 2 * p + 1, 2 * d + 1))
    wt[1::2] = np.where(sib, e2 - pe, np.where(isch, off[p + 1] - pe, 0))
    # 4. rank
    for _ in range(rounds_for(D)):
        wt = (wt + wt[succ]) & 0xFFFFFFFF
        succ = succ[succ]
    dist = wt + 1
    end = succ[0::2]
    r = end >> 1
    ok = ((end & 1) == 1) & (claims[r] == 1) & (kidx[r] < 0)
    dbase = np.where(ok, rootbase[r], -1)
    size = (dist[0::2] - dist[1::2] + 1) & 0xFFFFFFFF
    start = (dist[2 * r] - dist[0::2]) & 0xFFFFFFFF
    # 5. flag and size
    flag = np.zeros(G, bool)
    flag[dbase[(dbase >= 0) & shared]] = True
    hasroot = root < D
    rt = np.where(hasroot, root, 0)
    flag |= hasroot & (claims[rt] >= 2)
    bsize = np.where(hasroot & ~flag, dist[2 * rt], 0)
    bo = np.concatenate([[0], np.cumsum(bsize)])
    T = int(bo[-1])
    # 6. emit
    valid = (dbase >= 0) & ~flag[np.maximum(dbase, 0)]
    dopen = np.where(valid, bo[np.maximum(dbase, 0)] + start, -1)
    dclose = dopen + size - 1
    kind, doc, ent = np.full(T, 0xEE, U8), np.full(T, NONE, U32), np.full(T, NONE, U32)
    via = np.where(kidx >= 0, pe, NONE)
    v = np.nonzero(valid)[0]
    for at, kd in ((dopen, TOK_OPEN), (dclose, TOK_CLOSE)):
        kind[at[v]], doc[at[v]], ent[at[v]] = kd, v, via[v]
    e = np.nonzero(valid[ent_doc] & ~tree)[0] if E else np.zeros(0, I64)
    assert not (ref[e] < D).any()                       # a ref to a shared document flags the base
    ed = ent_doc[e]
    kk = np.searchsorted(cref, e, side="left")          # the tree refs before e
    after = kk > crank[ed]
    prev = np.where(after, kk - 1, 0)
    pcl = dclose[child[prev]] if len(cref) else np.zeros(len(e), I64)
    pen = cref[prev] if len(cref) else np.zeros(len(e), I64)
    pos = np.where(after, pcl + (e - pen), dopen[ed] + 1 + (e - off[ed]))
    kind[pos], doc[pos], ent[pos] = np.where(ref[e] == NONE, TOK_LEAF, TOK_NIL), ed, e
    assert not (kind == 0xEE).any()                     # every token position was written once
    return RenderBasesResult(bo.astype(U64), kind, doc, ent, np.where(flag, STATUS_REF_SHARED, 0).astype(U32),
                             np.where(valid, dbase, NONE).astype(U32), np.where(valid, dopen, NONE).astype(U32))


def same(got: RenderBasesResult, exp: RenderBasesResult, tokens=True):
    for f in ("base_tok_offsets", "base_status", "doc_base") + (("tok_kind", "tok_doc", "tok_entry") if tokens else ()):
        a, b = getattr(got, f), getattr(exp, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (f, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=f)
    at = exp.doc_base != NONE
    np.testing.assert_array_equal(got.doc_open[at], exp.doc_open[at], err_msg="doc_open")


# ------------------------------------------------------------------ generators
def random_table(rng, n_docs, n_bases, max_ent=6, p_ref=0.4, p_wild=0.25):
    """A random entry table: mostly forests (each document picked as a target at
    most once, parents before or after their children), then with probability
    p_wild per base some refs that break the rule: a second referrer, a ref to a
    root or an ancestor, a dangling target, UINT32_MAX - 1."""
    D = n_docs
    sizes = [rng.choice([0, 0, 1, 2, rng.randint(0, max_ent)]) for _ in range(D)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(U64)
    E = int(off[-1])
    ref = np.full(E, NONE, U32)
    free = list(range(D))
    rng.shuffle(free)
    root = []
    for _ in range(n_bases):
        x = rng.random()
        root.append(free.pop() if free and x < 0.8 else rng.randrange(D) if D and x < 0.9 else D + rng.randrange(3))
    for e in range(E):
        if rng.random() < p_ref:
            x = rng.random()
            if free and x < 1 - p_wild:
                ref[e] = free.pop()
            elif x < 1 - p_wild / 2:
                ref[e] = rng.randrange(D)
            else:
                ref[e] = rng.choice([D, D + 7, NONE - 1])
    return off, ref, np.array(root, U32)
