"""Array-level K128 batches with a cheap exact reference.

A K64 batch (offsets, id_key, cause_key, kind, layout) -- from gen.generate or
pack.pack_lists -- is split into (ts, site, tx) by its layout and every
component is sent through a strictly increasing map:

    hi = f(ts)        lo = g(site) << 32 | h(tx)        nil stays (NIL, NIL)

(compare a b) on ids is lexicographic on [ts site tx] (util.cljc:4-10), so
strictly increasing maps per component keep every order relation and every
equality between ids and causes.  The weave, the rendered bits, the counts and
the status of the widened batch are therefore the oracle's on the K64 batch;
::lamport-ts is f(largest ts) and the yarns are the K64 yarns (g keeps the
site order).  h may differ from site to site: tx only decides between ids of
one ts and one site.  The root [0 "0" 0] keeps ts 0 (f(0) = 0).

No GPU result enters an expectation: tests/test_k128_gen.py proves this
module on the CPU (lexsort ranks of the wide words against the K64 ranks, the
word edges each widening is named for, the status of every corruption, and the
tuple route pack_lists_k128 + renumber that tests/test_gpu_k128.py trusts).

Corruptions are written onto the 128-bit words and mirrored on the K64 side.
The literal fold looks at a cause only to find the node it names and, once
found, to compare it with the node's id; an absent cause is absent whatever
its value.  So a wide cause without a K64 preimage (one word flipped in one
bit) is mirrored by a K64 key that no node of the document holds.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np

import oracle
from cause_amd import abi, gen, pack
from oracle import causal_ref as R

TILE = 4096                # cw_internal.h TILE: the segmented sort's tile
NIL = np.uint64(pack.NIL)
TOP63 = (1 << 63) - 1      # the largest lamport-ts (a Clojure Long)
M32 = (1 << 32) - 1        # the largest site rank and the largest tx-index
BIT63 = np.uint64(1 << 63)
WIDENINGS = ("top", "hi_only", "lo_only", "sparse")


def _u(x):
    return np.uint64(x)


@dataclass
class K64:
    off: np.ndarray
    idk: np.ndarray
    ck: np.ndarray
    kd: np.ndarray
    layout: pack.KeyLayout

    @property
    def D(self):
        return len(self.off) - 1

    def span(self, d):
        return int(self.off[d]), int(self.off[d + 1])


@dataclass
class Wide:
    """A K128 batch, its K64 mirror (what the oracle is given) and what the
    mirror does not say: ::lamport-ts and where the yarns' site field lies."""
    name: str
    k64: K64
    id2: np.ndarray        # uint64 [N, 2] (hi, lo)
    ca2: np.ndarray        # uint64 [N, 2]
    max_ts: np.ndarray     # uint64 [D] f(largest ts); 0 for an empty document
    yarn_shift: int        # site(K64 key) = key >> yarn_shift & yarn_mask
    yarn_mask: int
    dup_docs: frozenset = frozenset()  # documents deliberately given a repeated id
    claims: dict = dataclasses.field(default_factory=dict)  # doc -> (corruption, status bits)

    @property
    def off(self):
        return self.k64.off

    @property
    def kd(self):
        return self.k64.kd


# ------------------------------------------------------------ K64 batches ----

def concat(docs, layout) -> K64:
    """docs: (id_key, cause_key, kind) per document, all of one layout."""
    off = np.zeros(len(docs) + 1, np.uint64)
    off[1:] = np.cumsum([len(d[0]) for d in docs])
    cat = lambda j, dt: (np.concatenate([np.asarray(d[j], dt) for d in docs]) if docs
                         else np.zeros(0, dt))
    return K64(off, cat(0, np.uint64), cat(1, np.uint64), cat(2, np.uint8), layout)


def random_docs(sizes, seed0, n_sites=gen.CONFIG2.n_sites) -> K64:
    """config-2 shaped documents (hides, shows, conjoined runs), one per size
    (nodes with the root; 0 = an empty document)."""
    docs = []
    for i, n in enumerate(sizes):
        if n == 0:
            docs.append((np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8)))
            continue
        spec = dataclasses.replace(gen.CONFIG2, nodes_per_doc=n - 1, seed=seed0 + i, n_sites=n_sites)
        _, idk, ck, kd = gen.generate(spec, 0, 1)
        docs.append((idk, ck, kd))
    lay = dataclasses.replace(gen.CONFIG2, nodes_per_doc=max(max(sizes) - 1, 1),
                              n_sites=n_sites).layout()
    return concat(docs, lay)


def from_tuples(docs) -> K64:
    """Clojure-shaped documents (nodes with the root) through pack.pack_lists."""
    b = pack.pack_lists(docs)
    return K64(b.offsets, b.id_key, b.cause_key, b.kind, b.layout)


LO_SITES = ("aaaaaaaaaaaaa", "bbbbbbbbbbbbb", "ccccccccccccc")


def one_ts(doc):
    """A one-site document with ids (t, site, 0), t = 1 .. n - 1 (the chain, star
    and comb of tests/test_gpu_tree_sweep2.py), relabelled so that every
    non-root node has ts 1: id t becomes (1, LO_SITES[(t - 1) // m], (t - 1) % m)
    with m = ceil((n - 1) / 3), which orders the ids as t did.  The second and
    the third site hold the same tx-indices."""
    n = len(doc)
    m = max(1, -(-(n - 1) // len(LO_SITES)))

    def w(i):
        if i is None or i == R.ROOT_ID:
            return i
        t = i[0]
        return (1, LO_SITES[(t - 1) // m], (t - 1) % m)

    return [(w(i), w(c), v) for i, c, v in doc]


# ---------------------------------------------------- strictly increasing ----

class Mono:
    """A strictly increasing map given on the sorted values it is used on."""

    def __init__(self, dom, img):
        self.dom = np.asarray(dom, np.uint64)
        self.img = np.asarray(img, np.uint64)
        assert len(self.dom) == len(self.img)
        assert (self.dom[1:] > self.dom[:-1]).all()
        assert (self.img[1:] > self.img[:-1]).all(), "not strictly increasing"

    def index(self, x):
        j = np.searchsorted(self.dom, x)
        assert (j < len(self.dom)).all() and (self.dom[np.minimum(j, len(self.dom) - 1)] == x).all(), \
            "value outside the map's domain"
        return j

    def __call__(self, x):
        return self.img[self.index(np.asarray(x, np.uint64))]


def _spread(n, top):
    """0 .. top in n even steps, the last one at top."""
    if n == 1:
        return np.zeros(1, np.uint64)
    return np.array([j * top // (n - 1) for j in range(n)], np.uint64)


def _random_increasing(rng, dom, top):
    """Random gaps of 1 .. top / n: strictly increasing, at most top; 0 -> 0."""
    n = len(dom)
    img = np.cumsum(rng.integers(1, max(top // n, 1), size=n, dtype=np.uint64, endpoint=True),
                    dtype=np.uint64)
    if n and dom[0] == 0:
        img = img - img[0]
    return img


def split(keys, lay):
    """(ts, site, tx) of K64 keys by the layout (nil entries give garbage)."""
    k = np.asarray(keys, np.uint64)
    ts = k >> _u(lay.ts_shift)
    site = (k >> _u(lay.site_shift)) & _u((1 << lay.site_bits) - 1)
    tx = k & _u((1 << lay.tx_bits) - 1)
    return ts, site, tx


def _domains(b: K64):
    """Sorted values of each component over the ids and the id causes."""
    isid = b.ck != NIL
    assert (b.idk < BIT63).all() and (b.ck[isid] < BIT63).all(), "widen a clean K64 batch"
    both = np.concatenate([b.idk, b.ck[isid]])
    return tuple(np.unique(c) for c in split(both, b.layout))


def _f_top(ts_dom):
    """ts + 2^63 - 1 - max ts, the root's ts 0 kept."""
    mx = int(ts_dom[-1]) if len(ts_dom) else 0
    return Mono(ts_dom, [0 if int(t) == 0 else int(t) + TOP63 - mx for t in ts_dom])


def widen(b: K64, name: str, seed: int = 0) -> Wide:
    assert name in WIDENINGS
    lay = b.layout
    N = len(b.idk)
    isid = b.ck != NIL
    ts_dom, site_dom, tx_dom = _domains(b)
    rng = np.random.default_rng(seed)
    yarn_shift, yarn_mask = lay.site_shift, (1 << lay.site_bits) - 1

    if name == "hi_only":
        # the whole id in hi (one site, tx 0): hi = key * c, the largest key near 2^63 - 1
        mx = int(max(b.idk.max() if N else 0, b.ck[isid].max() if isid.any() else 0))
        c = _u(TOP63 // mx if mx else 1)
        F = lambda k: np.stack([np.asarray(k, np.uint64) * c, np.zeros(len(k), np.uint64)], axis=1)
        id2, ca2 = F(b.idk), F(b.ck)
        ts_of = lambda k: np.asarray(k, np.uint64) * c
        yarn_shift, yarn_mask = 0, 0
    else:
        if name == "top":
            f = _f_top(ts_dom)
            g = Mono(site_dom, _spread(len(site_dom), M32))
            k = M32 // int(tx_dom[-1]) if len(tx_dom) and int(tx_dom[-1]) else 1
            H = np.tile(tx_dom * _u(k), (len(site_dom), 1))
        elif name == "lo_only":
            assert len(ts_dom[ts_dom != 0]) <= 1, "lo_only: every non-root node of one ts"
            f = _f_top(ts_dom)
            m = len(site_dom)
            # the two largest sites differ in bit 31 alone: lo bit 63
            if m >= 3:
                img = [j * (M32 >> 1) // (m - 2) for j in range(m - 2)] + [M32 >> 1, M32]
            else:
                img = [0, M32][:m]
            g = Mono(site_dom, img)
            # tx 2j and 2j + 1 differ in bit 0 alone; the pairs spread to the top
            n = len(tx_dom)
            step = max(2, (M32 // ((n + 1) // 2 or 1)) & ~1)
            H = np.tile(np.array([(j >> 1) * step | (j & 1) for j in range(n)], np.uint64), (m, 1))
        else:  # sparse
            f = Mono(ts_dom, _random_increasing(rng, ts_dom, TOP63))
            g = Mono(site_dom, _random_increasing(rng, site_dom, M32))
            H = np.stack([_random_increasing(rng, tx_dom, M32) if len(tx_dom) > 1
                          else rng.integers(0, M32, size=1, dtype=np.uint64, endpoint=True)
                          for _ in site_dom]) if len(site_dom) else np.zeros((0, 0), np.uint64)
            if len(site_dom) and len(tx_dom) and site_dom[0] == 0 and tx_dom[0] == 0:
                H[0] = H[0] - H[0, 0]  # the root's lo word stays 0
        assert (H <= _u(M32)).all() and (g.img <= _u(M32)).all() and (f.img <= _u(TOP63)).all()
        assert all((row[1:] > row[:-1]).all() for row in H)
        site_ix, tx_ix = Mono(site_dom, np.arange(len(site_dom))), Mono(tx_dom, np.arange(len(tx_dom)))

        def F(keys, ok):
            out = np.full((len(keys), 2), NIL, np.uint64)
            ts, site, tx = split(keys[ok], lay)
            s = site_ix.index(site)
            out[ok, 0] = f(ts)
            out[ok, 1] = (g.img[s] << _u(32)) | H[s, tx_ix.index(tx)]
            return out

        id2, ca2 = F(b.idk, np.ones(N, bool)), F(b.ck, isid)
        ts_of = lambda k: f(split(k, lay)[0])

    ca2[~isid] = NIL
    max_ts = np.zeros(b.D, np.uint64)
    for d in range(b.D):
        lo, hi = b.span(d)
        if hi > lo:
            max_ts[d] = ts_of(b.idk[lo:hi].max(keepdims=True))[0]
    k64 = K64(b.off, b.idk.copy(), b.ck.copy(), b.kd, lay)
    return Wide(name, k64, id2, ca2, max_ts, yarn_shift, yarn_mask)


# ------------------------------------------------------------ expectation ----

@dataclass
class Expected:
    perm: np.ndarray      # uint32 [N] doc-local input index per weave position
    vis: np.ndarray       # uint8 [N] per weave position
    st: np.ndarray        # uint32 [D]
    vcount: np.ndarray    # uint32 [D]
    yarns: dict           # (yarn_shift, yarn_mask) -> uint32 [N] doc-local


def expect(b: K64, method) -> Expected:
    """The oracle on the K64 batch: one run serves every widening of it."""
    perm, vis, st = oracle.batch_lists(b.off, b.idk, b.ck, b.kd, method=method)
    vcount = np.array([int(vis[slice(*b.span(d))].sum()) for d in range(b.D)], np.uint32)
    e = Expected(perm, vis, st, vcount, {})
    for a in (perm, vis, st, vcount):
        a.setflags(write=False)
    return e


def yarns_of(e: Expected, w: Wide) -> np.ndarray:
    key = (w.yarn_shift, w.yarn_mask)
    if key not in e.yarns:
        b = w.k64
        y = np.zeros(len(b.idk), np.uint32)
        for d in range(b.D):
            lo, hi = b.span(d)
            y[lo:hi] = oracle.list_yarns(b.idk[lo:hi], *key)
        y.setflags(write=False)
        e.yarns[key] = y
    return e.yarns[key]


def compare(res, w: Wide, e: Expected, max_ts=True, yarns=True):
    """Bit-exact, per document.  Only the documents deliberately given a
    repeated id are skipped for order, visibility, count and yarns (their output
    is unspecified); their status is compared, and the documents the oracle
    flags DUP must be exactly those."""
    b = w.k64
    dup = frozenset(int(d) for d in np.nonzero(e.st & abi.STATUS_DUP)[0])
    assert dup == w.dup_docs, (sorted(dup), sorted(w.dup_docs))
    assert np.array_equal(res.status, e.st), (w.name, res.status, e.st)
    gvis = res.visible()
    want_y = yarns_of(e, w) if yarns else None
    for d in range(b.D):
        if d in dup:
            continue
        lo, hi = b.span(d)
        tag = f"{w.name} doc {d} ({hi - lo} nodes)"
        assert np.array_equal(res.weave_perm[lo:hi], e.perm[lo:hi]), f"{tag}: order"
        assert np.array_equal(gvis[lo:hi], e.vis[lo:hi]), f"{tag}: visibility"
        assert int(res.visible_count[d]) == int(e.vcount[d]), f"{tag}: count"
        if max_ts:
            assert int(res.max_ts[d]) == int(w.max_ts[d]), f"{tag}: lamport-ts"
        if yarns:
            assert np.array_equal(res.yarn_perm[lo:hi], want_y[lo:hi]), f"{tag}: yarns"


# ------------------------------------------------------------ corruptions ----

ORPHAN, NON_LAMPORT, DUP = abi.STATUS_ORPHAN, abi.STATUS_NON_LAMPORT, abi.STATUS_DUP
NON_ID2 = np.array(pack.NON_ID_CAUSE2, np.uint64)

# name -> the status the document must get (an in-domain document, one node changed)
CORRUPTIONS = {"hi_hit_lo_miss": ORPHAN,   # a cause equal to an id in hi, its lo absent
               "lo_hit_hi_miss": ORPHAN,   # ... equal in lo, its hi absent
               "above_all": ORPHAN,        # a cause above every id
               "nil_hi": ORPHAN,           # (NIL, x), x != NIL: not nil, an absent id
               "non_id": ORPHAN,           # pack.NON_ID_CAUSE2
               "nil_cause": ORPHAN,        # a nil cause on a non-root node
               "younger": NON_LAMPORT,     # a cause younger than its node
               "dup": DUP}                 # a repeated id across sorted position TILE


def _has(id2, hi, lo):
    return bool(((id2[:, 0] == _u(hi)) & (id2[:, 1] == _u(lo))).any())


def corrupt(w: Wide, plan, seed=0) -> Wide:
    """plan[d]: a name of CORRUPTIONS, or None to leave document d alone.  One
    node of the document is changed, on the wide words and on the K64 mirror."""
    rng = np.random.default_rng(seed)
    b = w.k64
    id2, ca2 = w.id2.copy(), w.ca2.copy()
    idk, ck = b.idk.copy(), b.ck.copy()
    dups, claims = set(w.dup_docs), dict(w.claims)
    for d, what in enumerate(plan):
        if what is None:
            continue
        lo, hi = b.span(d)
        n = hi - lo
        i2, c2, ik, cc = id2[lo:hi], ca2[lo:hi], idk[lo:hi], ck[lo:hi]  # views
        order = np.lexsort((i2[:, 1], i2[:, 0]))  # sorted position -> input index
        assert n > TILE + 1 and b.kd[lo + order[0]] & pack.KIND_ROOT
        absent64 = _u(int(ik.max()) + 1)           # a K64 key no node holds
        v = int(order[rng.integers(n // 4, n // 2)])   # the node that gets the cause
        t = int(order[rng.integers(1, n)])             # an id of the document (not the root)
        th, tl = int(i2[t, 0]), int(i2[t, 1])
        if what == "hi_hit_lo_miss":
            for bit in (1, 1 << 63, 1 << 32, 2):
                if not _has(i2, th, tl ^ bit):
                    break
            assert not _has(i2, th, tl ^ bit)
            c2[v], cc[v] = (th, tl ^ bit), absent64
        elif what == "lo_hit_hi_miss":
            for bit in (1, 2, 4, 8, 1 << 62):  # the nearest hi that no id of the document has
                if not (i2[:, 0] == _u(th ^ bit)).any():
                    break
            assert not (i2[:, 0] == _u(th ^ bit)).any()
            c2[v], cc[v] = (th ^ bit, tl), absent64
        elif what == "above_all":
            c2[v], cc[v] = (int(i2[:, 0].max()), (1 << 64) - 3), absent64
        elif what == "nil_hi":
            assert tl != pack.NIL
            c2[v], cc[v] = (pack.NIL, tl), absent64
        elif what == "non_id":
            c2[v], cc[v] = NON_ID2, pack.NON_ID_CAUSE
        elif what == "nil_cause":
            c2[v], cc[v] = (pack.NIL, pack.NIL), pack.NIL
        elif what == "younger":
            pos = int(np.nonzero(order == v)[0][0])
            y = int(order[rng.integers(pos + 1, n)])
            c2[v], cc[v] = i2[y], ik[y]
        elif what == "dup":
            # sorted positions TILE - 1 and TILE get one id: the node that no
            # other node names as its cause takes its neighbour's
            p, q = int(order[TILE - 1]), int(order[TILE])
            if not (cc == ik[p]).any():
                i2[p], ik[p] = i2[q], ik[q]
            else:
                i2[q], ik[q] = i2[p], ik[p]
            dups.add(d)
        else:
            raise ValueError(what)
        claims[d] = (what, CORRUPTIONS[what])
    k64 = K64(b.off, idk, ck, b.kd, b.layout)
    # a repeated id does not move the largest ts of these documents (position TILE of > TILE + 1)
    return Wide(w.name, k64, id2, ca2, w.max_ts, w.yarn_shift, w.yarn_mask, frozenset(dups), claims)


# --------------------------------------------------- numpy ranks (the proof) --

def _dense(cols):
    """Dense group numbers of the rows of `cols` (equal rows, equal number;
    ordered as the rows compare, first column first)."""
    order = np.lexsort(tuple(reversed(cols)))
    new = np.zeros(len(order), bool)
    for c in cols:
        s = c[order]
        new[1:] |= s[1:] != s[:-1]
    g = np.empty(len(order), np.int64)
    g[order] = np.cumsum(new)
    return g


def ranks(id_cols, cause_cols, nil):
    """One document: (rank of every id among the document's ids, equal ids
    sharing the first's; the rank of the id every cause equals, -1 for a cause
    that is no id of the document, -2 for nil)."""
    n = len(id_cols[0])
    g = _dense([np.concatenate([i, c]) for i, c in zip(id_cols, cause_cols)])
    gi, gc = g[:n], g[n:]
    order = np.argsort(gi, kind="stable")
    first = np.full(int(g.max()) + 1 if len(g) else 0, -1, np.int64)  # group -> rank of its first id
    sg = gi[order]
    starts = np.nonzero(np.r_[True, sg[1:] != sg[:-1]])[0] if n else np.zeros(0, np.int64)
    first[sg[starts]] = starts
    rid = first[gi]
    rc = first[gc] if n else np.zeros(0, np.int64)
    rc = np.where(nil, -2, rc)
    return rid, rc


def ranks_k64(b: K64, d):
    lo, hi = b.span(d)
    return ranks([b.idk[lo:hi]], [b.ck[lo:hi]], b.ck[lo:hi] == NIL)


def ranks_k128(w: Wide, d):
    lo, hi = w.k64.span(d)
    i, c = w.id2[lo:hi], w.ca2[lo:hi]
    return ranks([i[:, 0], i[:, 1]], [c[:, 0], c[:, 1]], (c[:, 0] == NIL) & (c[:, 1] == NIL))


# ------------------------------------------------- back to Clojure shapes ----

_VALUES = {pack.KIND_NORMAL: "x", pack.KIND_HIDE: R.HIDE, pack.KIND_HHIDE: R.H_HIDE,
           pack.KIND_HSHOW: R.H_SHOW}


def to_tuples(w: Wide):
    """The wide batch as Clojure-shaped documents: [hi site tx] with a
    13-character site-id that sorts as the site rank does (the root is
    [0 "0" 0] whatever its words).  For small batches
    (the tuple route of tests/test_gpu_k128.py)."""
    docs = []
    for d in range(w.k64.D):
        lo, hi = w.k64.span(d)
        roots = [tuple(w.id2[j].tolist()) for j in range(lo, hi) if w.kd[j] & pack.KIND_ROOT]
        r0 = roots[0][1] >> 32 if roots else 0  # the site "0" keeps its place among the sites

        def ident(hi, lo):
            if (int(hi), int(lo)) in roots:
                return R.ROOT_ID
            x = int(lo) >> 32
            if x == r0:
                return (int(hi), "0", int(lo) & M32)
            return (int(hi), (" " if x < r0 else "a") + f"{x:012d}", int(lo) & M32)

        doc = []
        for j in range(lo, hi):
            i, c, k = w.id2[j], w.ca2[j], int(w.kd[j])
            if k & pack.KIND_ROOT:
                doc.append(R.ROOT_NODE)
                continue
            if c[0] == NIL and c[1] == NIL:
                cause = None
            elif c[0] == NIL:
                cause = "not-an-id"
            else:
                cause = ident(c[0], c[1])
            doc.append((ident(i[0], i[1]), cause, _VALUES[k & 3]))
        docs.append(doc)
    return docs


# ------------------------------------------------- the batches of the tests --
# name -> (K64 builder, widenings, oracle method).  tests/test_k128_gen.py
# proves every one of them; tests/test_gpu_k128_shapes.py weaves them.

EDGE_SIZES = (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 20_000)
SEVERAL_SIZES = (70_001, 3_000, 0, 66_000)
CAUSE_PLAN = tuple(CORRUPTIONS) + (None,)   # eight corrupted documents and a clean one
CAUSE_NODES = 9_000


def _shape_docs():
    from tests.test_gpu_tree_sweep2 import chain, comb, star
    import random

    docs = [shape(n) for shape in (chain, star, comb) for n in (TILE - 1, TILE + 1)]
    return docs, random.Random(5)


def _shapes():
    docs, rng = _shape_docs()
    for d in docs:
        rng.shuffle(d)
    return from_tuples(docs)


def _shapes_one_ts():
    docs, rng = _shape_docs()
    docs = [one_ts(d) for d in docs]
    for d in docs:
        rng.shuffle(d)
    return from_tuples(docs)


BATCHES = {
    "edges": (lambda: random_docs(EDGE_SIZES, 2100), ("top", "sparse", "hi_only"), oracle.METHOD_EFF),
    "shapes": (_shapes, ("top",), oracle.METHOD_EFF),
    "shapes_one_ts": (_shapes_one_ts, ("lo_only",), oracle.METHOD_EFF),
    "n65535": (lambda: random_docs((65_535,), 2200), ("top", "sparse"), oracle.METHOD_EFF),
    "n65536": (lambda: random_docs((65_536,), 2201), ("top", "sparse"), oracle.METHOD_EFF),
    "n5000": (lambda: random_docs((5_000,), 2202), ("top",), oracle.METHOD_EFF),
    "several": (lambda: random_docs(SEVERAL_SIZES, 2300), ("sparse",), oracle.METHOD_EFF),
    "causes": (lambda: random_docs((CAUSE_NODES,) * len(CAUSE_PLAN), 2400), ("top",),
               oracle.METHOD_LITERAL),
}

_K64, _WIDE, _EXPECTED = {}, {}, {}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def wide(name, widening) -> Wide:
    """The batch `name` under a widening: made once, never written to."""
    assert widening in BATCHES[name][1]
    if (name, widening) not in _WIDE:
        if name not in _K64:
            _K64[name] = BATCHES[name][0]()
        w = widen(_K64[name], widening, seed=len(name))
        if name == "causes":
            w = corrupt(w, CAUSE_PLAN, seed=7)
        _freeze(w.id2, w.ca2, w.max_ts, w.k64.off, w.k64.idk, w.k64.ck, w.k64.kd)
        _WIDE[name, widening] = w
    return _WIDE[name, widening]


def expected(name) -> Expected:
    """The oracle's outputs for the batch `name` (its K64 mirror, the same under
    every widening): one run, shared."""
    if name not in _EXPECTED:
        _EXPECTED[name] = expect(wide(name, BATCHES[name][1][0]).k64, BATCHES[name][2])
    return _EXPECTED[name]
