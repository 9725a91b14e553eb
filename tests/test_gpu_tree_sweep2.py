"""k_tree_l's second sweep at its own tile edges (run on the MI355X box: -m gpu).

Sweep 2 of tree_l_doc (threads by pointer jumping, the links) runs in tiles of
T2 = 4,096 ranks, twice sweep 1's.  Documents of T2 - 1, T2, T2 + 1 and
2 T2 + 1 nodes put the last rank of a tile, the first rank of the next and a
one-rank last tile at every edge; the trees below are the shapes a wrong tile
index would change.  Each batch is woven by the fused kernel (k_weave_doc,
default options) and by the separate kernels (fused = 0, k_tree_l) and compared
with the oracle's effective-tree preorder by equality: weave order, rendered
bits, visible counts, ::lamport-ts, yarns and status.
"""
import random

import numpy as np
import pytest

import oracle
from oracle import causal_ref as R
from cause_amd import abi, pack

pytestmark = pytest.mark.gpu

T2 = 4096  # sweep 2's tile (causeweave.hip tree_l_doc: TILE2 = 2 TILE_T)
SIZES = (T2 - 1, T2, T2 + 1, 2 * T2 + 1)  # nodes a document, the root included
SITE = "aaaaaaaaaaaaa"
ROUTES = {"fused": {}, "separate": {"fused": 0}}


def _id(t):
    return (t, SITE, 0)


def chain(n):
    """Every node caused by the one before it: one in-tile pointer chain as long
    as the tile, and every tile's first rank takes its thread from tab."""
    return [R.ROOT_NODE] + [(_id(t), _id(t - 1) if t > 1 else R.ROOT_ID, "c") for t in range(1, n)]


def star(n):
    """Every node a child of the root: every thread is a sibling."""
    return [R.ROOT_NODE] + [(_id(t), R.ROOT_ID, "s") for t in range(1, n)]


def comb(n):
    """A chain (odd ids) with a leaf (the next even id) at every node: the leaf
    just after a tile start reads its parent's thread across the edge."""
    doc = [R.ROOT_NODE]
    for t in range(1, n):
        if t % 2:
            doc.append((_id(t), _id(t - 2) if t > 1 else R.ROOT_ID, "b"))
        else:
            doc.append((_id(t), _id(t - 1), "l"))
    return doc


def random_tree(n, seed):
    """Random parents (half of them among the newest 64 nodes), about 10% hides
    and 2% shows.  Around every tile edge the specials alternate between a
    target before the edge and one after it (the render bit of a link depends on
    hide_at of the first special child, wherever that lies)."""
    rng = random.Random(seed)
    doc = [R.ROOT_NODE]
    normal = []
    for t in range(1, n):
        near = min((t % T2, T2 - t % T2))  # ranks to the nearest tile edge
        u = rng.random()
        if normal and (u < 0.12 or (near <= 6 and t > 8 and t % 2)):
            if near <= 6 and t > 8:
                edge = (t + 6) // T2 * T2
                before = [x for x in normal[-40:] if x < edge]
                after = [x for x in normal[-40:] if x >= edge]
                pool = after if after and t % 4 == 1 else before or normal
                target = rng.choice(pool)
            else:
                target = rng.choice(normal[-64:] if rng.random() < 0.5 else normal)
            doc.append((_id(t), _id(target), R.H_SHOW if u < 0.02 or t % 8 == 5 else R.HIDE))
        else:
            if not normal:
                parent = R.ROOT_ID
            else:
                parent = _id(rng.choice(normal[-64:] if rng.random() < 0.5 else normal))
            doc.append((_id(t), parent, "x"))
            normal.append(t)
    return doc


def _shuffled(docs, seed):
    rng = random.Random(seed)
    for d in docs:
        rng.shuffle(d)
    return docs


def _batches():
    b = {"chain": [chain(n) for n in SIZES],
         "star": [star(n) for n in SIZES],
         "comb": [comb(n) for n in SIZES],
         "random": [random_tree(n, 100 + i) for i, n in enumerate(SIZES)],
         # every size and shape in one batch, an empty and a one-node document among them
         "ragged": [chain(T2 + 1), [], star(T2 - 1), [R.ROOT_NODE], comb(2 * T2 + 1),
                    random_tree(T2, 7), chain(T2 - 1), random_tree(2 * T2 + 1, 8), star(T2 + 1)]}
    return {name: _shuffled(docs, 5) for name, docs in b.items()}


@pytest.fixture(scope="module")
def cases():
    """name -> (packed batch, the oracle's outputs), computed once for both routes."""
    out = {}
    for name, docs in _batches().items():
        b = pack.pack_lists(docs)
        off, lay = b.offsets, b.layout
        perm, vis, st = oracle.batch_lists(off, b.id_key, b.cause_key, b.kind, method=oracle.METHOD_EFF)
        D = len(off) - 1
        span = [(int(off[d]), int(off[d + 1])) for d in range(D)]
        vcount = np.array([int(vis[lo:hi].sum()) for lo, hi in span], np.uint32)
        max_ts = np.array([int(b.id_key[lo:hi].max() >> np.uint64(lay.ts_shift)) if hi > lo else 0
                           for lo, hi in span], np.uint64)
        mask = (1 << lay.site_bits) - 1
        yarns = [oracle.list_yarns(b.id_key[lo:hi], lay.site_shift, mask) for lo, hi in span]
        out[name] = (b, span, perm, vis, st, vcount, max_ts, yarns)
    return out


@pytest.fixture(scope="module", params=sorted(ROUTES))
def weaver(request):
    with abi.Weaver(0, options=ROUTES[request.param]) as w:
        yield w


@pytest.mark.parametrize("name", ["chain", "star", "comb", "random", "ragged"])
def test_sweep2_tile_edges(weaver, cases, name):
    b, span, perm, vis, st, vcount, max_ts, yarns = cases[name]
    res = weaver.weave_lists(b.offsets, b.id_key, b.cause_key, b.kind, b.layout, yarns=True)
    assert np.array_equal(res.status, st), (res.status, st)
    gvis = res.visible()
    for d, (lo, hi) in enumerate(span):
        assert np.array_equal(res.weave_perm[lo:hi], perm[lo:hi]), f"{name} doc {d} ({hi - lo} nodes): order"
        assert np.array_equal(gvis[lo:hi], vis[lo:hi]), f"{name} doc {d} ({hi - lo} nodes): visibility"
        if b.layout.site_bits:
            assert np.array_equal(res.yarn_perm[lo:hi], yarns[d]), f"{name} doc {d}: yarns"
    assert np.array_equal(res.visible_count, vcount)
    ne = np.array([hi > lo for lo, hi in span])
    assert np.array_equal(res.max_ts[ne], max_ts[ne])


def test_shapes_are_what_they_claim():
    """The generators give the sizes and shapes the edge cases rest on (no GPU
    work: a wrong generator would leave the edges untested without a failure)."""
    for n in SIZES:
        for doc in (chain(n), star(n), comb(n), random_tree(n, 1)):
            assert len(doc) == n and len({x[0] for x in doc}) == n
    c = chain(T2 + 1)
    assert all(c[t][1] == c[t - 1][0] for t in range(1, T2 + 1))
    assert all(x[1] == R.ROOT_ID for x in star(T2)[1:])
    cb = comb(T2 + 1)
    assert cb[T2][1] == _id(T2 - 1) and cb[T2 - 1][1] == _id(T2 - 3)  # the leaf at rank T2: parent before the edge
    rt = random_tree(2 * T2 + 1, 100)
    spec = [x for x in rt[1:] if x[2] in (R.HIDE, R.H_SHOW)]
    assert 0.08 < len(spec) / len(rt) < 0.16
    near = [x for x in spec if abs(x[0][0] - T2) <= 6]  # (the edge at 2 T2 has one rank after it)
    assert any(x[1][0] < T2 <= x[0][0] for x in near)  # a special after the edge, target before it
    assert any(x[1][0] >= T2 for x in near)  # ... and a target after it
    assert any(x[0][0] < T2 for x in near)  # ... and specials before it
