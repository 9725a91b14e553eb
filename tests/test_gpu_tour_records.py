"""The tour's split walk records (tour_doc: k_weave_doc and k_tour): a node's
sublist goes to HBM scratch as a u16, its index inside the sublist into the
node's own successor slot in LDS, and the placement takes the indices of its
nodes into registers (two a VGPR, 64 a thread at the most) before the weave
reuses the slots.  Bit-exact against the CPU oracle (run on the MI355X box:
-m gpu).

Every document of every batch is compared with oracle.batch_lists(...,
METHOD_EFF) on weave order, visibility, visible count and status, as in
tests/test_gpu_tour_pipeline.py: one oracle run per batch serves every
context configuration.

Sizes (nodes of a document, the root included).  A thread's k-th index
register entry is node tid + k * 1,024: 1,023 / 1,024 / 1,025 are one entry a
thread and the first of a second; 8,191 / 8,192 / 8,193 one placement batch
(8 entries) and the first node of the next; 50,001 the flagship's 49 entries
(the seventh batch partly filled) with, at the default 8-node splitter blocks,
S = 6,251 sublists, most of them taken from the LDS counter; below 64 a single
wave's partial batch.  The splitter blocks are sized by a batch's largest
document, so 65,535 (64 entries: the whole register array; the blocks grow to
32 nodes) has a batch of its own, one document of every shape.

Under tour_log2k 7 the sublists average 128 nodes: indices pass 255 and use
the second byte of the slot (asserted below on the CPU for the 65,535-node
random document).  yarns=True on a layout with a 5-bit site field sends the
batch through the u32-sval instantiation of k_weave_doc.
"""
import dataclasses

import numpy as np
import pytest

import oracle
from cause_amd import abi, gen, pack

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 50_001]
BIG = 65_535
CONFIGS = {"default": {}, "separate": {"fused": 0}, "log2k4": {"tour_log2k": 4},
           "log2k7": {"tour_log2k": 7}}
LAYOUT = pack.KeyLayout(17, 1, 0)  # chain and star: ts | site rank (the root's "0" = 0, one site = 1)


def _tree_doc(n, shape, rng):
    """n nodes with the root, ids 1..n-1 of one site, in shuffled input order.
    chain: every node caused by the one before; star: every node a child of
    the root."""
    t = np.arange(n, dtype=np.uint64)
    idk = (t << np.uint64(1)) | np.uint64(1)
    idk[0] = 0
    prev = ((t - np.uint64(1)) << np.uint64(1)) | np.uint64(1)
    ck = prev if shape == "chain" else np.zeros(n, np.uint64)
    ck = ck.copy()
    if n > 1:
        ck[1] = 0
    ck[0] = np.uint64(pack.NIL)
    kd = np.zeros(n, np.uint8)
    kd[0] = pack.KIND_ROOT
    p = rng.permutation(n)
    return idk[p], ck[p], kd[p]


def _concat(docs):
    off = np.zeros(len(docs) + 1, np.uint64)
    off[1:] = np.cumsum([len(d[0]) for d in docs])
    return (off, np.concatenate([d[0] for d in docs]), np.concatenate([d[1] for d in docs]),
            np.concatenate([d[2] for d in docs]))


def _random_docs(sizes, seed0, n_sites=gen.CONFIG2.n_sites):
    """config-2 style documents (hides, shows, conjoined runs), one per size"""
    docs = []
    for i, n in enumerate(sizes):
        spec = dataclasses.replace(gen.CONFIG2, nodes_per_doc=n - 1, seed=seed0 + i, n_sites=n_sites)
        _, idk, ck, kd = gen.generate(spec, 0, 1)
        docs.append((idk, ck, kd))
    lay = dataclasses.replace(gen.CONFIG2, nodes_per_doc=max(sizes) - 1, n_sites=n_sites).layout()
    return _concat(docs), lay


def _make(shape):
    rng = np.random.default_rng(11)
    if shape in ("chain", "star"):
        return _concat([_tree_doc(n, shape, rng) for n in SIZES]), LAYOUT
    if shape == "random":
        return _random_docs(SIZES, 1200)
    if shape == "sites20":  # a 5-bit site field: the yarns leave the fused kernel's u16 sval
        return _random_docs([1025, 8193, 50_001], 1300, n_sites=20)
    assert shape == "big"  # every shape at the largest u16 document; the random one first
    (off, idk, ck, kd), lay = _random_docs([BIG], 1250)
    sh = np.uint64(lay.ts_shift - LAYOUT.ts_shift)  # chain and star in the random document's layout
    docs = [(idk, ck, kd)]
    for s in ("chain", "star"):
        i, c, k = _tree_doc(BIG, s, rng)
        docs.append((i << sh, np.where(c == np.uint64(pack.NIL), c, c << sh), k))
    return _concat(docs), lay


_BATCHES = {}


def _batch(shape):
    """(inputs, layout, oracle outputs) of a shape: made and woven by the
    oracle once, shared by every configuration, never written to"""
    if shape not in _BATCHES:
        (off, idk, ck, kd), lay = _make(shape)
        perm, vis, st = oracle.batch_lists(off, idk, ck, kd, method=oracle.METHOD_EFF)
        for a in (off, idk, ck, kd, perm, vis, st):
            a.setflags(write=False)
        _BATCHES[shape] = (off, idk, ck, kd, lay, perm, vis, st)
    return _BATCHES[shape]


def _check(res, off, perm, vis, st):
    assert np.array_equal(res.status, st), (res.status, st)
    gvis = res.visible()
    for d in range(len(off) - 1):
        b, e = int(off[d]), int(off[d + 1])
        assert np.array_equal(res.weave_perm[b:e], perm[b:e]), f"doc {d} ({e - b} nodes) order"
        assert np.array_equal(gvis[b:e], vis[b:e]), f"doc {d} ({e - b} nodes) visibility"
        assert int(res.visible_count[d]) == int(vis[b:e].sum()), f"doc {d} ({e - b} nodes) count"


@pytest.mark.parametrize("shape", ["chain", "star", "random", "big"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_tour_records_vs_oracle(config, shape):
    off, idk, ck, kd, lay, perm, vis, st = _batch(shape)
    assert not st.any(), st
    with abi.Weaver(0, options=CONFIGS[config]) as w:
        res = w.weave_lists(off, idk, ck, kd, lay, yarns=False)
    _check(res, off, perm, vis, st)


def test_tour_records_u32_sval_with_yarns():
    """yarns of a site field wider than k_yarn_doc's 4 bits: k_weave_doc
    writes u32 sval for the yarn sort, and the tour places those."""
    off, idk, ck, kd, lay, perm, vis, st = _batch("sites20")
    assert lay.site_bits > 4 and not st.any()
    with abi.Weaver(0) as w:
        res = w.weave_lists(off, idk, ck, kd, lay, yarns=True)
    _check(res, off, perm, vis, st)
    mask = (1 << lay.site_bits) - 1
    for d in range(len(off) - 1):
        b, e = int(off[d]), int(off[d + 1])
        want = oracle.list_yarns(idk[b:e], lay.site_shift, mask)
        assert np.array_equal(res.yarn_perm[b:e], want), f"doc {d} yarns"


def _mix32(a, b):
    """cw_internal.h mix32"""
    m = 0xFFFFFFFF
    h = (a * 0x9E3779B1 + b) & m
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def _sublist_lengths(d, idk, perm, log2k):
    """Lengths of document d's tour sublists under 2^log2k-node splitter
    blocks, from the oracle's order: the tour's nodes are the id ranks, block
    j's splitter is cw_internal.h split_node(d, j), and a sublist runs in weave
    order from one splitter to the next."""
    n = len(idk)
    rank = np.empty(n, np.int64)
    rank[np.argsort(idk, kind="stable")] = np.arange(n)
    pos_of_rank = np.empty(n, np.int64)
    pos_of_rank[rank[perm]] = np.arange(n)
    S = (n + (1 << log2k) - 1) >> log2k
    split = [0]
    for j in range(1, S):
        lo = j << log2k
        m = min(1 << log2k, n - lo)
        split.append(lo + ((_mix32(d, j) * m) >> 32))
    starts = np.sort(pos_of_rank[np.array(split)])
    assert starts[0] == 0  # the root starts the tour
    return np.diff(np.append(starts, n))


def test_big_random_document_has_sublists_past_255_nodes():
    """(CPU arithmetic on the shared batch: the log2k7 case above stores
    indices that need the slot's second byte)"""
    off, idk, ck, kd, lay, perm, vis, st = _batch("big")
    b, e = int(off[0]), int(off[1])
    assert e - b == BIG
    lens = _sublist_lengths(0, idk[b:e], perm[b:e], 7)
    assert lens.sum() == BIG and lens.max() > 255, lens.max()


@pytest.mark.parametrize("config", ["default", "separate"])
def test_tour_records_repeat_calls_identical(config):
    """A sublist's head slot is read (and discarded) by the previous sublist's
    walker while its own walker overwrites it: the result must not depend on
    which comes first."""
    spec = dataclasses.replace(gen.CONFIG2, seed=47)
    off, idk, ck, kd = gen.generate(spec, 0, 64)
    with abi.Weaver(0, options=CONFIGS[config]) as w:
        a = w.weave_lists(off, idk, ck, kd, spec.layout(), yarns=False)
        b = w.weave_lists(off, idk, ck, kd, spec.layout(), yarns=False)
    assert not a.status.any() and not b.status.any()
    assert np.array_equal(a.weave_perm, b.weave_perm)
    assert np.array_equal(a.visible_bits, b.visible_bits)
