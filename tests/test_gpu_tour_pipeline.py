"""The tour's pipelined handoff loads and its barrier-free sublist ranking
(tour_doc: k_weave_doc and k_tour), bit-exact against the CPU oracle
(run on the MI355X box: -m gpu).

Every document of every batch is compared with oracle.batch_lists(...,
METHOD_EFF): weave order, visibility, visible count and status -- the checks
of tests/test_gpu_parity.py::check_batch, restated here so that one oracle
run per batch serves every context configuration.

Sizes (nodes of a document, the root included): the smallest at which each
piece can go wrong.  The load and the placement take LU * NT = 8 * 1,024
nodes a batch: 8,191 / 8,192 / 8,193 are one full batch and the first node
of a second (and, at the default 8-node splitter
blocks, S = 1,024 = NT sublists and then the first sublist taken from the
LDS counter); 16,384 / 16,385 an even number of batches and the first node
of a third; 20,000 an odd number; below 64 a single wave's partial batch.
65,535 is the largest u16 document: the splitter blocks grow to 32 nodes
there, S = 2,048 (two ranking entries a thread; 50,001-node documents, seven
a thread, are test_gpu_parity's).  Under tour_log2k 7 every S here is < NT
(one entry a thread, most threads none).
"""
import dataclasses

import numpy as np
import pytest

import oracle
from cause_amd import abi, gen, pack

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 8191, 8192, 8193, 16_384, 16_385, 20_000]
BIG = 65_535
CONFIGS = {"default": {}, "separate": {"fused": 0}, "log2k3": {"tour_log2k": 3},
           "log2k4": {"tour_log2k": 4}, "log2k7": {"tour_log2k": 7}}
LAYOUT = pack.KeyLayout(17, 1, 0)  # chain and star: ts | site rank (the root's "0" = 0, one site = 1)


def _tree_doc(n, shape, rng):
    """n nodes with the root, ids 1..n-1 of one site, in shuffled input order.
    chain: every node caused by the one before (one sublist after the other in
    weave order: the sublist list is as long and as ordered as it gets);
    star: every node a child of the root."""
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


def _random_docs(sizes, seed0):
    """config-2 style documents (hides, shows, conjoined runs), one per size"""
    docs = []
    for i, n in enumerate(sizes):
        spec = dataclasses.replace(gen.CONFIG2, nodes_per_doc=n - 1, seed=seed0 + i)
        _, idk, ck, kd = gen.generate(spec, 0, 1)
        docs.append((idk, ck, kd))
    lay = dataclasses.replace(gen.CONFIG2, nodes_per_doc=max(sizes) - 1).layout()
    return _concat(docs), lay


def _make(shape):
    rng = np.random.default_rng(5)
    if shape in ("chain", "star"):
        return _concat([_tree_doc(n, shape, rng) for n in SIZES]), LAYOUT
    if shape == "random":
        return _random_docs(SIZES, 900)
    assert shape == "big"  # every shape at the largest u16 document
    (off, idk, ck, kd), lay = _random_docs([BIG], 950)
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


@pytest.mark.parametrize("shape", ["chain", "star", "random", "big"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_tour_pipeline_vs_oracle(config, shape):
    off, idk, ck, kd, lay, perm, vis, st = _batch(shape)
    assert not st.any(), st
    with abi.Weaver(0, options=CONFIGS[config]) as w:
        res = w.weave_lists(off, idk, ck, kd, lay, yarns=False)
    assert np.array_equal(res.status, st), (res.status, st)
    gvis = res.visible()
    for d in range(len(off) - 1):
        b, e = int(off[d]), int(off[d + 1])
        assert np.array_equal(res.weave_perm[b:e], perm[b:e]), f"doc {d} ({e - b} nodes) order"
        assert np.array_equal(gvis[b:e], vis[b:e]), f"doc {d} ({e - b} nodes) visibility"
        assert int(res.visible_count[d]) == int(vis[b:e].sum()), f"doc {d} ({e - b} nodes) count"


@pytest.mark.parametrize("config", ["default", "separate"])
def test_tour_pipeline_repeat_calls_identical(config):
    """The ranking is asynchronous: the result must not depend on timing."""
    spec = dataclasses.replace(gen.CONFIG2, nodes_per_doc=20_000, seed=31)
    off, idk, ck, kd = gen.generate(spec, 0, 300)
    with abi.Weaver(0, options=CONFIGS[config]) as w:
        a = w.weave_lists(off, idk, ck, kd, spec.layout(), yarns=False)
        b = w.weave_lists(off, idk, ck, kd, spec.layout(), yarns=False)
    assert not a.status.any() and not b.status.any()
    assert np.array_equal(a.weave_perm, b.weave_perm)
    assert np.array_equal(a.visible_bits, b.visible_bits)
