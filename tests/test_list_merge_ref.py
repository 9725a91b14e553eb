"""The host union the GPU list-merge tests trust (tests/listmerge_union.py),
pinned to the restatement of the reference (oracle/causal_ref.py): for seeded
random histories split into two causally closed replicas, the helper's merged
node set and order, woven by refresh_caches over list_weave, is what
merge_trees of the two trees returns -- weave, nodes and yarns.
"""
import random

import numpy as np

from cause_amd import pack
from oracle import causal_ref as R
from tests import refgen as G
from tests.listmerge_union import host_union, sides_of
from tests.test_gpu_merge import closure

N_DOCS = 48


def _ct(nodes, uuid):
    ct = R.new_list_ct(uuid=uuid, rng=random.Random(9))
    ct["nodes"] = {n[0]: (n[1], n[2]) for n in [R.ROOT_NODE] + nodes}
    return R.refresh_caches(R.list_weave, ct)


def _replicas(seed):
    rng = random.Random(seed)
    docs, parts = [], []
    for j in range(N_DOCS):
        nodes, _ = G.random_history(rng, (1, 9, 30, 120)[j % 4])
        mixed = list(nodes)
        rng.shuffle(mixed)
        k = rng.randrange(len(mixed) + 1)
        docs.append(nodes)
        parts.append((closure(nodes, mixed[:k]), closure(nodes, mixed[k:])))
    return docs, parts


def test_host_union_is_merge_trees():
    docs, parts = _replicas(31)
    rng = np.random.default_rng(32)
    b = pack.pack_lists([[R.ROOT_NODE] + nodes for nodes in docs])
    tok = {}
    val = np.array([tok.setdefault(repr(n[2]), len(tok)) for d in b.docs for n in d.nodes], np.uint64)
    # each replica: the root and its nodes, in a random order, as batch indices
    ia, ib = [], []
    for d, (na, nb) in enumerate(parts):
        lo = int(b.offsets[d])
        at = {n[0]: lo + j for j, n in enumerate(b.docs[d].nodes)}
        ia.append(rng.permutation([lo] + [at[n[0]] for n in na]))
        ib.append(rng.permutation([lo] + [at[n[0]] for n in nb]))
    def side(ix):
        off = np.concatenate([[0], np.cumsum([len(x) for x in ix])]).astype(np.uint64)
        cat = np.concatenate(ix).astype(np.int64)
        return (off, b.id_key[cat], b.cause_key[cat], b.kind[cat], val[cat]), cat
    (a, ca), (bb, cb) = side(ia), side(ib)
    src, bits = host_union(a, bb)
    assert not bits.any()
    shared = 0
    for d, (na, nb) in enumerate(parts):
        lo = int(b.offsets[d])
        ct1 = _ct(na, "u" * 21)
        ct2 = _ct(nb, "u" * 21)
        want = R.merge_trees(R.list_weave, ct1, ct2)
        # the helper's merged nodes, in its order
        pick = {0: (ca, int(a[0][d])), 1: (cb, int(bb[0][d]))}
        merged = [b.docs[d].nodes[int(pick[s][0][pick[s][1] + j]) - lo] for s, j in sides_of(src, a, bb)[d]]
        ids = [n[0] for n in merged]
        assert ids == sorted(want["nodes"], key=R.id_key), f"document {d}: merged set or order"
        # of a shared node a's copy is kept
        in_a = {n[0] for n in na} | {R.ROOT_ID}
        assert all((s == 0) == (n[0] in in_a) for (s, _), n in zip(sides_of(src, a, bb)[d], merged))
        shared += len(in_a & {n[0] for n in nb})
        ct = R.new_list_ct(uuid="u" * 21, rng=random.Random(9))
        ct["nodes"] = {n[0]: (n[1], n[2]) for n in merged}
        got = R.refresh_caches(R.list_weave, ct)
        assert got["weave"] == want["weave"], f"document {d}: weave"
        assert got["nodes"] == want["nodes"], f"document {d}: nodes"
        assert got["yarns"] == want["yarns"], f"document {d}: yarns"
    assert shared > N_DOCS  # the closures overlap: equal ids were really united


def test_host_union_flags_changed_bodies_and_keeps_the_first_copy():
    """Three copies of one id (two inside a): the smallest source index is kept;
    a body that differs in cause, kind or value token is a DUP."""
    off = lambda *n: np.array((0,) + n, np.uint64)
    u64, u8 = (lambda *x: np.array(x, np.uint64)), (lambda *x: np.array(x, np.uint8))
    a = (off(3), u64(5, 0, 5), u64(0, 2**64 - 1, 0), u8(0, 4, 0), u64(7, 0, 7))
    for k, changed in ((2, u64(1)), (3, u8(1)), (4, u64(8)), (None, None)):
        b = [off(1), u64(5), u64(0), u8(0), u64(7)]
        if k:
            b[k] = changed
        src, bits = host_union(a, tuple(b))
        assert [list(s) for s in src] == [[1, 0]]
        assert bits[0] == (2 if k else 0)
