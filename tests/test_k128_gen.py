"""tests/k128_gen.py proved on the CPU: what tests/test_gpu_k128_shapes.py
expects of the GPU comes from the oracle on a K64 batch and from the widening
maps, so the maps must keep the order and the equalities of the ids, carry the
word edges they are named for, and agree with the tuple route
(pack_lists_k128 + renumber + METHOD_LITERAL) that tests/test_gpu_k128.py
already trusts.  No GPU work here."""
import random

import numpy as np
import pytest

import oracle
from cause_amd import abi, pack
from oracle import causal_ref as R
from tests import k128_gen as K
from tests import refgen as G
from tests.test_gpu_k128 import expected_yarns, renumber

CASES = [(name, wd) for name, (_, wds, _) in K.BATCHES.items() for wd in wds]
TOP63, M32 = K.TOP63, K.M32
BIT63 = np.uint64(1 << 63)


@pytest.mark.parametrize("name,widening", CASES)
def test_widening_keeps_ranks_and_causes(name, widening):
    """Per document: the rank of every id under np.lexsort((lo, hi)) is its rank
    among the K64 ids, and every wide cause names the id its K64 cause names
    (or none, or nil)."""
    w = K.wide(name, widening)
    b = w.k64
    assert w.id2.shape == (len(b.idk), 2) and w.ca2.shape == w.id2.shape
    for d in range(b.D):
        lo, hi = b.span(d)
        rid64, rc64 = K.ranks_k64(b, d)
        rid128, rc128 = K.ranks_k128(w, d)
        assert np.array_equal(rid64, rid128), f"{name}/{widening} doc {d}: id ranks"
        assert np.array_equal(rc64, rc128), f"{name}/{widening} doc {d}: cause ranks"
        # ... and the ranks are what a plain lexsort of the two words gives
        i2 = w.id2[lo:hi]
        order = np.lexsort((i2[:, 1], i2[:, 0]))
        if d not in w.dup_docs:
            assert np.array_equal(rid128[order], np.arange(hi - lo))
            assert np.array_equal(np.argsort(b.idk[lo:hi], kind="stable"), order)
        # nil is nil on both sides, and nothing else is
        nil128 = (w.ca2[lo:hi] == K.NIL).all(axis=1)
        assert np.array_equal(nil128, b.ck[lo:hi] == K.NIL)
        if hi > lo:
            assert int(w.max_ts[d]) == int(i2[:, 0].max())
    sizes = np.diff(b.off.astype(np.int64))
    assert (w.max_ts[sizes == 0] == 0).all()


def test_batches_have_the_sizes_they_are_named_for():
    T = K.TILE
    assert list(np.diff(K.wide("edges", "top").off.astype(np.int64))) == \
        [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 20_000]
    for name in ("shapes", "shapes_one_ts"):
        assert list(np.diff(K.wide(name, K.BATCHES[name][1][0]).off.astype(np.int64))) == [T - 1, T + 1] * 3
    assert int(K.wide("n65535", "top").off[-1]) == (1 << 16) - 1  # below OS_MIN_KEYS and giant_min
    assert int(K.wide("n65536", "top").off[-1]) == 1 << 16
    assert list(np.diff(K.wide("several", "sparse").off.astype(np.int64))) == [70_001, 3_000, 0, 66_000]
    assert list(np.diff(K.wide("causes", "top").off.astype(np.int64))) == [9_000] * 9


@pytest.mark.parametrize("name", ["edges", "n65535", "n65536", "n5000", "causes", "shapes"])
def test_top_reaches_the_top_of_both_words(name):
    w = K.wide(name, "top")
    hi, lo = w.id2[:, 0], w.id2[:, 1]
    assert int(hi.max()) == TOP63                       # hi_bits = 63
    assert int(hi.min()) == 0                           # the root: every bit below decides
    assert int(lo.max() >> np.uint64(32)) == M32        # the largest site rank
    assert (lo & BIT63).any() and not (lo & BIT63).all()
    assert int(w.max_ts.max()) == TOP63


def test_top_scales_tx_to_32_bits():
    """A layout with tx-indices (the hand-built one-ts shapes have them): top's
    h sends the largest to 2^32 - 1."""
    w = K.widen(K.wide("shapes_one_ts", "lo_only").k64, "top")
    assert int((w.id2[:, 1] & np.uint64(M32)).max()) > M32 - 4096
    assert int(w.id2[:, 0].max()) == TOP63


def test_hi_only_has_an_all_zero_lo_column():
    w = K.wide("edges", "hi_only")
    assert not w.id2[:, 1].any()                        # find_key_bits(lo) = 1
    isid = ~(w.ca2 == K.NIL).all(axis=1)
    assert not w.ca2[isid, 1].any()
    assert int(w.id2[:, 0].max()) > TOP63 // 2          # bit 62 of hi in use
    assert (w.yarn_shift, w.yarn_mask) == (0, 0)        # one site: the yarn is the id order
    for d in range(w.k64.D):
        lo, hi = w.k64.span(d)
        assert len(np.unique(w.id2[lo:hi, 0])) == hi - lo   # hi alone decides


def test_lo_only_is_decided_by_lo_alone():
    w = K.wide("shapes_one_ts", "lo_only")
    b = w.k64
    for d in range(b.D):
        lo, hi = b.span(d)
        nonroot = (b.kd[lo:hi] & pack.KIND_ROOT) == 0
        assert len(np.unique(w.id2[lo:hi, 0][nonroot])) == 1    # one distinct hi
        assert int(w.id2[lo:hi, 0][nonroot][0]) == TOP63
        los = set(int(x) for x in w.id2[lo:hi, 1][nonroot])
        assert len(los) == int(nonroot.sum())
        assert any(x ^ (1 << 63) in los for x in los), f"doc {d}: no pair differing in lo bit 63 alone"
        assert any(x ^ 1 in los for x in los), f"doc {d}: no pair differing in lo bit 0 alone"
        assert max(los) >> 32 == M32


def test_sparse_uses_the_full_ranges():
    for name in ("edges", "several"):
        w = K.wide(name, "sparse")
        hi, lo = w.id2[:, 0], w.id2[:, 1]
        assert int(hi.max()) > TOP63 // 4 and int(hi.max()) <= TOP63
        assert int(lo.max() >> np.uint64(32)) > M32 // 4
        assert (lo & np.uint64(M32)).any()              # the low half of lo in use as well
        assert len(np.unique(hi >> np.uint64(52))) > 16  # not a shifted copy of the small ts


def test_corruptions_give_the_status_they_claim():
    w = K.wide("causes", "top")
    e = K.expected("causes")
    assert [w.claims.get(d, (None, 0))[0] for d in range(w.k64.D)] == list(K.CAUSE_PLAN)
    for d in range(w.k64.D):
        what, bits = w.claims.get(d, (None, 0))
        assert int(e.st[d]) == bits, f"doc {d} ({what}): status {int(e.st[d])}, claimed {bits}"
    # only the documents given a repeated id are DUP; the flagged share is 8 of 9
    assert frozenset(np.nonzero(e.st & abi.STATUS_DUP)[0].tolist()) == w.dup_docs == frozenset({7})
    assert int((e.st != 0).sum()) == len(K.CORRUPTIONS) == 8 and e.st[8] == 0
    # the same bits from the oracle's general fold
    _, _, st3 = oracle.batch_lists(w.k64.off, w.k64.idk, w.k64.ck, w.k64.kd,
                                   method=oracle.METHOD_GENERAL)
    assert np.array_equal(st3, e.st)


def test_corrupted_words_are_what_they_are_named_for():
    w = K.wide("causes", "top")
    clean = K.widen(K.random_docs((K.CAUSE_NODES,) * len(K.CAUSE_PLAN), 2400), "top", seed=len("causes"))
    for d, what in enumerate(K.CAUSE_PLAN):
        lo, hi = w.k64.span(d)
        i2, c2 = w.id2[lo:hi], w.ca2[lo:hi]
        ch = np.nonzero((c2 != clean.ca2[lo:hi]).any(axis=1) | (i2 != clean.id2[lo:hi]).any(axis=1))[0]
        if what is None:
            assert len(ch) == 0
            continue
        assert len(ch) == 1, f"doc {d} ({what}): one node changed"
        c = c2[ch[0]]
        his, los = set(i2[:, 0].tolist()), set(i2[:, 1].tolist())
        ids = set(map(tuple, i2.tolist()))
        if what == "hi_hit_lo_miss":
            assert int(c[0]) in his and tuple(c.tolist()) not in ids
        elif what == "lo_hit_hi_miss":
            assert int(c[1]) in los and int(c[0]) not in his
        elif what == "above_all":
            assert (int(c[0]), int(c[1])) > max(ids)
        elif what == "nil_hi":
            assert int(c[0]) == pack.NIL and int(c[1]) != pack.NIL and int(c[1]) in los
        elif what == "non_id":
            assert tuple(c.tolist()) == pack.NON_ID_CAUSE2
        elif what == "nil_cause":
            assert tuple(c.tolist()) == pack.NIL2 and not w.kd[lo + ch[0]] & pack.KIND_ROOT
        elif what == "younger":
            assert tuple(c.tolist()) in ids and tuple(c.tolist()) > tuple(i2[ch[0]].tolist())
        elif what == "dup":
            order = np.lexsort((i2[:, 1], i2[:, 0]))
            a, b = i2[order[K.TILE - 1]], i2[order[K.TILE]]
            assert np.array_equal(a, b)                 # the equal run straddles position TILE
            assert len(ids) == hi - lo - 1


def _small_docs():
    rng = random.Random(77)
    docs = []
    for steps in (1, 2, 5, 20, 60, 150):
        for _ in range(4):
            nodes, _ = G.random_history(rng, steps)
            d = [R.ROOT_NODE] + nodes
            rng.shuffle(d)
            docs.append(d)
    for case in G.EDGE_CASES:
        docs.append([R.ROOT_NODE] + list(case))
    docs += [[], [R.ROOT_NODE]]
    return docs


@pytest.mark.parametrize("widening", ["top", "sparse", "hi_only"])
def test_agrees_with_the_tuple_route(widening):
    """Small documents: the widened words read back as Clojure-shaped nodes
    ([hi site tx]) and sent down the tuple route give what this module expects."""
    b = K.from_tuples(_small_docs())
    w = K.widen(b, widening, seed=3)
    e = K.expect(w.k64, oracle.METHOD_LITERAL)
    docs = K.to_tuples(w)
    # the tuple route packs the same documents (its site ranks are dense, ours are not)
    p = pack.pack_lists_k128(docs)
    assert np.array_equal(p.offsets, b.off) and np.array_equal(p.kind, b.kd)
    nr = (b.kd & pack.KIND_ROOT) == 0  # (the root reads back as [0 "0" 0])
    assert np.array_equal(p.id_key[nr, 0], w.id2[nr, 0])
    assert np.array_equal(p.id_key[nr, 1] & np.uint64(M32), w.id2[nr, 1] & np.uint64(M32))
    off, idk, ck, kd = renumber(docs)
    perm, vis, st = oracle.batch_lists(off, idk, ck, kd, method=oracle.METHOD_LITERAL)
    assert np.array_equal(st, e.st) and np.array_equal(perm, e.perm) and np.array_equal(vis, e.vis)
    want_y = K.yarns_of(e, w)
    for d, nodes in enumerate(docs):
        lo, hi = b.span(d)
        if nodes:
            assert int(w.max_ts[d]) == max(n[0][0] for n in nodes)
            assert np.array_equal(want_y[lo:hi], expected_yarns(nodes)), f"doc {d} yarns"


def test_one_ts_tuple_route():
    """lo_only on small documents of one ts, against the tuple route."""
    from tests.test_gpu_tree_sweep2 import chain, comb, star

    docs = [K.one_ts(shape(n)) for shape in (chain, star, comb) for n in (2, 5, 33)]
    b = K.from_tuples(docs)
    w = K.widen(b, "lo_only")
    e = K.expect(w.k64, oracle.METHOD_LITERAL)
    assert not e.st.any()
    tup = K.to_tuples(w)
    off, idk, ck, kd = renumber(tup)
    perm, vis, st = oracle.batch_lists(off, idk, ck, kd, method=oracle.METHOD_LITERAL)
    assert np.array_equal(st, e.st) and np.array_equal(perm, e.perm) and np.array_equal(vis, e.vis)
    want_y = K.yarns_of(e, w)
    for d, nodes in enumerate(tup):
        lo, hi = b.span(d)
        assert np.array_equal(want_y[lo:hi], expected_yarns(nodes))


def test_in_domain_batches_are_in_domain():
    """EFF is the oracle's rule inside the domain only: no status bit there, and
    the literal fold agrees on the multi-tile batch."""
    for name, (_, wds, method) in K.BATCHES.items():
        if method == oracle.METHOD_EFF:
            e = K.expected(name)
            sizes = np.diff(K.wide(name, wds[0]).off.astype(np.int64))
            assert np.array_equal(e.st != 0, sizes == 0), name   # an empty document has no root
    b = K.wide("shapes_one_ts", "lo_only").k64
    e = K.expected("shapes_one_ts")
    perm, vis, st = oracle.batch_lists(b.off, b.idk, b.ck, b.kd, method=oracle.METHOD_LITERAL)
    assert np.array_equal(perm, e.perm) and np.array_equal(vis, e.vis) and np.array_equal(st, e.st)
