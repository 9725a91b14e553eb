"""cw_merge_lists on the GPU: the fused union kernel (k_list_union), the general
route, device memory and async contexts (-m gpu).

Every merge is checked against a host reading of the union
(tests/listmerge_union.py: merged source indices in id order, the smallest
source index kept, DUP bits; pinned to the restatement by
test_list_merge_ref.py) and against the C oracle's weave of that union
(oracle.batch_lists, METHOD_EFF).  The weaver is parametrised over the fused
kernel and the general route; the two must return identical arrays.
"""
import ctypes as C
import dataclasses
import random

import numpy as np
import pytest

import oracle
from cause_amd import abi, gen, pack
from oracle import causal_ref as R
from tests import refgen as G
from tests.listmerge_union import host_union, merged_offsets, union_arrays
from tests.test_gpu_merge import split_batch

pytestmark = pytest.mark.gpu

LAYOUT = pack.KeyLayout(16, 4, 0)  # gen.CONFIG2's documents of up to 65,536 nodes
FIELDS = ("weave_perm", "visible_bits", "visible_count", "status", "max_ts", "yarn_perm")
DIR_END = 245_760  # ids from here on lie past the rank directory of the fused route


@pytest.fixture(scope="module", params=[1, 0], ids=["fused", "general"])
def weaver(request):
    w = abi.Weaver(0, options={"list_merge_fused": request.param})
    w.fused = bool(request.param)
    yield w
    w.close()


@pytest.fixture(scope="module")
def both():
    wf = abi.Weaver(0, options={"list_merge_fused": 1})
    wg = abi.Weaver(0, options={"list_merge_fused": 0})
    yield wf, wg
    wf.close()
    wg.close()


# ------------------------------------------------------------------ helpers
def docs_of(sizes, seed=0, n_sites=None):
    """A list batch whose documents have exactly these sizes (root included):
    gen.CONFIG2 with nodes_per_doc replaced; 1 = the root alone, 0 = empty."""
    off, cols = [0], ([], [], [])
    for d, n in enumerate(sizes):
        if n == 1:
            part = (np.zeros(1, np.uint64), np.full(1, pack.NIL, np.uint64),
                    np.full(1, pack.KIND_ROOT, np.uint8))
        elif n:
            spec = dataclasses.replace(gen.CONFIG2, nodes_per_doc=n - 1, seed=gen.CONFIG2.seed + seed + d,
                                       **({"n_sites": n_sites} if n_sites else {}))
            part = gen.generate(spec, 0, 1, nthreads=1)[1:]
        else:
            part = (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8))
        for c, p in zip(cols, part):
            c.append(p)
        off.append(off[-1] + n)
    return (np.array(off, np.uint64),) + tuple(np.concatenate(c) for c in cols)


def split_at(off, idk, ck, kd, rng, na):
    """Disjoint replicas: a random na[d] nodes of document d to a, the rest to b."""
    ia, ib, oa, ob = [], [], [0], [0]
    for d in range(len(off) - 1):
        p = int(off[d]) + rng.permutation(int(off[d + 1]) - int(off[d]))
        ia.append(p[:na[d]])
        ib.append(p[na[d]:])
        oa.append(oa[-1] + len(ia[-1]))
        ob.append(ob[-1] + len(ib[-1]))
    ia, ib = np.concatenate(ia).astype(np.int64), np.concatenate(ib).astype(np.int64)
    side = lambda o, ix: (np.array(o, np.uint64), idk[ix], ck[ix], kd[ix], ix.astype(np.uint64))
    return side(oa, ia), side(ob, ib)


def check(weaver, a, b, layout, oracle_too=True):
    """One merge against the host union and the oracle's weave of the union."""
    res = weaver.merge_lists(a, b, layout)
    src, bits = host_union(a, b)
    moff = merged_offsets(src)
    np.testing.assert_array_equal(res.offsets, moff)
    np.testing.assert_array_equal(res.src, np.concatenate(src) if src else np.zeros(0, np.uint32))
    np.testing.assert_array_equal(res.weave.status & abi.STATUS_DUP, bits)
    empty = np.diff(moff.astype(np.int64)) == 0
    np.testing.assert_array_equal((res.weave.status & abi.STATUS_ROOT != 0)[empty], True)
    if oracle_too:
        uoff, uid, uc, uk = union_arrays(src, a, b)
        perm, vis, st = oracle.batch_lists(uoff, uid, uc, uk, method=oracle.METHOD_EFF)
        np.testing.assert_array_equal(res.weave.status, st | bits)
        gvis = res.weave.visible()
        for d in np.flatnonzero(st == 0):
            lo, hi = int(moff[d]), int(moff[d + 1])
            np.testing.assert_array_equal(res.weave.weave_perm[lo:hi], perm[lo:hi], err_msg=f"document {d}")
            np.testing.assert_array_equal(gvis[lo:hi], vis[lo:hi], err_msg=f"document {d}")
            assert res.weave.visible_count[d] == int(vis[lo:hi].sum())
    return res


def same(x, y):
    np.testing.assert_array_equal(x.offsets, y.offsets)
    np.testing.assert_array_equal(x.src, y.src)
    full = np.diff(x.offsets.astype(np.int64)) > 0  # (max_ts of an empty document is not written)
    for f in FIELDS:
        u, v = getattr(x.weave, f), getattr(y.weave, f)
        np.testing.assert_array_equal(u[full] if f == "max_ts" else u, v[full] if f == "max_ts" else v, err_msg=f)


def routes(weaver, call):
    """Kernel stat names of one merge call (the sort's passes, m_idsort_hist
    and so on, under the sort's name)."""
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        call()
        return {"m_idsort" if n.startswith("m_idsort") else n for n in weaver.kernel_stats()}
    finally:
        weaver.set_profiling(False)
        weaver.reset_kernel_stats()


SIZES = [1, 2, 63, 64, 65, 95, 96, 97, 1023, 1024, 1025, 4000]


@pytest.fixture(scope="module")
def sizes_batch():
    return docs_of(SIZES)


@pytest.fixture(scope="module")
def sizes_split(sizes_batch):
    (a, _), (b, _) = split_batch(*sizes_batch, np.random.default_rng(3), overlap=0.2)
    return a, b


def mk(docs, layout):
    """Hand-made sides.  docs[d] = (a_nodes, b_nodes), a node = (ts, site, cause,
    kind, value token) with cause None (nil) or (ts, site)."""
    def side(k):
        off, idk, ck, kd, val = [0], [], [], [], []
        for doc in docs:
            for ts, site, cause, kind, v in doc[k]:
                idk.append(layout.pack(ts, site, 0))
                ck.append(pack.NIL if cause is None else layout.pack(cause[0], cause[1], 0))
                kd.append(kind)
                val.append(v)
            off.append(len(idk))
        return (np.array(off, np.uint64), np.array(idk, np.uint64), np.array(ck, np.uint64),
                np.array(kd, np.uint8), np.array(val, np.uint64))
    return side(0), side(1)


ROOT = (0, 0, None, pack.KIND_ROOT, 0)
X1 = (1, 1, (0, 0), 0, 1)
Y2 = (2, 1, (1, 1), 0, 3)


X1B = (1, 1, (0, 0), 0, 2)                # X1's id with another value token
CLEAN = ([ROOT, X1], [X1, Y2])
SMALL = pack.KeyLayout(4, 2, 0)


def status_batch():
    """Ids repeated across the sides only: the fused kernel keeps the call."""
    x1b, clean = X1B, CLEAN
    orphan = (3, 1, (9, 2), 0, 4)
    docs = [
        ([ROOT, X1], [x1b]),              # 0: DUP (test_merge_conflict_and_orphan_status)
        ([ROOT, X1], [Y2, orphan]),       # 1: ORPHAN
        clean,                            # 2
        ([], []),                         # 3: empty
        ([ROOT, X1, Y2], [(2, 1, (0, 0), 0, 3)]),   # 4: only the cause differs
        clean,
        ([ROOT, X1], [(1, 1, (0, 0), 1, 1)]),       # 6: only the kind differs
        clean,
        ([ROOT, X1], [(1, 1, (0, 0), 0, 9)]),       # 8: only the value token differs
        clean,
    ]
    return mk(docs, SMALL), SMALL


def repeat_batch():
    """An id repeated inside one side: the fused kernel hands the call over."""
    docs = [
        CLEAN,
        ([ROOT, X1, X1], [Y2]),           # 1: repeated inside a, same body
        ([ROOT], [X1, X1B]),              # 2: repeated inside b, another body
        CLEAN,
    ]
    return mk(docs, SMALL), SMALL


def one_changed_body(a, b, d, field):
    """b with the body field (2 cause, 3 kind, 4 value token) of one node of
    document d changed: a node whose id a holds too."""
    a0, a1, b0, b1 = int(a[0][d]), int(a[0][d + 1]), int(b[0][d]), int(b[0][d + 1])
    shared = np.flatnonzero(np.isin(b[1][b0:b1], a[1][a0:a1]) & (b[3][b0:b1] == 0))
    j = b0 + int(shared[len(shared) // 2])
    out = [x.copy() for x in b]
    out[field][j] = out[field][j] + 1 if field != 3 else 1
    return tuple(out)


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("overlap", [0.0, 0.2, 1.0])
def test_sizes_and_overlaps(weaver, sizes_batch, overlap):
    (a, _), (b, _) = split_batch(*sizes_batch, np.random.default_rng(int(overlap * 10)), overlap=overlap)
    res = check(weaver, a, b, LAYOUT)
    assert not res.weave.status.any()
    np.testing.assert_array_equal(np.diff(res.offsets), SIZES)  # the union is the document
    if overlap == 1.0:  # of a shared node a's copy is kept
        na = np.diff(a[0].astype(np.int64))
        assert np.all(res.src < np.repeat(na, np.diff(res.offsets.astype(np.int64))))


def test_reference_histories(weaver):
    rng = random.Random(5)
    docs = []
    for steps in (1, 9, 30, 120):
        for _ in range(5):
            nodes, _ = G.random_history(rng, steps)
            docs.append([R.ROOT_NODE] + nodes)
    p = pack.pack_lists(docs)
    (a, _), (b, _) = split_batch(p.offsets, p.id_key, p.cause_key, p.kind, np.random.default_rng(6))
    res = check(weaver, a, b, p.layout)
    assert not res.weave.status.any()


def test_largest_fused_document(weaver):
    """na + nb = 65,535 (32,768 + 32,767, disjoint) next to small documents: three
    sites keep its ids inside the directory, so the fused kernel takes it."""
    off, idk, ck, kd = docs_of([65_535, 97, 4000], seed=7, n_sites=3)
    assert int(idk.max()) < DIR_END - 8 * 96
    a, b = split_at(off, idk, ck, kd, np.random.default_rng(7), [32_768, 50, 1])
    lay = pack.KeyLayout(16, 2, 0)
    assert int(a[0][1]) + int(b[0][1]) == 65_535
    res = check(weaver, a, b, lay)
    assert not res.weave.status.any()
    names = routes(weaver, lambda: weaver.merge_lists(a, b, lay))
    assert ("list_union" in names) == weaver.fused and ("merge_concat" in names) != weaver.fused


def test_one_node_more_takes_the_general_route(weaver):
    off, idk, ck, kd = docs_of([65_536, 97], seed=8, n_sites=3)
    a, b = split_at(off, idk, ck, kd, np.random.default_rng(8), [32_768, 50])
    lay = pack.KeyLayout(16, 2, 0)
    assert int(a[0][1]) + int(b[0][1]) == 65_536
    res = check(weaver, a, b, lay)
    assert not res.weave.status.any()
    names = routes(weaver, lambda: weaver.merge_lists(a, b, lay))
    assert "list_union" not in names and {"merge_concat", "m_idsort"} <= names


# ------------------------------------------------------------------ 2. route taken
def test_route_taken(weaver, sizes_split):
    a, b = sizes_split
    names = routes(weaver, lambda: weaver.merge_lists(a, b, LAYOUT))
    general = {"merge_concat", "m_idsort", "merge_count", "merge_write"}
    if weaver.fused:
        assert "list_union" in names and not names & general
    else:
        assert "list_union" not in names and general <= names


# ------------------------------------------------------------------ 3. empty sides
def test_empty_sides(weaver):
    off, idk, ck, kd = docs_of([300, 300, 0, 300, 64], seed=20)
    na = [0, 300, 0, 120, 64]  # a empty, b empty, both empty, neither, b empty
    a, b = split_at(off, idk, ck, kd, np.random.default_rng(20), na)
    res = check(weaver, a, b, LAYOUT)
    assert list(res.weave.status) == [0, 0, abi.STATUS_ROOT, 0, 0]


def test_whole_batch_empty_and_one_document(weaver):
    z = lambda dt: np.zeros(0, dt)
    e = (np.zeros(4, np.uint64), z(np.uint64), z(np.uint64), z(np.uint8), z(np.uint64))
    res = weaver.merge_lists(e, e, LAYOUT)
    assert list(res.offsets) == [0, 0, 0, 0] and list(res.weave.status) == [abi.STATUS_ROOT] * 3
    assert not res.weave.visible_count.any()
    off, idk, ck, kd = docs_of([1500], seed=21)
    (a, _), (b, _) = split_batch(off, idk, ck, kd, np.random.default_rng(21))
    res = check(weaver, a, b, LAYOUT)
    assert list(res.weave.status) == [0]


# ------------------------------------------------------------------ 4. status
GENERAL = {"merge_concat", "m_idsort", "merge_count", "merge_write"}


def test_status_bits_across_sides(weaver, both):
    """Ids repeated across the sides, differing only in cause, only in kind and
    only in value token, with clean neighbours, an orphan and an empty
    document: the fused kernel's own body compare (no fallback)."""
    (a, b), lay = status_batch()
    names = routes(weaver, lambda: weaver.merge_lists(a, b, lay))
    if weaver.fused:
        assert "list_union" in names and not names & GENERAL
    res = check(weaver, a, b, lay)
    st = res.weave.status
    assert all(st[d] == abi.STATUS_DUP for d in (0, 4, 6, 8))
    assert st[1] & abi.STATUS_ORPHAN and not st[1] & abi.STATUS_DUP and st[3] == abi.STATUS_ROOT
    assert not st[[2, 5, 7, 9]].any()
    assert list(np.diff(res.offsets)) == [2, 4, 3, 0, 3, 3, 2, 3, 2, 3]
    same(res, both[1].merge_lists(a, b, lay))  # the general route's arrays


@pytest.mark.parametrize("field", [2, 3, 4], ids=["cause", "kind", "value"])
def test_one_changed_body_among_many_shared_nodes(weaver, both, sizes_split, field):
    """Hundreds of equal ids with equal bodies and one with another body, in two
    documents: DUP there and nowhere else, by the fused kernel."""
    a, b = sizes_split
    for d in (8, 11):
        b = one_changed_body(a, b, d, field)
    names = routes(weaver, lambda: weaver.merge_lists(a, b, LAYOUT))
    if weaver.fused:
        assert "list_union" in names and not names & GENERAL
    res = weaver.merge_lists(a, b, LAYOUT)
    src, bits = host_union(a, b)
    assert list(np.flatnonzero(bits)) == [8, 11]
    np.testing.assert_array_equal(res.src, np.concatenate(src))
    np.testing.assert_array_equal(res.weave.status, bits)
    same(res, both[1].merge_lists(a, b, LAYOUT))


def test_id_repeated_inside_one_side(weaver, both):
    """Kept once, the smallest source index; another body is a DUP.  The fused
    kernel notices the repeat and the general route takes the call."""
    (a, b), lay = repeat_batch()
    names = routes(weaver, lambda: weaver.merge_lists(a, b, lay))
    assert GENERAL <= names and ("list_union" in names) == weaver.fused
    res = check(weaver, a, b, lay)
    assert list(res.weave.status) == [0, 0, abi.STATUS_DUP, 0]
    assert list(np.diff(res.offsets)) == [3, 3, 2, 3]
    lo = int(res.offsets[1])
    assert list(res.src[lo:lo + 3]) == [0, 1, 3]
    same(res, both[1].merge_lists(a, b, lay))


# ------------------------------------------------------------------ 5. fallbacks
def sparse_batch():
    """Document 1 has Lamport timestamps 3,000 apart: its largest packed id lies
    past the directory.  Document 3 holds a key >= 2^63."""
    lay = pack.KeyLayout(60, 4, 0)
    chain = [ROOT] + [(3000 * k, 1 + k % 3, (3000 * (k - 1), 1 + (k - 1) % 3) if k > 1 else (0, 0), 0, k)
                      for k in range(1, 8)]
    assert lay.pack(*chain[-1][:2], 0) >= DIR_END
    wide = [ROOT, X1, (1 << 59, 1, (1, 1), 0, 5)]
    assert lay.pack(1 << 59, 1, 0) >= 1 << 63 and lay.key_bits == 64
    docs = [([ROOT, X1], [X1, Y2]), (chain[:5], chain[3:]), ([ROOT, X1, Y2], [Y2]), (wide[:2], wide[1:]),
            ([ROOT], [X1, Y2])]
    return mk(docs, lay), lay


@pytest.mark.parametrize("which", ["sparse", "key_range"])
def test_fallbacks_keep_the_result(both, which):
    (a, b), lay = sparse_batch()
    keep = [0, 1, 2, 4] if which == "sparse" else [0, 2, 3, 4]
    def sub(t):
        off = t[0].astype(np.int64)
        ix = np.concatenate([np.arange(off[d], off[d + 1]) for d in keep])
        o = np.concatenate([[0], np.cumsum([off[d + 1] - off[d] for d in keep])]).astype(np.uint64)
        return (o,) + tuple(x[ix] for x in t[1:])
    a, b = sub(a), sub(b)
    wf, wg = both
    x, y = wf.merge_lists(a, b, lay), wg.merge_lists(a, b, lay)
    same(x, y)
    src, bits = host_union(a, b)
    np.testing.assert_array_equal(x.src, np.concatenate(src))
    if which == "key_range":
        assert x.weave.status[2] & abi.STATUS_KEY_RANGE and not x.weave.status[[0, 1, 3]].any()
    else:
        assert not x.weave.status.any()
    # the fused kernel ran, gave up, and the general route took the call
    names = routes(wf, lambda: wf.merge_lists(a, b, lay))
    assert {"list_union", "merge_concat", "m_idsort"} <= names


# ------------------------------------------------------------------ 6. both routes
def test_both_routes_give_identical_arrays(both, sizes_split):
    wf, wg = both
    a, b = sizes_split
    same(wf.merge_lists(a, b, LAYOUT), wg.merge_lists(a, b, LAYOUT))
    for (a, b), lay in (status_batch(), repeat_batch()):
        same(wf.merge_lists(a, b, lay), wg.merge_lists(a, b, lay))


# ------------------------------------------------------------------ 7. device memory
def device_call(weaver, a, b, layout, want):
    import torch

    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    ga, gb = [up(x) for x in a[1:]], [up(x) for x in b[1:]]
    NC, D = len(a[1]) + len(b[1]), len(a[0]) - 1
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    o = {"weave_perm": z(NC, torch.int32), "visible_bits": z((NC + 31) // 32 + 1, torch.int32),
         "visible_count": z(D, torch.int32), "max_ts": z(D, torch.int64), "status": z(D, torch.int32),
         "yarn_perm": z(NC, torch.int32)}
    o = {k: v for k, v in o.items() if k in want}
    src = z(NC, torch.int32)
    ptr = lambda xs: [x.data_ptr() if x.numel() else 0 for x in xs]
    mo = weaver.merge_lists_device(a[0], ptr(ga), b[0], ptr(gb), layout, src.data_ptr(),
                                   {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    view = lambda t: t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32)
    return mo, view(src), {k: view(v) for k, v in o.items()}


def check_device(weaver, a, b, layout, want):
    host = weaver.merge_lists(a, b, layout)
    mo, src, o = device_call(weaver, a, b, layout, want)
    M, D = int(mo[-1]), len(a[0]) - 1
    np.testing.assert_array_equal(mo, host.offsets)
    np.testing.assert_array_equal(src[:M], host.src)
    size = {"weave_perm": M, "yarn_perm": M, "visible_bits": (M + 31) // 32}
    for k, v in o.items():
        np.testing.assert_array_equal(v[:size.get(k, D)], getattr(host.weave, k), err_msg=k)


@pytest.mark.parametrize("is_async", [False, True], ids=["sync", "async"])
def test_device_memory_call_matches_host(weaver, sizes_split, is_async):
    a, b = sizes_split
    weaver.set_async(is_async)
    try:
        check_device(weaver, a, b, LAYOUT, FIELDS)
        check_device(weaver, a, b, LAYOUT, ("weave_perm", "visible_count", "status"))
        (sa, sb), lay = status_batch()  # DUP, ORPHAN and the ROOT of an empty document, on the device
        small = ("weave_perm", "visible_bits", "visible_count", "status", "yarn_perm")
        names = routes(weaver, lambda: device_call(weaver, sa, sb, lay, small))
        assert ("list_union" in names and not names & GENERAL) if weaver.fused else GENERAL <= names
        check_device(weaver, sa, sb, lay, small)
        (ra, rb), lay = repeat_batch()  # the fallback in device memory
        check_device(weaver, ra, rb, lay, small)
    finally:
        weaver.set_async(False)


def test_device_memory_empty_batch(weaver):
    z = lambda dt: np.zeros(0, dt)
    e = (np.zeros(3, np.uint64), z(np.uint64), z(np.uint64), z(np.uint8), z(np.uint64))
    mo, _, o = device_call(weaver, e, e, LAYOUT, ("weave_perm", "visible_count", "status", "max_ts"))
    assert list(mo) == [0, 0, 0] and list(o["status"]) == [abi.STATUS_ROOT] * 2
    assert not o["visible_count"].any() and not o["max_ts"].any()


# ------------------------------------------------------------------ 8. repeated calls
def test_repeated_and_alternating_calls(weaver, sizes_split):
    """The look-back words carry an epoch and are not cleared between calls, and
    the uploaded layouts are cached: the same batch three times, then a batch
    with another document count, then the first again."""
    a, b = sizes_split
    first = weaver.merge_lists(a, b, LAYOUT)
    for _ in range(2):
        same(weaver.merge_lists(a, b, LAYOUT), first)
    off, idk, ck, kd = docs_of([500] * 40 + [97, 1], seed=30)
    (oa, _), (ob, _) = split_batch(off, idk, ck, kd, np.random.default_rng(30))
    other = check(weaver, oa, ob, LAYOUT)
    same(weaver.merge_lists(a, b, LAYOUT), first)
    same(weaver.merge_lists(oa, ob, LAYOUT), other)


# ------------------------------------------------------------------ 9. look-back windows
def tiny_docs(D, empty_every=0):
    """D documents of 2 to 5 nodes, 1 to 3 of them a side; every empty_every-th
    document empty on both sides."""
    sizes = [0 if empty_every and d % empty_every == empty_every - 1 else 2 + d % 4 for d in range(D)]
    (a, _), (b, _) = split_batch(*docs_of(sizes, seed=50), np.random.default_rng(D), overlap=0.2)
    na, nb = np.diff(a[0].astype(np.int64)), np.diff(b[0].astype(np.int64))
    full = np.array(sizes) > 0
    assert ((na[full] >= 1) & (na[full] <= 3) & (nb[full] >= 1) & (nb[full] <= 3)).all()
    assert not na[~full].any() and not nb[~full].any()
    return a, b


@pytest.mark.parametrize("D", [64, 65, 66, 128, 129, 130, 200])
def test_document_counts_around_the_look_back_window(weaver, D):
    """k_list_union sums its predecessors' merged counts 64 words at a time: a
    document with 64 or 128 predecessors ends its look-back exactly on a window's
    boundary, one with 65 or 129 reads a window of one word."""
    a, b = tiny_docs(D)
    res = check(weaver, a, b, LAYOUT)
    assert not res.weave.status.any()


def test_empty_documents_among_the_look_back_words(weaver):
    """Every tenth of 200 documents is empty on both sides: its word adds 0, and
    the document after it starts where it does."""
    a, b = tiny_docs(200, empty_every=10)
    res = check(weaver, a, b, LAYOUT)
    moff = res.offsets.astype(np.int64)
    empty = np.arange(9, 200, 10)
    np.testing.assert_array_equal(moff[empty + 1], moff[empty])
    np.testing.assert_array_equal(res.weave.status[empty], abi.STATUS_ROOT)
    assert not np.delete(res.weave.status, empty).any()


# ------------------------------------------------------------------ 10. bad inputs
def raw_call(weaver, a, b, layout, tweak, memspace=abi.CW_MEM_HOST):
    """cw_merge_lists through the C ABI with one field spoiled by tweak(batch,
    result, a_offsets).  The arrays are host memory; every check this test aims
    at fails before anything is read from them."""
    keep = [np.ascontiguousarray(x) for x in a + b]
    ao, bo = keep[0].copy(), keep[5].copy()
    ba, _ = weaver._batch(ao, *(abi._ptr(x) for x in keep[1:4]), layout)
    bb, _ = weaver._batch(bo, *(abi._ptr(x) for x in keep[6:9]), layout)
    mb = abi.CwMergeBatch(ba, abi._ptr(keep[4]), bb, abi._ptr(keep[9]))
    NC, D = len(keep[1]) + len(keep[6]), len(ao) - 1
    mo = np.zeros(D + 1, np.uint64)
    out = [np.zeros(NC + 32, np.uint32) for _ in range(3)] + [np.zeros(D, np.uint32) for _ in range(2)]
    r = abi.CwMergeResult(mo.ctypes.data_as(C.POINTER(C.c_uint64)), abi._ptr(out[0]),
                          abi.CwListResult(abi._ptr(out[1]), abi._ptr(out[2]), abi._ptr(out[3]), None,
                                           abi._ptr(out[4]), None))
    tweak(mb, r, ao)
    with pytest.raises(abi.WeaveError) as e:
        weaver._check(weaver._L.cw_merge_lists(weaver._h, C.byref(mb), C.byref(r), memspace),
                      "cw_merge_lists")
    assert len(str(e.value)) > len("cw_merge_lists: ")
    return str(e.value)


def test_bad_inputs_fail_with_a_text(weaver):
    off, idk, ck, kd = docs_of([64, 65, 97], seed=40)
    (a, _), (b, _) = split_batch(off, idk, ck, kd, np.random.default_rng(40))
    def n_docs(mb, r, ao): mb.b.n_docs = 2
    def start(mb, r, ao): ao[0] = 1
    def monotone(mb, r, ao): ao[1], ao[2] = ao[2], ao[1]
    def no_status(mb, r, ao): r.weave.status = None
    def no_value(mb, r, ao): mb.a_value = None
    assert "same number" in raw_call(weaver, a, b, LAYOUT, n_docs)
    assert "start at 0" in raw_call(weaver, a, b, LAYOUT, start)
    assert "monotone" in raw_call(weaver, a, b, LAYOUT, monotone)
    assert "required" in raw_call(weaver, a, b, LAYOUT, no_status)
    assert "null" in raw_call(weaver, a, b, LAYOUT, no_value)
    assert "memspace" in raw_call(weaver, a, b, LAYOUT, lambda *x: None, memspace=7)
    # the context still works
    check(weaver, a, b, LAYOUT)
