"""cw_merge_maps (CausalMap's causal-merge, map.cljc:248-249) on the GPU, through
the C ABI and the Python mirror.

Per collection the call returns the full map reweave of the union of the two
replicas' node bags deduplicated by id (include/causeweave.h).  Every case is
checked three ways: the merged nodes against a host reading of the union (ids
strictly ascending, a's copy kept, DUP / ORPHAN bits), the key weaves against
cw_weave_maps of that union (identical arrays: the indices are collection-local
into merged_src), and against the C oracle's literal map fold.  The weaver is
parametrised over the fused union kernel (k_map_union) and the general route.
"""
import random

import numpy as np
import pytest

from cause_amd import abi, gen
from cause_amd import causal as C
from oracle import causal_ref as R
from tests import mapmerge_hist as H
from tests.test_gpu_maps import gpu_maps, literal_histories, oracle_maps

pytestmark = pytest.mark.gpu

UNION_BITS = abi.STATUS_DUP | abi.STATUS_ORPHAN
MAP_FIELDS = ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm", "status")


@pytest.fixture(scope="module", params=[1, 0], ids=["fused", "general"])
def weaver(request):
    w = abi.Weaver(0, options={"map_merge_fused": request.param})
    w.fused = bool(request.param)
    yield w
    w.close()


# ------------------------------------------------------------------ helpers
def split(off, cols, shared, rng, only=None):
    """Two replicas of a batch.  Per collection `shared` (a fraction, or a list
    of counts) of the nodes go to both sides, the others to one side at random
    (only[d] = "a" / "b": the whole collection on that side alone); each side's
    nodes arrive in a random order.  The value token of a node is its index in
    the batch.  Returns the two sides as cw_merge_maps takes them, and each
    side's batch indices."""
    D = len(off) - 1
    ia, ib, oa, ob = [], [], [0], [0]
    for d in range(D):
        lo, n = int(off[d]), int(off[d + 1]) - int(off[d])
        k = shared[d] if hasattr(shared, "__len__") else int(round(shared * n))
        perm = rng.permutation(n)
        both, rest = perm[:k], perm[k:]
        to_a = rng.random(len(rest)) < 0.5
        if only and d in only:
            both, to_a = perm[:0], np.full(n, only[d] == "a")
            rest = perm
        a = np.concatenate([both, rest[to_a]])
        b = np.concatenate([both, rest[~to_a]])
        ia.append(lo + rng.permutation(a))
        ib.append(lo + rng.permutation(b))
        oa.append(oa[-1] + len(a))
        ob.append(ob[-1] + len(b))
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)
    ia, ib = cat(ia), cat(ib)
    val = np.arange(int(off[-1]), dtype=np.uint64)
    side = lambda o, ix: (np.array(o, np.uint64),) + tuple(c[ix] for c in cols) + (val[ix],)
    return side(oa, ia), side(ob, ib), ia, ib


def coll_of(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))


def merged_index(res, a, b):
    """For every merged node: (from a?, index into that side's arrays)."""
    d = coll_of(res.offsets)
    s = res.src.astype(np.int64)
    oa, ob = a[0].astype(np.int64), b[0].astype(np.int64)
    na = (oa[1:] - oa[:-1])[d]
    from_a = s < na
    return from_a, np.where(from_a, oa[d] + s, ob[d] + s - na)


def gather_union(res, a, b):
    from_a, ix = merged_index(res, a, b)
    pick = lambda k: np.where(from_a, a[k][np.minimum(ix, max(len(a[k]) - 1, 0))] if len(a[k]) else 0,
                              b[k][np.minimum(ix, max(len(b[k]) - 1, 0))] if len(b[k]) else 0)
    return tuple(pick(k).astype(a[k].dtype) for k in (1, 2, 3, 4))


def host_union(a, b):
    """Host reading of the union: per collection the merged (side, index) list in
    id order with a's copy first, and the DUP / ORPHAN bits."""
    D = len(a[0]) - 1
    bits = np.zeros(D, np.uint32)
    merged = []
    for d in range(D):
        seen = {}
        for sd, t in ((0, a), (1, b)):
            for j in range(int(t[0][d]), int(t[0][d + 1])):
                body = (int(t[2][j]), int(t[3][j]), int(t[4][j]) & 0x3F, int(t[5][j]))
                i = int(t[1][j])
                if i not in seen:
                    seen[i] = (body, sd, j)
                elif seen[i][0] != body:
                    bits[d] |= abi.STATUS_DUP
        for body, _, _ in seen.values():
            if body[1] == 1 and body[0] not in seen:
                bits[d] |= abi.STATUS_ORPHAN
        merged.append([(seen[i][1], seen[i][2]) for i in sorted(seen)])
    return merged, bits


def check(weaver, a, b, tb, oracle_too=True):
    """The merge of a and b against the host union, cw_weave_maps of the union
    and the C oracle's map fold.  Returns the result and the union's bits."""
    res = weaver.merge_maps(a, b, tb)
    D = len(a[0]) - 1
    merged, bits = host_union(a, b)
    # the merged nodes: the union, ids strictly ascending, a's copy kept
    from_a, ix = merged_index(res, a, b)
    want = [(0 if sd == 0 else 1, j) for m in merged for sd, j in m]
    got = list(zip((~from_a).astype(int).tolist(), ix.tolist()))
    assert got == want
    np.testing.assert_array_equal(res.offsets, np.cumsum([0] + [len(m) for m in merged]).astype(np.uint64))
    uid, uc, uci, ukd = gather_union(res, a, b)
    for d in range(D):
        seg = uid[int(res.offsets[d]):int(res.offsets[d + 1])].astype(np.int64)
        assert np.all(seg[1:] > seg[:-1]), f"collection {d}: merged ids not strictly ascending"
    # the weave: cw_weave_maps of the union, array for array
    ref = weaver.weave_maps(res.offsets, uid, uc, uci, ukd, tb)
    for f in MAP_FIELDS[:-1]:
        np.testing.assert_array_equal(getattr(res.maps, f), getattr(ref, f), err_msg=f)
    np.testing.assert_array_equal(res.maps.status, ref.status | bits)
    if oracle_too:
        got, want = gpu_maps(res.maps, D), oracle_maps(res.offsets, uid, uc, uci, ukd)
        for d in range(D):
            if not (bits[d] & abi.STATUS_DUP or ref.status[d] & (abi.STATUS_DUP | abi.STATUS_MAP_KEY)):
                assert got[d] == want[d], f"collection {d}"
    return res, bits


def routes(weaver, call):
    """Kernel stat names of one merge call."""
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        call()
        return set(weaver.kernel_stats())
    finally:
        weaver.set_profiling(False)
        weaver.reset_kernel_stats()


def concat(batches):
    off = [np.zeros(1, np.uint64)]
    for o in (x[0] for x in batches):
        off.append(off[-1][-1] + o[1:])
    return (np.concatenate(off),) + tuple(np.concatenate([x[k] for x in batches]) for k in (1, 2, 3, 4))


def sized(sizes, seed):
    """A map batch with collections of exactly these sizes (0 allowed)."""
    parts = []
    for d, n in enumerate(sizes):
        if n == 0:
            parts.append((np.zeros(2, np.uint64),) + (np.zeros(0, np.uint64),) * 2 + (np.zeros(0, np.uint8),) * 2)
            continue
        spec = gen.MapSpec(nodes_per_coll=n, n_keys=7, seed=seed + d)
        parts.append(gen.generate_maps(spec, d, d + 1, nthreads=1))
    return concat(parts)


# ------------------------------------------------------------------ 1. config 4
@pytest.fixture(scope="module")
def config4():
    _, tb = gen.CONFIG4.layout()
    return gen.generate_maps(gen.CONFIG4, 0, 300, nthreads=8), tb


@pytest.mark.parametrize("overlap", [0.2, 0.0, 1.0])
def test_config4_splits(weaver, config4, overlap):
    (off, *cols), tb = config4
    a, b, ia, ib = split(off, cols, overlap, np.random.default_rng(int(overlap * 10)))
    res, bits = check(weaver, a, b, tb)
    assert not bits.any() and not res.maps.status.any()
    # the union is the collection
    np.testing.assert_array_equal(res.offsets, off)
    from_a, ix = merged_index(res, a, b)
    g = np.where(from_a, ia[np.minimum(ix, len(ia) - 1)] if len(ia) else 0,
                 ib[np.minimum(ix, len(ib) - 1)] if len(ib) else 0)
    np.testing.assert_array_equal(np.sort(g), np.arange(int(off[-1])))
    np.testing.assert_array_equal(coll_of(off)[g], coll_of(res.offsets))


# ------------------------------------------------------------------ 2. packs and routes
def test_pack_limit_sizes_take_the_fused_kernel(weaver):
    """na + nb of 1, 2,047 and 2,048 next to small collections: one kernel
    when the option is on."""
    off, *cols = sized([1, 2000, 2000, 5, 9], 40)
    tb = 3
    shared = [0, 47, 48, 2, 3]
    a, b, _, _ = split(off, cols, shared, np.random.default_rng(2))
    tot = np.diff(a[0].astype(np.int64)) + np.diff(b[0].astype(np.int64))
    assert tot.tolist() == [1, 2047, 2048, 7, 12]
    check(weaver, a, b, tb)
    names = routes(weaver, lambda: weaver.merge_maps(a, b, tb))
    assert ("map_union" in names) == weaver.fused and ("mm_concat" in names) == (not weaver.fused)


def test_one_oversize_collection_takes_the_general_route(weaver):
    """na + nb = 2,049 in one collection: the whole call goes the general way
    under either option."""
    off, *cols = sized([6, 2000, 3], 50)
    a, b, _, _ = split(off, cols, [1, 49, 0], np.random.default_rng(3))
    assert int(a[0][2] - a[0][1] + b[0][2] - b[0][1]) == 2049
    check(weaver, a, b, 3)
    names = routes(weaver, lambda: weaver.merge_maps(a, b, 3))
    assert "mm_concat" in names and "map_union" not in names


def test_packs_filled_exactly(weaver):
    """Eight collections of na + nb = 128: two 512-node packs filled to the last
    node, then a third pack; and four of 512, one pack each."""
    for n, k, reps in ((100, 28, 9), (400, 112, 4)):
        off, *cols = sized([n] * reps, 60 + n)
        a, b, _, _ = split(off, cols, [k] * reps, np.random.default_rng(n))
        tot = np.diff(a[0].astype(np.int64)) + np.diff(b[0].astype(np.int64))
        assert (tot == n + k).all() and 512 % (n + k) == 0
        check(weaver, a, b, 3)


@pytest.mark.parametrize("colls", [65, 129])
def test_packs_at_a_look_back_window_boundary(weaver, colls):
    """Collections of na + nb = 300 are one 512-node pack each: with 65 and 129 of
    them the last pack of k_map_union has 64 and 128 predecessors: its look-back
    ends exactly on the boundary of a 64-word window (the first, the second)."""
    off, *cols = sized([250] * colls, 300)
    a, b, _, _ = split(off, cols, [50] * colls, np.random.default_rng(colls))
    tot = np.diff(a[0].astype(np.int64)) + np.diff(b[0].astype(np.int64))
    assert (tot == 300).all()
    res, bits = check(weaver, a, b, 3)
    assert not bits.any()
    np.testing.assert_array_equal(res.offsets, off)


def test_empty_collections_and_empty_batches(weaver):
    off, *cols = sized([4, 7, 0, 5, 0, 0, 9, 3], 70)
    a, b, _, _ = split(off, cols, 0.3, np.random.default_rng(4), only={1: "a", 3: "b", 7: "a"})
    na, nb = np.diff(a[0].astype(np.int64)), np.diff(b[0].astype(np.int64))
    assert nb[1] == 0 and na[3] == 0 and na[2] == nb[2] == 0 and nb[7] == 0
    res, _ = check(weaver, a, b, 3)
    assert res.maps.status[2] == 0 and 2 not in res.maps.seg_coll.tolist()
    # a batch of zero nodes, and one side of zero nodes
    e = (np.zeros(4, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
         np.zeros(0, np.uint8), np.zeros(0, np.uint64))
    res = weaver.merge_maps(e, e, 3)
    assert res.offsets.tolist() == [0, 0, 0, 0] and len(res.src) == 0
    assert len(res.maps.seg_key) == 0 and res.maps.status.tolist() == [0, 0, 0]
    off3, *cols3 = sized([3, 0, 6], 71)
    a3, b3, _, _ = split(off3, cols3, 0.0, np.random.default_rng(5), only={0: "b", 2: "b"})
    assert len(a3[1]) == 0
    check(weaver, a3, b3, 3)


def test_one_collection(weaver):
    for n in (1, 37, 700):
        off, *cols = sized([n], 80 + n)
        a, b, _, _ = split(off, cols, 0.5, np.random.default_rng(n))
        check(weaver, a, b, 3)


def test_bad_inputs_fail_with_a_text(weaver):
    off, *cols = sized([2, 3], 90)
    a, b, _, _ = split(off, cols, 1.0, np.random.default_rng(1))
    back = (np.array([0, 7, 5], np.uint64),) + a[1:]  # offsets that run backwards inside
    with pytest.raises(abi.WeaveError, match="not monotone"):
        weaver.merge_maps(back, b, 3)
    with pytest.raises(abi.WeaveError, match="token_bits"):
        weaver.merge_maps(a, b, 0)
    with pytest.raises(abi.WeaveError, match="same number of collections"):
        r = abi.CwMapMergeResult()
        mb = abi.CwMapMergeBatch()
        mb.a.n_colls, mb.b.n_colls = 2, 3
        weaver._check(weaver._L.cw_merge_maps(weaver._h, abi.C.byref(mb), abi.C.byref(r), 0), "cw_merge_maps")
    with pytest.raises(abi.WeaveError, match="coll_offsets is required"):
        mb.b.n_colls = 2
        weaver._check(weaver._L.cw_merge_maps(weaver._h, abi.C.byref(mb), abi.C.byref(r), 0), "cw_merge_maps")
    check(weaver, a, b, 3)  # the context is still good


# ------------------------------------------------------------------ 3. self merge
def test_merging_a_batch_with_itself(weaver, config4):
    (off, idk, ck, ci, kd), tb = config4
    s = (off, idk, ck, ci, kd, np.arange(len(idk), dtype=np.uint64))
    res = weaver.merge_maps(s, s, tb)
    np.testing.assert_array_equal(res.offsets, off)
    na = np.diff(off.astype(np.int64))[coll_of(off)]
    assert (res.src < na).all()  # every node is a's copy
    assert not res.maps.status.any()
    # the weave of the batch, through merged_src
    ref = weaver.weave_maps(off, idk, ck, ci, kd, tb)
    for f in ("seg_offsets", "seg_coll", "seg_key", "status"):
        np.testing.assert_array_equal(getattr(res.maps, f), getattr(ref, f))
    base = off.astype(np.int64)[res.maps.seg_coll]
    act = res.maps.seg_active
    got_act = np.where(act < 0, -1, res.src.astype(np.int64)[np.maximum(base + act, 0)])
    np.testing.assert_array_equal(got_act, ref.seg_active)
    seg_of = np.repeat(np.arange(len(ref.seg_key)), np.diff(ref.seg_offsets.astype(np.int64)))
    p = res.maps.seg_perm.astype(np.int64)
    root = p == 0xFFFFFFFF
    got_perm = np.where(root, 0xFFFFFFFF, res.src.astype(np.int64)[np.where(root, 0, base[seg_of] + p)])
    np.testing.assert_array_equal(got_perm, ref.seg_perm)


# ------------------------------------------------------------------ 4. status bits
T = lambda ts, site=1: (ts << 2) | site


def hand(colls):
    """Sides from per-collection (a nodes, b nodes) of (id, cause, cis, kind, value)."""
    def side(k):
        off, rows = [0], []
        for c in colls:
            rows += c[k]
            off.append(len(rows))
        col = lambda j, dt: np.array([r[j] for r in rows], dt)
        return (np.array(off, np.uint64), col(0, np.uint64), col(1, np.uint64), col(2, np.uint8),
                col(3, np.uint8), col(4, np.uint64))
    return side(0), side(1)


def test_union_status_bits(weaver):
    X, Y, Z = T(1), T(2), T(3)
    colls = [
        # 0: equal bodies are one node
        ([(X, 0, 0, 0, 7)], [(Y, 1, 0, 0, 8), (X, 0, 0, 0, 7)]),
        # 1-4: the second copy differs only in value token / cause / cause_is_id / kind
        ([(X, 0, 0, 0, 7)], [(X, 0, 0, 0, 9)]),
        ([(X, 0, 0, 0, 7)], [(X, 1, 0, 0, 7)]),
        ([(X, 0, 0, 0, 7), (Y, X, 1, 0, 8)], [(Y, X, 0, 0, 8)]),  # the same 64-bit word
        ([(X, 0, 0, 0, 7)], [(X, 0, 0, 1, 7)]),
        # 5, 6: the same id in two collections of one pack is no repeat
        ([(X, 0, 0, 0, 7)], []),
        ([], [(X, 1, 0, 1, 9)]),
        # 7: an id cause absent from both sides; 8: a cause equal to the root id
        ([(X, 0, 0, 0, 7), (Y, T(40), 1, 2, 8)], [(Z, X, 1, 1, 9)]),
        ([(X, 0, 0, 0, 7)], [(Y, 0, 1, 0, 8)]),
        # 9: the cause is on the other side only
        ([(Y, X, 1, 2, 8)], [(X, 0, 0, 0, 7)]),
        ([(X, 0, 0, 0, 7)], [(Z, X, 1, 3, 8)]),
    ]
    a, b = hand(colls)
    res, bits = check(weaver, a, b, 3)
    D, O = abi.STATUS_DUP, abi.STATUS_ORPHAN
    assert bits.tolist() == [0, D, D, D, D, 0, 0, O, O, 0, 0]
    assert (res.maps.status & UNION_BITS).tolist() == bits.tolist()
    assert res.src[:2].tolist() == [0, 1]  # collection 0: X is a's copy, Y is b's node 0
    # orphans are still woven as cw_weave_maps weaves them: under the nil key
    nil = np.uint64((1 << 64) - 1)
    for d in (7, 8):
        assert ((res.maps.seg_coll == d) & (res.maps.seg_key == nil)).sum() == 1


# ------------------------------------------------------------------ 5. F8c collections
def test_f8c_collections_equal_the_weave_of_the_union(weaver):
    """Id keys, the nil key, self-caused ids (test_gpu_maps.literal_histories)
    split across the replicas: the stated definition, the reweave of the union."""
    off, *cols = literal_histories(random.Random(31), 250, 2, 30, t_max=200)
    a, b, _, _ = split(off, cols, 0.25, np.random.default_rng(6))
    res, bits = check(weaver, a, b, 2)
    assert (bits & abi.STATUS_ORPHAN).any() and not (bits & abi.STATUS_DUP).any()
    assert (res.maps.seg_key >> np.uint64(63)).any()  # id keys and nil keys occur


# ------------------------------------------------------------------ 6. both routes
def test_both_routes_give_identical_arrays(config4):
    (off, *cols), tb = config4
    lo, *lcols = literal_histories(random.Random(32), 100, 2, 30, t_max=200)
    cases = [split(off, cols, 0.2, np.random.default_rng(7))[:2] + (tb,),
             split(lo, lcols, 0.3, np.random.default_rng(8))[:2] + (2,)]
    with abi.Weaver(0, options={"map_merge_fused": 1}) as wf, \
            abi.Weaver(0, options={"map_merge_fused": 0}) as wg:
        for a, b, bits in cases:
            x, y = wf.merge_maps(a, b, bits), wg.merge_maps(a, b, bits)
            np.testing.assert_array_equal(x.offsets, y.offsets)
            np.testing.assert_array_equal(x.src, y.src)
            for f in MAP_FIELDS:
                np.testing.assert_array_equal(getattr(x.maps, f), getattr(y.maps, f), err_msg=f)


# ------------------------------------------------------------------ 7. device memory
def test_device_memory_call_matches_host(weaver, config4):
    import torch

    (off, *cols), tb = config4
    a, b, _, _ = split(off, cols, 0.2, np.random.default_rng(9))
    host = weaver.merge_maps(a, b, tb)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    ga, gb = [up(x) for x in a[1:]], [up(x) for x in b[1:]]
    NC, D = len(a[1]) + len(b[1]), len(off) - 1
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    o = {"seg_offsets": z(NC + 1, torch.int64), "seg_coll": z(NC, torch.int32),
         "seg_key": z(NC, torch.int64), "seg_active": z(NC, torch.int64),
         "seg_perm": z(2 * NC, torch.int32), "status": z(D, torch.int32)}
    src = z(NC, torch.int32)
    mo, S = weaver.merge_maps_device(a[0], [x.data_ptr() for x in ga], b[0],
                                     [x.data_ptr() for x in gb], tb, 0, src.data_ptr(),
                                     {k: v.data_ptr() for k, v in o.items()}, NC)
    torch.cuda.synchronize()
    M = int(mo[-1])
    np.testing.assert_array_equal(mo, host.offsets)
    assert S == len(host.maps.seg_key)
    np.testing.assert_array_equal(src[:M].cpu().numpy().view(np.uint32), host.src)
    h = {k: v.cpu().numpy() for k, v in o.items()}
    np.testing.assert_array_equal(h["seg_offsets"][:S + 1].view(np.uint64), host.maps.seg_offsets)
    np.testing.assert_array_equal(h["seg_coll"][:S].view(np.uint32), host.maps.seg_coll)
    np.testing.assert_array_equal(h["seg_key"][:S].view(np.uint64), host.maps.seg_key)
    np.testing.assert_array_equal(h["seg_active"][:S], host.maps.seg_active)
    np.testing.assert_array_equal(h["seg_perm"][:M + S].view(np.uint32), host.maps.seg_perm)
    np.testing.assert_array_equal(h["status"].view(np.uint32), host.maps.status)


# ------------------------------------------------------------------ 8. repeated calls
def test_repeated_calls_are_identical(weaver, config4):
    """The look-back words carry an epoch and are not cleared between calls: the
    same batch three times, with a smaller and a larger batch in between."""
    (off, *cols), tb = config4
    a, b, _, _ = split(off, cols, 0.2, np.random.default_rng(10))
    o2, *c2 = gen.generate_maps(gen.CONFIG4, 300, 340, nthreads=4)
    small = split(o2, c2, 0.2, np.random.default_rng(11))[:2]
    o3, *c3 = gen.generate_maps(gen.CONFIG4, 400, 900, nthreads=8)
    large = split(o3, c3, 0.2, np.random.default_rng(12))[:2]
    first = weaver.merge_maps(a, b, tb)
    for other in (small, large):
        weaver.merge_maps(other[0], other[1], tb)
        again = weaver.merge_maps(a, b, tb)
        np.testing.assert_array_equal(again.offsets, first.offsets)
        np.testing.assert_array_equal(again.src, first.src)
        for f in MAP_FIELDS:
            np.testing.assert_array_equal(getattr(again.maps, f), getattr(first.maps, f), err_msg=f)


# ------------------------------------------------------------------ 9. the mirror
def _mv(v):
    return C.Keyword(v.ns, v.name) if isinstance(v, R.Keyword) else v


def _mirror_ct(nodes, ref):
    ct = C.new_map_ct(site_id=ref["site_id"], uuid=ref["uuid"])
    ct["nodes"] = {i: (c, _mv(v)) for i, (c, v) in nodes.items()}
    ct["lamport_ts"] = ref["lamport_ts"]
    return ct


def _mweave(w):
    return {k: [(n[0], n[1], _mv(n[2])) for n in kw] for k, kw in w.items()}


def test_mirror_merge_trees_equals_the_reference():
    pairs, want = [], []
    for seed in range(40):
        a, b = H.split(H.history(seed), seed)
        r1, r2 = H.ref_ct(a), H.ref_ct(b)
        want.append(R.merge_trees(R.map_weave, r1, r2))
        pairs.append((_mirror_ct(a, r1), _mirror_ct(b, r2)))
    got = C.merge_maps(pairs)
    got[0] = C.merge_trees(C.map_weave, *pairs[0])  # the one-pair entry point
    for g, w in zip(got, want):
        assert g["weave"] == _mweave(w["weave"])
        assert C.causal_map_to_edn(g) == {k: _mv(v) for k, v in R.causal_map_to_edn(w).items()}
        assert g["lamport_ts"] == w["lamport_ts"]
        assert g["nodes"] == {i: (c, _mv(v)) for i, (c, v) in w["nodes"].items()}


def test_mirror_merge_errors():
    a, b = H.split(H.history(3), 3)
    r1, r2 = H.ref_ct(a), H.ref_ct(b)
    m1, m2 = _mirror_ct(a, r1), _mirror_ct(b, r2)

    def causes(x, y):
        with pytest.raises(C.CauseError) as e:
            C.merge_trees(C.map_weave, x, y)
        return e.value.causes

    assert causes(m1, C.new_list_ct(uuid=m1["uuid"])) == {"type-missmatch"}
    assert causes(C.new_list_ct(uuid=m1["uuid"]), m1) == {"type-missmatch"}
    assert causes(m1, dict(m2, uuid="V" * 21)) == {"uuid-missmatch"}
    i, (c, v) = next(iter(m1["nodes"].items()))
    edited = dict(m2, nodes=dict(m2["nodes"]))
    edited["nodes"][i] = (c, "another value")
    assert causes(m1, edited) == {"append-only", "edits-not-allowed"}
    orphan = dict(m2, nodes=dict(m2["nodes"]))
    orphan["nodes"][(99, i[1], 0)] = ((98, i[1], 0), 1)
    assert causes(m1, orphan) == {"cause-must-exist"}


def test_mirror_map_insert_bulk_and_list_merges():
    nodes = H.history(5)
    a, b = H.split(nodes, 5)
    ct = C.weave_maps([_mirror_ct(a, H.ref_ct(a))])[0]
    got = C.map_insert_bulk(ct, [(i, c, _mv(v)) for i, (c, v) in b.items()])
    allc = dict(a)
    allc.update(b)
    want = C.refresh_caches(C.map_weave, _mirror_ct(allc, H.ref_ct(allc)))
    assert got["weave"] == want["weave"] and got["_active"] == want["_active"]
    assert got["nodes"] == want["nodes"]
    # lists still merge through merge_trees
    l1 = C.list_conj(C.new_list_ct(rng=random.Random(1)), "a")
    l2 = C.list_conj(l1, "b")
    assert C.causal_list_to_edn(C.merge_trees(C.list_weave, l1, l2)) == ["a", "b"]
