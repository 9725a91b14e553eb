"""cw_insert_maps on the GPU (include/causeweave_map_insert.h, mapinsert.hip)
against tests/mapinsert_model.py, array for array, at both group widths
(map_insert_wave = 1: a wave a collection; 0: a workgroup a collection).

The old collections are woven by cw_weave_maps; the model then says what one
tx a collection makes of them.  Collections are built as columns: ids are
ts << 12 | site << 8 | tx, key tokens small integers.
"""
import ctypes as C
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest

from cause_amd import abi, abi_map_insert
from tests import mapinsert_gen as G
from tests import mapinsert_model as M

pytestmark = pytest.mark.gpu

U8, U32, U64, I64 = np.uint8, np.uint32, np.uint64, np.int64
NORMAL, HIDE, HHIDE, HSHOW, KINDS = G.NORMAL, G.HIDE, G.HHIDE, G.HSHOW, G.KINDS
key, gen_coll, gen_tx = G.key, G.gen_coll, G.gen_tx
NONE = 0xFFFFFFFF
TOKEN_BITS = 20


@pytest.fixture(scope="module", params=[1, 0], ids=["wave", "workgroup"])
def weaver(request):
    with abi.Weaver(0, options={"map_insert_wave": request.param}) as w:
        w.wave = request.param
        yield w


def columns(lists):
    off = np.zeros(len(lists) + 1, U64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = [r for x in lists for r in x]
    col = lambda c, dt: np.array([r[c] for r in flat], dt)
    idk, kd = col(0, U64), col(3, U8)
    return off, idk, col(1, U64), col(2, U8), kd, idk * U64(3) + kd.astype(U64)


def batch(weaver, colls, txs):
    """The batch of collections (woven here by cw_weave_maps) and their txs."""
    off, idk, ca, ci, kd, val = columns(colls)
    toff, tid, tca, tci, tkd, tval = columns(txs)
    segs = weaver.weave_maps(off, idk, ca, ci, kd, TOKEN_BITS)
    assert not (segs.status & (abi.STATUS_DUP | abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL)).any()
    return NS(off=off, idk=idk, ca=ca, ci=ci, kd=kd, val=val, toff=toff, tid=tid, tca=tca, tci=tci, tkd=tkd,
              tval=tval, segs=segs, colls=colls, txs=txs)


def model_of(b, values=True):
    s = b.segs
    return M.insert_maps(b.off, b.idk, b.ca, b.ci, b.kd, s.seg_offsets, s.seg_coll, s.seg_key, s.seg_active,
                         s.seg_perm, b.toff, b.tid, b.tca, b.tci, b.tkd, b.val if values else None,
                         b.tval if values else None)


def host_call(weaver, b, values=True, cols=True):
    return abi_map_insert.insert_maps(weaver, (b.off, b.idk, b.ca, b.ci, b.kd), b.segs,
                                      (b.toff, b.tid, b.tca, b.tci, b.tkd, b.tval if values else None),
                                      coll_value=b.val if values else None, columns=cols)


def up(x):
    import torch

    signed = {np.dtype(U64): np.int64, np.dtype(U32): np.int32}.get(x.dtype)
    x = np.ascontiguousarray(x)
    if not len(x):
        x = np.zeros(1, x.dtype)
    return torch.from_numpy(x.view(signed) if signed else x).to(torch.device("cuda", 0))


def device_call(weaver, b, null=()):
    """The device-memory call on torch tensors; returns a MapInsertResult of host copies."""
    import torch

    s = b.segs
    N, T, S, D = len(b.idk), len(b.tid), len(s.seg_key), len(b.off) - 1
    cap, M_ = max(S + T, 1), max(N + T, 1)
    g = [up(x) for x in (b.idk, b.ca, b.ci, b.kd, b.val, s.seg_offsets, s.seg_coll, s.seg_key, s.seg_active,
                         s.seg_perm, b.tid, b.tca, b.tci, b.tkd, b.tval)]
    z = lambda n, dt: torch.full((max(n, 1),), 0x55, dtype=dt, device=g[0].device)
    o = {"seg_offsets": z(cap + 1, torch.int64), "seg_coll": z(cap, torch.int32), "seg_key": z(cap, torch.int64),
         "seg_active": z(cap, torch.int64), "seg_perm": z(M_ + cap, torch.int32), "status": z(D, torch.int32)}
    tseg, tpos = z(T, torch.int32), z(T, torch.int32)
    cols = [z(M_, torch.int64), z(M_, torch.int64), z(M_, torch.uint8), z(M_, torch.uint8), z(M_, torch.int64)]
    ptr = lambda t, name: None if name in null else t.data_ptr()
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    offs, ns = abi_map_insert.insert_maps_device(
        weaver, b.off, [t.data_ptr() for t in g[:4]], S, [t.data_ptr() for t in g[5:10]], b.toff,
        [t.data_ptr() for t in g[10:14]] + [ptr(g[14], "value")], {k: v.data_ptr() for k, v in o.items()}, cap,
        tx_seg_ptr=ptr(tseg, "tx_seg"), tx_pos_ptr=ptr(tpos, "tx_pos"), value_ptr=ptr(g[4], "value"),
        col_ptrs=None if "columns" in null else [t.data_ptr() for t in cols[:4]] + [ptr(cols[4], "value")])
    torch.cuda.synchronize()
    m = int(offs[-1])
    host = lambda t, dt, n, name="": None if name in null else t.cpu().numpy().view(dt)[:n]
    mr = abi.MapResult(host(o["seg_offsets"], U64, ns + 1), host(o["seg_coll"], U32, ns),
                       host(o["seg_key"], U64, ns), host(o["seg_active"], I64, ns),
                       host(o["seg_perm"], U32, m + ns), host(o["status"], U32, D))
    c = "columns"
    return abi_map_insert.MapInsertResult(
        offs, host(tseg, U32, T, "tx_seg"), host(tpos, U32, T, "tx_pos"), mr, host(cols[0], U64, m, c),
        host(cols[1], U64, m, c), host(cols[2], U8, m, c), host(cols[3], U8, m, c),
        host(cols[4], U64, m, "value" if "value" in null else c))


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(at)} of {len(want)} differ, first at {at[0]}: "
                             f"{got[at[0]]} != {want[at[0]]}")


def compare(res, exp, null=()):
    """Every array of a MapInsertResult against the model's."""
    same(res.offsets, exp.new_offsets, "new_offsets")
    same(res.maps.status, exp.status, "status")
    for f in ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm"):
        same(getattr(res.maps, f), getattr(exp, f), f)
    for f in ("tx_seg", "tx_pos"):
        if f not in null:
            same(getattr(res, f), getattr(exp, f), f)
    if "columns" not in null:
        for f in ("id_key", "cause", "cause_is_id", "kind"):
            same(getattr(res, f), getattr(exp, f), f)
        if "value" not in null and exp.value is not None:
            same(res.value, exp.value, "value")


def reweave_equal(weaver, res):
    """maps equals cw_weave_maps of the output columns, array for array."""
    w = weaver.weave_maps(res.offsets, res.id_key, res.cause, res.cause_is_id, res.kind, TOKEN_BITS)
    for f in ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm"):
        same(getattr(res.maps, f), getattr(w, f), "reweave " + f)


# ------------------------------------------------------------------- the batch
SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def refusals(rng):
    """(collection, tx, status) for every refusal, and the accepted first assoc."""
    rows = gen_coll(rng, 20)
    x = rows[5]
    fresh = key(500, 7)
    return [
        (rows, [x, (key(500, 7, 1), 1, 0, NORMAL)], 0),                       # the same body: skipped
        (rows, [(x[0], x[1], x[2], x[3] ^ 1)], M.STATUS_DUP),                 # another body
        (rows, [(fresh, key(9998, 3), 1, NORMAL)], M.STATUS_ORPHAN),          # an absent id cause
        (rows, [(fresh, 0, 1, NORMAL)], M.STATUS_ORPHAN),                     # the root id
        (rows, [(fresh, 0, 2, NORMAL)], M.STATUS_ORPHAN),                     # nil
        (rows, [(fresh, key(500, 7, 1), 1, NORMAL), (key(500, 7, 1), 1, 0, NORMAL)], M.STATUS_ORPHAN),
        (rows, [(fresh, 1, 0, NORMAL), (key(500, 7, 1), 1 << 62, 0, NORMAL)], M.STATUS_MAP_KEY),
        ([], [(fresh, 0, 1, NORMAL)], M.STATUS_ORPHAN),
        ([], [(fresh, 3, 0, NORMAL)], 0),                                      # the first assoc
        ([], [], 0), (rows, [], 0),
    ] + [(c, t, 0) for c, t in shapes()]


def shapes():
    """(collection, tx) with the key weaves and same-tx causes the batch must hold
    whatever the random part gives."""
    A, B, Cn, f = key(1, 1), key(2, 1), key(3, 1), lambda m: key(500, 7, m)
    plain = [(A, 1, 0, NORMAL)]
    idk = [(A, 1, 0, NORMAL), (B, A, 1, NORMAL)]  # a node under B goes to the id key weave of A
    return [
        (plain + [(B, 0, 2, NORMAL)], [(f(0), 1, 0, NORMAL), (f(1), 0, 2, NORMAL)]),  # the nil key weave, existing
        (plain, [(f(0), 1, 0, NORMAL), (f(1), 0, 2, HIDE)]),                          # ... and new
        (idk + [(Cn, B, 1, NORMAL)], [(f(0), 1, 0, NORMAL), (f(1), B, 1, HSHOW)]),    # an id key weave, existing
        (idk, [(f(0), 1, 0, NORMAL), (f(1), B, 1, NORMAL)]),                          # ... and new
        (plain, [(f(0), 1, 0, NORMAL), (f(1), f(0), 1, HHIDE)]),                      # under an earlier tx node
        (plain, [(f(0), 1, 0, NORMAL), (f(1), f(2), 1, NORMAL), (f(2), 3, 0, NORMAL)]),  # under a later one
    ]


@pytest.fixture(scope="module")
def big(weaver):
    rng = random.Random(21)
    colls, txs, want = [], [], []
    for i in range(300):
        n = SIZES[i % len(SIZES)] if i % 3 else rng.randrange(0, 40)
        rows = gen_coll(rng, n, hot=0.7 if i % 7 == 0 else 0.0)
        colls.append(rows)
        txs.append(gen_tx(rng, rows, [0, 1, 2, 3, 8][i % 5], 1000 + i))
        want.append(None)
    for rows, tx, st in refusals(rng):
        at = rng.randrange(len(colls))
        colls.insert(at, rows), txs.insert(at, tx), want.insert(at, st)
    b = batch(weaver, colls, txs)
    b.want = want
    b.exp = model_of(b)
    return b


def test_the_batch_holds_the_cases_it_names(big):
    exp, b = big.exp, big
    for d, st in enumerate(b.want):
        if st is not None:
            assert int(exp.status[d]) == st
    grew = np.diff(exp.new_offsets.astype(I64)) - np.diff(b.off.astype(I64))
    k = np.diff(b.toff.astype(I64))
    assert ((grew == k) | (grew == 0)).all() and (grew[k > 0] == 0).sum() >= 8 and (grew > 0).sum() > 200
    ok = exp.tx_seg != NONE
    assert exp.n_segs > len(b.segs.seg_key)                       # new key weaves
    first = np.concatenate([[True], exp.seg_coll[1:] != exp.seg_coll[:-1]])
    last = np.concatenate([exp.seg_coll[1:] != exp.seg_coll[:-1], [True]])
    old = set(zip(b.segs.seg_coll.tolist(), b.segs.seg_key.tolist()))
    new = np.array([(c, kk) not in old for c, kk in zip(exp.seg_coll.tolist(), exp.seg_key.tolist())])
    assert (new & first).any() and (new & last).any() and (new & ~first & ~last).any()
    # the nil key weave and an id key weave, each existing and new, took a tx node
    tkey, tnew = exp.seg_key[exp.tx_seg[ok]], new[exp.tx_seg[ok]]
    nil, idkey = tkey == U64(M.NIL), (tkey >> U64(63) == 1) & (tkey != U64(M.NIL))
    assert (nil & tnew).any() and (nil & ~tnew).any() and (idkey & tnew).any() and (idkey & ~tnew).any()
    # an accepted tx node under an earlier and under a later node of its own tx
    earlier = later = 0
    for d, tx in enumerate(b.txs):
        if grew[d]:
            at = {r[0]: m for m, r in enumerate(tx)}
            earlier += sum(r[2] == 1 and at.get(r[1], m) < m for m, r in enumerate(tx))
            later += sum(r[2] == 1 and at.get(r[1], m) > m for m, r in enumerate(tx))
    assert earlier and later
    lens = np.diff(exp.seg_offsets.astype(I64))
    pos, seg = exp.tx_pos[ok].astype(I64), exp.tx_seg[ok]
    assert (pos == 1).any() and (pos == lens[seg] - 1).any() and ((pos > 1) & (pos < lens[seg] - 1)).any()
    assert (lens[seg][~new[seg]] > 64).any()                      # a key weave longer than a wave
    assert (np.bincount(seg).max() >= 2)                          # the same key weave twice in a tx


def test_host_call_equals_the_model(weaver, big):
    compare(host_call(weaver, big), big.exp)


def test_device_call_equals_the_model(weaver, big):
    compare(device_call(weaver, big), big.exp)


def test_async_device_call(big, weaver):
    with abi.Weaver(0, options={"map_insert_wave": weaver.wave}) as w:
        w.set_async(True)
        compare(device_call(w, big), big.exp)
        compare(device_call(w, big), big.exp)


@pytest.mark.parametrize("null", [("tx_seg",), ("tx_pos",), ("columns",), ("value",), ("tx_seg", "tx_pos", "columns")])
def test_optional_outputs_null(weaver, big, null):
    exp = big.exp if "value" not in null else model_of(big, values=False)
    compare(device_call(weaver, big, null), exp, null)


def test_host_call_without_values_and_columns(weaver, big):
    res = host_call(weaver, big, values=False, cols=False)
    assert res.id_key is None and res.value is None
    compare(res, model_of(big, values=False), ("columns",))


@pytest.mark.parametrize("total", [2047, 2048, 2049])
def test_the_width_threshold(weaver, total):
    rng = random.Random(total)
    rows = gen_coll(rng, total - 3, keys=40, hot=0.3)
    small = gen_coll(rng, 9)
    b = batch(weaver, [small, rows], [gen_tx(rng, small, 2, 5000), gen_tx(rng, rows, 3, 5000)])
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        res = host_call(weaver, b)
        stats = weaver.kernel_stats()
    finally:
        weaver.set_profiling(False)
    compare(res, model_of(b))
    wave = bool(weaver.wave) and total <= 2048
    assert ("map_insert" in stats) == wave and ("map_insert_wg" in stats) == (not wave)


def test_one_large_collection_with_a_long_key_weave(weaver):
    rng = random.Random(5)
    rows = gen_coll(rng, 5000, keys=30, hot=0.6)
    tx = gen_tx(rng, rows, 8, 9000)
    tx[0] = (key(9000, 7, 0), 1, 0, NORMAL)   # into the long key weave
    b = batch(weaver, [rows], [tx])
    assert np.diff(b.segs.seg_offsets.astype(I64)).max() > 2500
    compare(host_call(weaver, b), model_of(b))


def test_a_tx_too_long_for_lds(weaver):
    rng = random.Random(6)
    colls = [gen_coll(rng, n) for n in (30, 0, 200)]
    b = batch(weaver, colls, [gen_tx(rng, colls[0], 150, 700), gen_tx(rng, colls[1], 40, 700),
                              gen_tx(rng, colls[2], 3, 700)])
    compare(host_call(weaver, b), model_of(b))


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5])
def test_the_tail_of_a_workgroup(weaver, D):
    rng = random.Random(D)
    colls = [gen_coll(rng, rng.randrange(0, 30)) for _ in range(D)]
    b = batch(weaver, colls, [gen_tx(rng, c, rng.choice([1, 2, 3]), 600 + i) for i, c in enumerate(colls)])
    compare(host_call(weaver, b), model_of(b))


def test_no_collections_and_all_empty_txs(weaver):
    z = np.zeros(1, U64)
    res = abi_map_insert.insert_maps(weaver, (z, [], [], [], []), (z, [], [], [], []), (z, [], [], [], []))
    assert res.offsets.tolist() == [0] and len(res.maps.seg_key) == 0
    rng = random.Random(8)
    colls = [gen_coll(rng, n) for n in (5, 0, 70)]
    b = batch(weaver, colls, [[], [], []])
    res = host_call(weaver, b)
    compare(res, model_of(b))
    same(res.maps.seg_perm, b.segs.seg_perm, "seg_perm")
    same(res.offsets, b.off, "offsets")


# ------------------------------------------------------------------ seg_active
A, B_, Hd = key(1, 1), key(2, 1), key(3, 1)
ACTIVE = {
    "hide_behind_the_root": ([(A, 1, 0, NORMAL)], [(key(9, 7), 1, 0, HIDE)], -1),
    # a hide of A lands behind B: B is passed over (any hide follows), A is hidden too
    "any_hide_follows": ([(A, 1, 0, NORMAL), (B_, 1, 0, NORMAL)], [(key(9, 7), A, 1, HIDE)], None),
    "hhide_under_the_active": ([(A, 1, 0, NORMAL)], [(key(9, 7), A, 1, HHIDE)], -1),
    "hshow_under_the_hhide": ([(A, 1, 0, NORMAL), (Hd, A, 1, HHIDE)], [(key(9, 7), A, 1, HSHOW)], 0),
    "an_untouched_key_weave": ([(A, 1, 0, NORMAL), (B_, 3, 0, NORMAL)], [(key(9, 7), 3, 0, NORMAL)], None),
    "a_new_blank_one": ([(A, 1, 0, NORMAL)], [(key(9, 7), 5, 0, HSHOW)], -1),
}


def test_seg_active(weaver):
    names = list(ACTIVE)
    b = batch(weaver, [ACTIVE[n][0] for n in names], [ACTIVE[n][1] for n in names])
    exp = model_of(b)
    res = host_call(weaver, b)
    compare(res, exp)
    for d, n in enumerate(names):
        want = ACTIVE[n][2]
        s = int(res.tx_seg[d])
        if want is not None:
            assert int(res.maps.seg_active[s]) == want, n
    # the untouched key weave (token 1 of that collection) keeps its word
    d = names.index("an_untouched_key_weave")
    s = [i for i in range(len(res.maps.seg_key)) if res.maps.seg_coll[i] == d and res.maps.seg_key[i] == 1][0]
    assert int(res.maps.seg_active[s]) == 0


# --------------------------------------------------------- the full reweave
def test_base_shaped_batches_equal_the_full_reweave(weaver):
    rng = random.Random(31)
    colls = [gen_coll(rng, rng.choice([0, 3, 40, 100, 300]), wild=False) for _ in range(60)]
    b = batch(weaver, colls, [gen_tx(rng, c, rng.choice([1, 2, 3, 8]), 2000 + i, wild=False)
                              for i, c in enumerate(colls)])
    res = host_call(weaver, b)
    compare(res, model_of(b))
    assert not res.maps.status.any()
    reweave_equal(weaver, res)


def test_a_chain_of_twenty_calls(weaver):
    rng = random.Random(32)
    colls = [gen_coll(rng, n, wild=False) for n in (0, 1, 20, 64, 150)]
    b = batch(weaver, colls, [[] for _ in colls])
    cur = NS(off=b.off, idk=b.idk, ca=b.ca, ci=b.ci, kd=b.kd, val=b.val, segs=b.segs)
    for step in range(20):
        cut = lambda a, d: a[int(cur.off[d]):int(cur.off[d + 1])].tolist()
        rows = [list(zip(cut(cur.idk, d), cut(cur.ca, d), cut(cur.ci, d), cut(cur.kd, d)))
                for d in range(len(colls))]
        txs = [gen_tx(rng, r, rng.choice([0, 1, 2, 3]), 3000 + step, wild=False) for r in rows]
        toff, tid, tca, tci, tkd, tval = columns(txs)
        s = cur.segs
        exp = M.insert_maps(cur.off, cur.idk, cur.ca, cur.ci, cur.kd, s.seg_offsets, s.seg_coll, s.seg_key,
                            s.seg_active, s.seg_perm, toff, tid, tca, tci, tkd, cur.val, tval)
        res = abi_map_insert.insert_maps(weaver, (cur.off, cur.idk, cur.ca, cur.ci, cur.kd), s,
                                         (toff, tid, tca, tci, tkd, tval), coll_value=cur.val)
        compare(res, exp)
        reweave_equal(weaver, res)
        cur = NS(off=res.offsets, idk=res.id_key, ca=res.cause, ci=res.cause_is_id, kd=res.kind, val=res.value,
                 segs=res.maps)
    assert int(cur.off[-1]) > int(b.off[-1]) + 40


def test_render_of_the_result(weaver, big):
    res = host_call(weaver, big)
    D = len(big.off) - 1
    r = weaver.render_maps(D, res.maps.seg_coll, res.maps.seg_key, res.maps.seg_active)
    live = big.exp.seg_active >= 0
    same(r.key, big.exp.seg_key[live], "rendered keys")
    same(r.src, big.exp.seg_active[live].astype(U32), "rendered nodes")
    assert np.array_equal(np.diff(r.offsets.astype(I64)), np.bincount(big.exp.seg_coll[live], minlength=D))


# ---------------------------------------------------------------------- errors
def small_call():
    """A valid host call on two collections as raw structs, and what keeps them alive."""
    off, toff = np.array([0, 2, 2], U64), np.array([0, 1, 2], U64)
    idk, ca = np.array([key(1, 1), key(2, 1)], U64), np.array([1, 1], U64)
    ci, kd, val = np.zeros(2, U8), np.zeros(2, U8), np.array([5, 6], U64)
    so, sc, sk = np.array([0, 3], U64), np.zeros(1, U32), np.array([1], U64)
    sa, sp = np.array([1], I64), np.array([NONE, 1, 0], U32)
    tid, tca = np.array([key(3, 1), key(1, 2)], U64), np.array([key(2, 1), 4], U64)
    tci, tkd, tval = np.array([1, 0], U8), np.array([HHIDE, 0], U8), np.array([7, 8], U64)
    mb = abi.CwMapBatch(2, abi._u64p(off), abi._ptr(idk), abi._ptr(ca), abi._ptr(ci), abi._ptr(kd), 0, 0)
    b = abi_map_insert.CwMapInsertBatch(mb, 1, abi._ptr(so), abi._ptr(sc), abi._ptr(sk), abi._ptr(sa),
                                        abi._ptr(sp), abi._ptr(val), abi._u64p(toff), abi._ptr(tid),
                                        abi._ptr(tca), abi._ptr(tci), abi._ptr(tkd), abi._ptr(tval))
    noff, seg, pos = np.full(3, 77, U64), np.full(2, 77, U32), np.full(2, 77, U32)
    out, mr = abi._new_map_result(3, 4, 2)
    cols = [np.full(4, 77, U64), np.full(4, 77, U64), np.full(4, 77, U8), np.full(4, 77, U8), np.full(4, 77, U64)]
    r = abi_map_insert.CwMapInsertResult(abi._u64p(noff), abi._ptr(seg), abi._ptr(pos), mr, *map(abi._ptr, cols))
    keep = NS(ins=(off, toff, idk, ca, ci, kd, val, so, sc, sk, sa, sp, tid, tca, tci, tkd, tval), noff=noff,
              seg=seg, pos=pos, out=out, cols=cols)
    return b, r, keep


def set_path(s, path, value):
    *head, last = path.split(".")
    for p in head:
        s = getattr(s, p)
    setattr(s, last, value)


BAD = [
    ("b", "colls.coll_offsets", None, "required"), ("b", "tx_offsets", None, "required"),
    ("r", "new_offsets", None, "required"),
    ("b", "colls.coll_offsets", [1, 2, 2], "must be 0"), ("b", "colls.coll_offsets", [0, 3, 2], "monotone"),
    ("b", "tx_offsets", [1, 1, 2], "must be 0"), ("b", "tx_offsets", [0, 2, 1], "monotone"),
    ("b", "colls.id_key", None, "null input"), ("b", "colls.cause", None, "null input"),
    ("b", "colls.cause_is_id", None, "null input"), ("b", "colls.kind", None, "null input"),
    ("b", "seg_offsets", None, "null input"), ("b", "seg_coll", None, "null input"),
    ("b", "seg_key", None, "null input"), ("b", "seg_active", None, "null input"),
    ("b", "seg_perm", None, "null input"),
    ("b", "tx_id", None, "null tx"), ("b", "tx_cause", None, "null tx"), ("b", "tx_cause_is_id", None, "null tx"),
    ("b", "tx_kind", None, "null tx"),
    ("b", "coll_value", None, "go together"), ("b", "tx_value", None, "go together"),
    ("r", "id_key", None, "all four or none"), ("r", "cause_is_id", None, "all four or none"),
    ("r", "maps.seg_offsets", None, "null output"), ("r", "maps.seg_coll", None, "null output"),
    ("r", "maps.seg_key", None, "null output"), ("r", "maps.seg_active", None, "null output"),
    ("r", "maps.seg_perm", None, "null output"), ("r", "maps.status", None, "null output"),
    ("r", "maps.cap_segs", 2, "cap_segs"),
    ("m", None, 2, "memspace"), ("nb", None, None, "null batch"), ("nr", None, None, "null batch"),
]


@pytest.mark.parametrize("which,path,value,text", BAD, ids=[f"{w}-{p}-{i}" for i, (w, p, _, _) in enumerate(BAD)])
def test_error_returns_write_nothing_and_the_context_lives_on(weaver, which, path, value, text):
    L = abi_map_insert.lib()
    b, r, keep = small_call()
    if isinstance(value, list):
        value = np.array(value, U64)
        keep.extra = value
        value = abi._u64p(value)
    if which in ("b", "r"):
        set_path(b if which == "b" else r, path, value)
    rc = L.cw_insert_maps(weaver._h, None if which == "nb" else C.byref(b), None if which == "nr" else C.byref(r),
                          value if which == "m" else abi.CW_MEM_HOST)
    assert rc < 0 and text in L.cw_last_error(weaver._h).decode()
    assert (keep.noff == 77).all() and (keep.seg == 77).all() and (keep.pos == 77).all()
    assert not keep.out.seg_perm.any() and not keep.out.seg_key.any() and (keep.cols[0] == 77).all()
    # ... and the same structs, untouched, are a valid call
    b, r, keep = small_call()
    assert L.cw_insert_maps(weaver._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST) == 0
    assert keep.noff.tolist() == [0, 3, 4] and r.maps.n_segs == 2
    assert keep.out.seg_perm[:6].tolist() == [NONE, 1, 2, 0, NONE, 0]
    assert keep.seg.tolist() == [0, 1] and keep.pos.tolist() == [2, 1]
    assert keep.out.seg_active[:2].tolist() == [0, 0] and keep.out.seg_key[:2].tolist() == [1, 4]


def test_a_value_output_without_coll_value_is_an_error(weaver):
    L = abi_map_insert.lib()
    b, r, keep = small_call()
    b.coll_value = b.tx_value = None
    assert L.cw_insert_maps(weaver._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST) < 0
    assert "coll_value" in L.cw_last_error(weaver._h).decode()


# ------------------------------------------------------- the Python-level calls
def test_causal_insert_maps_and_map_weave_node():
    from cause_amd import causal as K
    from oracle import causal_ref as R
    rng = random.Random(4)
    sites = [R.new_site_id(rng) for _ in range(4)]
    conv = lambda v: {R.HIDE: K.HIDE, R.H_HIDE: K.H_HIDE, R.H_SHOW: K.H_SHOW}.get(v, v) \
        if isinstance(v, R.Keyword) else v
    ref = R.new_map_ct(site_id=sites[0], uuid="u" * 21)
    ct = K.new_map_ct(site_id=sites[0], uuid="u" * 21)

    def agree():
        assert set(ct["nodes"]) == set(ref["nodes"]) and ct["lamport_ts"] == ref["lamport_ts"]
        assert {k: [(n[0], n[1]) for n in w] for k, w in ct["weave"].items()} == \
            {k: [(n[0], n[1]) for n in w] for k, w in ref["weave"].items()}
        for k, w in ref["weave"].items():
            a, g = R.active_node(k, w), K.active_node(ct, k)
            assert (a is R.BLANK) == (g is K.BLANK) and (a is R.BLANK or a[0] == g[0])

    for step in range(30):
        tx = G.rand_tx(ref, rng, sites, rng.choice([1, 1, 2, 4]), first_ok=True)
        ktx = [(i, c, conv(v)) for i, c, v in tx]
        try:
            new = R.insert(R.map_weave, ref, tx[0], tx[1:])
        except R.CauseError as e:
            with pytest.raises(K.CauseError) as ke:
                K.insert_maps([(ct, ktx[0], ktx[1:])])
            assert ke.value.causes == e.causes
            continue
        ref = new
        if step % 2:
            ct = K.insert(K.map_weave_node, ct, ktx[0], ktx[1:])
        else:
            ct = K.insert_maps([(ct, ktx[0], ktx[1:])])[0]
        agree()
    again = next(iter(ct["nodes"].items()))
    assert K.insert_maps([(ct, (again[0],) + tuple(again[1]), None)])[0] is ct
    with pytest.raises(K.CauseError) as e:
        K.insert_maps([(ct, (again[0], "zzz", "other"), None)])
    assert "edits-not-allowed" in e.value.causes
    # map_assoc / map_dissoc through append(map_weave_node, ...)
    for k, v in [("k0", "x"), ("k9", "y"), ("k0", None), ("k9", "y"), ("k9", "z"), ("k0", "w"), ("nokey", None)]:
        if v is None:
            ref = R.map_dissoc(ref, k)
            ct = K.map_dissoc(ct, k, weave_fn=K.map_weave_node)
        else:
            ref = R.map_assoc(ref, k, v)
            ct = K.map_assoc(ct, k, v, weave_fn=K.map_weave_node)
        agree()
        assert K.map_get(ct, k) == R.map_get(ref, k)
