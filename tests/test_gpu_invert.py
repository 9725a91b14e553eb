"""cw_invert on the GPU (include/causeweave_invert.h, invert.hip) against
tests/invert_model.py: every output array, part_offsets, base_parts and status,
bit for bit, in host and device memory, on the LDS route and on the general
route (invert_cap = 1, or a base above the cap); the call errors; the parts
chained into cw_merge_lists / cw_merge_maps in device memory; and
cause_amd/base.py's undo_, redo_ and invert_bases end to end.
"""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import oracle
from cause_amd import abi, abi_invert, base as B, causal as CA, pack
from tests import invert_gen as G
from tests import invert_model as M
from tests.test_gpu_maps import gpu_maps, oracle_maps

pytestmark = pytest.mark.gpu

U8, U32, U64, I64 = np.uint8, np.uint32, np.uint64, np.int64
S, T = "QeVBlHoQFZSx0", "ZZremoteSite1"
TILE = 8192                      # k_invert_mark's tile (IV_TILE)
GENERAL, LDS_W, LDS_WG = "k_iv_runs", "k_invert_base_w", "k_invert_base_wg"
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "invert_cases.json")))


@pytest.fixture(scope="module")
def weaver():
    with abi.Weaver(0) as w:
        yield w


@pytest.fixture(scope="module")
def general():
    with abi.Weaver(0, options={"invert_cap": 1}) as w:
        yield w


def up(x):
    import torch

    signed = {np.dtype(U64): np.int64, np.dtype(U32): np.int32}.get(x.dtype)
    x = np.ascontiguousarray(x)
    if not len(x):
        x = np.zeros(1, x.dtype)
    return torch.from_numpy(x.view(signed) if signed else x).to(torch.device("cuda", 0))


def host_call(w, pk):
    return abi_invert.invert(w, *pk.args())


def device_call(w, pk, keep=False):
    """The device-memory call on torch tensors; an InvertResult of host copies.
    Every output element starts as 0x55: what lies past the parts must stay so."""
    import torch

    N, D, Gn = len(pk.id_key), len(pk.doc_offsets) - 1, len(pk.base_offsets) - 1
    g = [up(x) for x in (pk.id_key, pk.cause, pk.kind)]
    cii = None if pk.cause_is_id is None else up(pk.cause_is_id)
    ref = None if pk.ref_doc is None else up(pk.ref_doc)
    sel = [up(x) for x in (pk.sel_lo, pk.sel_hi, pk.sel_sites, pk.new_tx)]
    z = lambda n, dt: torch.full((max(n, 1),), 0x55, dtype=dt, device=g[0].device)
    o = {"inv_id": z(N, torch.int64), "inv_cause": z(N, torch.int64), "inv_kind": z(N, torch.uint8),
         "inv_src": z(N, torch.int32), "base_parts": z(Gn, torch.int32), "status": z(D, torch.int32)}
    if cii is not None:
        o["inv_cause_is_id"] = z(N, torch.uint8)
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    po = abi_invert.invert_device(w, pk.doc_offsets, [t.data_ptr() for t in g], pk.layout, pk.base_offsets,
                                  [t.data_ptr() for t in sel], {k: v.data_ptr() for k, v in o.items()},
                                  cause_is_id_ptr=None if cii is None else cii.data_ptr(),
                                  ref_doc_ptr=None if ref is None else ref.data_ptr())
    torch.cuda.synchronize()
    P = int(po[-1])
    dts = {"inv_id": U64, "inv_cause": U64, "inv_kind": U8, "inv_src": U32, "inv_cause_is_id": U8}
    h = {k: v.cpu().numpy().view(dts.get(k, U32)) for k, v in o.items()}
    for k in dts:
        if k in h:
            assert (h[k][P:N] == 0x55).all(), f"{k} written past the parts"
    res = abi_invert.InvertResult(po, h["inv_id"][:P], h["inv_cause"][:P],
                                  h["inv_cause_is_id"][:P] if cii is not None else None, h["inv_kind"][:P],
                                  h["inv_src"][:P], h["base_parts"][:Gn], h["status"][:D])
    return (res, o, g, cii) if keep else res


def routes(w, call):
    """(result, kernel stat names) of one call."""
    w.set_profiling(True)
    w.reset_kernel_stats()
    try:
        res = call()
        return res, set(w.kernel_stats())
    finally:
        w.set_profiling(False)


def check(w, pk, exp=None, device=True):
    exp = exp or M.invert_columns(*pk.args())
    M.same(host_call(w, pk), exp)
    if device:
        M.same(device_call(w, pk), exp)
    return exp


# ------------------------------------------------------------ random bases ----
@pytest.fixture(scope="module")
def random_batch():
    """64 bases of 1-5 collections, lists and maps mixed, 0-300 nodes each, refs
    between the collections of a base; the five slice kinds in rotation."""
    rng = random.Random(20261021)
    bases, slices, new_tx = G.gen_batch(rng, 64)
    pk = M.pack_bases(bases, slices, new_tx, tx_bits=G.TX_BITS)
    exp = M.invert_columns(*pk.args())
    assert int(exp.part_offsets[-1]) > 1000 and not exp.status.any()
    assert (exp.base_parts == 0).sum() >= 20 and (pk.ref_doc != M.U32_MAX).sum() > 50
    return pk, exp


def test_random_bases(weaver, random_batch):
    pk, exp = random_batch
    res, names = routes(weaver, lambda: host_call(weaver, pk))
    M.same(res, exp)
    assert {"k_invert_mark", "k_invert_compact", LDS_W, LDS_WG, "k_invert_write"} <= names and GENERAL not in names
    M.same(device_call(weaver, pk), exp)
    weaver.set_async(True)
    try:
        M.same(device_call(weaver, pk), exp)      # the offsets cached, one wait
    finally:
        weaver.set_async(False)


def test_the_same_batch_through_the_general_route(general, random_batch):
    pk, exp = random_batch
    res, names = routes(general, lambda: host_call(general, pk))
    M.same(res, exp)
    assert GENERAL in names and any(n.startswith("iv_sort") for n in names)
    M.same(device_call(general, pk), exp)


# ----------------------------------------------------------------- the cap ----
def test_a_base_above_the_cap_next_to_small_ones(weaver):
    """3 collections of 2,000 nodes reset over their whole history (about 6,000
    candidates): the call takes the general route, small neighbours included."""
    rng = random.Random(7)
    big, sites = G.gen_base(rng, [2000] * 3, 3, ref_rate=0.0)      # no collection of it is nested
    bases, slices, new_tx = G.gen_batch(rng, 6, max_nodes=80, kinds=("everything", "one_tx"))
    bases.insert(2, big), slices.insert(2, (None, None, None)), new_tx.insert(2, (10 ** 4, sites[0]))
    pk = M.pack_bases(bases, slices, new_tx, tx_bits=13)
    exp = M.invert_columns(*pk.args())
    lo, hi = (int(pk.doc_offsets[int(pk.base_offsets[g])]) for g in (2, 3))
    assert hi - lo > 6000 and (pk.ref_doc[lo:hi] == M.U32_MAX).all()       # every node of it is a candidate
    assert int(exp.base_parts[2]) > 4096 and exp.base_parts[[0, 4]].all() and not exp.status.any()
    res, names = routes(weaver, lambda: host_call(weaver, pk))
    M.same(res, exp)
    assert GENERAL in names
    M.same(device_call(weaver, pk), exp)


@pytest.mark.parametrize("n", [4096, 4097])
def test_exactly_at_and_above_the_cap(weaver, n):
    """n candidates in one base: value nodes and one hide under every other one
    (a value node and its hide share a key).  4,096: the workgroup in LDS;
    4,097: the general route."""
    half = n // 2
    nodes = [CA.ROOT_NODE] + [((1 + k, S, 0), CA.ROOT_ID, k) for k in range(n - half)]
    nodes += [((10000 + k, T, 0), (1 + 2 * k % (n - half), S, 0), CA.HIDE) for k in range(half)]
    small = [("s", "map", [((1, S, 0), "a", 1), ((2, S, 0), "a", CA.HIDE)])]
    pk = M.pack_bases([small, [("L", "list", nodes)], small], [(None, None, None)] * 3, [(20000, S)] * 3, tx_bits=13)
    exp = M.invert_columns(*pk.args())
    assert exp.base_parts.tolist() == [2, n - half, 2]
    res, names = routes(weaver, lambda: device_call(weaver, pk))
    M.same(res, exp)
    assert (GENERAL in names) == (n > 4096) and LDS_WG in names
    M.same(host_call(weaver, pk), exp)


# ------------------------------------------------------------- sharp edges ----
def line(n, site=S, t0=1):
    """A list of n value nodes under the root, ids ascending with the position."""
    return [CA.ROOT_NODE] + [((t0 + k, site, 0), CA.ROOT_ID, k) for k in range(n)]


def test_range_bounds_are_inclusive_and_the_root_is_not_selected(weaver, general):
    base = [("L", "list", line(6))]
    for w in (weaver, general):
        pk = M.pack_bases([base], [((2, S, 0), (4, S, 0), None)], [(9, S)], tx_bits=4)
        exp = check(w, pk)
        assert sorted(exp.inv_src.tolist()) == [2, 3, 4]
        pk = M.pack_bases([base], [(None, None, None)], [(9, S)], tx_bits=4)      # lo = 0: the root's id
        assert int(pk.sel_lo[0]) == 0 and pk.kind[0] == pack.KIND_ROOT
        exp = check(w, pk)
        assert sorted(exp.inv_src.tolist()) == [1, 2, 3, 4, 5, 6]
        pk.sel_lo[0], pk.sel_hi[0] = pk.id_key[3], pk.id_key[3]
        assert check(w, pk).inv_src.tolist() == [3]
        pk.sel_lo[0] = pk.id_key[3] + U64(1)
        assert len(check(w, pk).inv_src) == 0


def test_a_hidden_collection_emits_nothing_but_still_hides_its_child(weaver, general):
    a = [((1, S, 0), "x", M.ref("B")), ((2, S, 0), "y", 5)]
    b = [CA.ROOT_NODE, ((3, S, 0), CA.ROOT_ID, M.ref("C")), ((4, S, 0), CA.ROOT_ID, 1)]
    c = [((5, S, 0), "k", 1), ((6, S, 0), "k", 2)]
    d = [((7, S, 0), "k", 1)]
    base = [("A", "map", a), ("B", "list", b), ("C", "map", c), ("D", "map", d)]
    for w in (weaver, general):
        pk = M.pack_bases([base], [(None, None, None)], [(9, S)], tx_bits=4)
        exp = check(w, pk)
        assert exp.part_offsets.tolist() == [0, 2, 2, 2, 3]
        pk = M.pack_bases([base], [((3, S, 0), None, None)], [(9, S)], tx_bits=4)   # B's ref to C, not A's to B
        assert check(w, pk).part_offsets.tolist() == [0, 0, 2, 2, 3]


def test_a_ref_doc_outside_the_base_is_ignored(weaver, general):
    one = lambda u: [(u, "map", [((1, S, 0), "x", 1), ((2, S, 0), "y", 2)])]
    pk = M.pack_bases([one("A"), one("B"), one("C")], [(None, None, None)] * 3, [(9, S)] * 3, tx_bits=4)
    for w in (weaver, general):
        for r in (0, 2, 3, 0xFFFFFFFE):          # another base's document, n_docs, nearly UINT32_MAX
            pk.ref_doc[:] = M.U32_MAX
            pk.ref_doc[2] = r                     # a node of base 1 (document 1)
            assert check(w, pk).part_offsets.tolist() == [0, 2, 4, 6]
        pk.ref_doc[2] = 1                         # its own document: hidden
        assert check(w, pk).part_offsets.tolist() == [0, 2, 2, 4]


def test_token_and_id_collision(weaver, general):
    base = [("M", "map", [((1, S, 0), "a", 1), ((2, S, 0), "a", CA.HIDE), ((3, S, 0), (1, S, 0), CA.H_HIDE)])]
    pk = M.pack_bases([base], [((2, S, 0), (3, S, 0), None)], [(4, S)])
    pk.cause[1] = pk.id_key[0]
    for w in (weaver, general):
        exp = check(w, pk)
        assert exp.inv_cause_is_id.tolist() == [1, 0] and exp.inv_cause[0] == exp.inv_cause[1]


def test_null_cause_is_id_equals_a_column_of_ones(weaver):
    rng = random.Random(3)
    bases, slices, new_tx = [], [], []
    for g in range(12):
        n = rng.randint(0, 200)
        nodes = line(n, t0=1)
        nodes += [((300 + k, T, 0), nodes[rng.randint(1, n)][0], rng.choice([CA.HIDE, CA.H_HIDE, CA.H_SHOW]))
                  for k in range(n // 3)]
        bases.append([(f"L{g}", "list", nodes)])
        slices.append((None, None, None) if g % 2 else ((1 + n // 2, S, 0), None, None))
        new_tx.append((999, S))
    ones = M.pack_bases(bases, slices, new_tx, tx_bits=G.TX_BITS, refs=False)
    null = M.pack_bases(bases, slices, new_tx, tx_bits=G.TX_BITS, refs=False, lists_only=True)
    assert null.cause_is_id is None and ones.cause_is_id.all() and null.ref_doc is None
    e1, e0 = check(weaver, ones), check(weaver, null)
    assert e0.inv_cause_is_id is None and (e1.inv_cause_is_id == 1).all()
    e1.inv_cause_is_id = None
    M.same(e1, e0)


def test_more_parts_than_the_tx_field_holds(weaver, general):
    """3 tx bits: 9 parts do not fit; the neighbours are untouched."""
    nodes = [((1 + k, S, 0), f"k{k}", k) for k in range(9)]
    small = [("N", "map", [((1, S, 0), "a", 1)])]
    eight = [("E", "map", nodes[:8])]
    pk = M.pack_bases([small, [("M", "map", nodes), ("L", "list", line(2, T))], eight, small],
                      [(None, None, None)] * 4, [(12, S)] * 4, tx_bits=3)
    for w in (weaver, general):
        exp = check(w, pk)
        assert exp.status.tolist() == [0, abi.STATUS_KEY_RANGE, abi.STATUS_KEY_RANGE, 0, 0]
        assert exp.base_parts.tolist() == [1, 0, 8, 1] and exp.part_offsets.tolist() == [0, 1, 1, 1, 9, 10]


@pytest.mark.parametrize("first", [TILE - 1, TILE, TILE + 1])
def test_a_collection_across_the_tile_boundary(weaver, general, first):
    """Documents of first, 3 and TILE + 2 positions; the slice spans the ends of
    the first document and of the first tile."""
    docs = [("A", "list", line(first - 1, S, 1)), ("B", "list", line(2, S, 20000)),
            ("C", "list", line(TILE + 1, T, 1))]
    sl = ((first - 40, S, 0), (20001, S, 0), None)       # A's last nodes, B, and C's nodes in that range
    pk = M.pack_bases([docs[:2], docs[2:]], [sl, ((TILE - 30, T, 0), (TILE + 1, T, 0), None)], [(50000, S)] * 2,
                      tx_bits=8)
    for w in (weaver, general):
        exp = check(w, pk)
        assert exp.base_parts.tolist() == [first - (first - 40) + 2, 32]


@pytest.mark.parametrize("site_bits,n_sites", [(1, 1), (10, 150)])
def test_site_bits(weaver, general, site_bits, n_sites):
    """One and sixteen mask words a base; with 150 sites the ranks reach the third word."""
    rng = random.Random(site_bits)
    sites = sorted(CA._uid(rng, 13) for _ in range(n_sites))
    nodes = [((1 + k, sites[k % n_sites], 0), f"k{k % 7}", k) for k in range(400)]
    chosen = set(sites[::3])
    pk = M.pack_bases([[("M", "map", nodes)], [("N", "map", nodes)]],
                      [(None, None, chosen), ((100, sites[0], 0), None, set(sites) - chosen)],
                      [(500, sites[0])] * 2, tx_bits=9, site_bits=site_bits)
    assert pk.layout.site_bits == site_bits and len(pk.sel_sites) == 2 * abi_invert.mask_words(site_bits)
    for w in (weaver, general):
        exp = check(w, pk)
        assert int(exp.base_parts[0]) == sum(1 for n in nodes if n[0][1] in chosen)


def test_empty_batches(weaver):
    lay = pack.KeyLayout(8, 2, 4)
    z = lambda dt, n=0: np.zeros(n, dt)
    res = abi_invert.invert(weaver, [0], z(U64), z(U64), z(U8), z(U8), None, lay, [0], z(U64), z(U64), z(U64), z(U64))
    assert res.part_offsets.tolist() == [0] and len(res.status) == 0
    res = abi_invert.invert(weaver, [0, 0, 0], z(U64), z(U64), z(U8), None, None, lay, [0, 0, 2, 2], z(U64, 3),
                            z(U64, 3), z(U64, 3), z(U64, 3))
    assert res.part_offsets.tolist() == [0, 0, 0] and res.status.tolist() == [0, 0]
    assert res.base_parts.tolist() == [0, 0, 0]


# -------------------------------------------------------------- call errors ----
def raw_call(w, n_docs, off, cols, n_bases, boff, sel, outs, lay=(20, 18, 2), memspace=0, null=()):
    """cw_invert on structs built field by field (None = NULL); (rc, error text)."""
    L = abi_invert.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    q = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))
    b = abi_invert.CwInvertBatch(n_docs, q(off), *map(p, cols), *lay, 0, n_bases, q(boff), *map(p, sel))
    r = abi_invert.CwInvertResult(q(outs[0]), *map(p, outs[1:]))
    rc = L.cw_invert(w._h, None if "batch" in null else C.byref(b), None if "result" in null else C.byref(r),
                     memspace)
    return rc, L.cw_last_error(w._h).decode()


def test_call_errors_write_nothing(weaver):
    N, D, Gn = 6, 3, 2
    off, boff = np.array([0, 4, 4, 6], U64), np.array([0, 2, 3], U64)
    cols = [np.arange(N, dtype=U64) + U64(1 << 20), np.zeros(N, U64), np.zeros(N, U8), np.ones(N, U8),
            np.full(N, 0xFFFFFFFF, U32)]
    sel = [np.zeros(Gn, U64), np.full(Gn, 1 << 40, U64), np.full(Gn, 0xF, U64), np.full(Gn, 1 << 30, U64)]
    fresh = lambda: [np.full(D + 1, 0x55, U64), np.full(N, 0x55, U64), np.full(N, 0x55, U64), np.full(N, 0x55, U8),
                     np.full(N, 0x55, U8), np.full(N, 0x55, U32), np.full(Gn, 0x55, U32), np.full(D, 0x55, U32)]
    ok = dict(n_docs=D, off=off, cols=cols, n_bases=Gn, boff=boff, sel=sel)
    outs = fresh()
    rc, _ = raw_call(weaver, outs=outs, **ok)
    assert rc == 0 and outs[0].tolist() == [0, 4, 4, 6] and outs[6].tolist() == [4, 2]
    drop = lambda xs, k: [None if j == k else x for j, x in enumerate(xs)]
    bad = [dict(null=("batch",)), dict(null=("result",)),
           dict(off=None), dict(boff=None),
           dict(cols=drop(cols, 0)), dict(cols=drop(cols, 1)), dict(cols=drop(cols, 2)),
           dict(cols=drop(cols, 3)),                                  # cause_is_id null, inv_cause_is_id set
           dict(sel=drop(sel, 0)), dict(sel=drop(sel, 2)), dict(sel=drop(sel, 3)),
           dict(off=np.array([1, 4, 4, 6], U64)), dict(off=np.array([0, 5, 4, 6], U64)),
           dict(boff=np.array([1, 2, 3], U64)), dict(boff=np.array([0, 3, 2], U64)),
           dict(boff=np.array([0, 2, 2], U64)), dict(boff=np.array([0, 2, 4], U64)),
           dict(lay=(20, 18, 0)), dict(lay=(20, 18, 11)),
           dict(off=np.array([0, 4, 4, 0xFFFFFFFF], U64)),
           dict(memspace=2), dict(memspace=-1)]
    for change in bad:
        outs = fresh()
        rc, text = raw_call(weaver, outs=outs, **{**ok, **change})
        assert rc < 0 and text, change
        assert all((o == 0x55).all() for o in outs), change
    for k in (0, 1, 2, 4, 7):                                         # required outputs
        outs = fresh()
        rc, text = raw_call(weaver, outs=drop(outs, k), **ok)
        assert rc < 0 and text, k
        assert all((o == 0x55).all() for o in outs), k
    outs = fresh()
    assert raw_call(weaver, outs=drop(drop(outs, 5), 6), **ok)[0] == 0      # inv_src and base_parts may be null
    assert (outs[5] == 0x55).all() and outs[0].tolist() == [0, 4, 4, 6]


# -------------------------------------------------------------------- chain ----
def model_union(pk, exp, d):
    """Document d's old nodes and the model's parts, in id order: the columns."""
    a0, a1, p0, p1 = (int(x) for x in (pk.doc_offsets[d], pk.doc_offsets[d + 1], exp.part_offsets[d],
                                       exp.part_offsets[d + 1]))
    ci = np.ones(len(pk.id_key), U8) if pk.cause_is_id is None else pk.cause_is_id
    eci = np.ones(len(exp.inv_id), U8) if exp.inv_cause_is_id is None else exp.inv_cause_is_id
    cols = [np.concatenate([x[a0:a1], y[p0:p1]]) for x, y in
            ((pk.id_key, exp.inv_id), (pk.cause, exp.inv_cause), (ci, eci), (pk.kind, exp.inv_kind))]
    order = np.argsort(cols[0], kind="stable")
    return [c[order] for c in cols], order.astype(U32)


def test_chain_into_merge_lists_on_the_device(weaver):
    """cw_invert -> cw_merge_lists with the parts as side b and part_offsets as
    its offsets, no host copy of a node column: the oracle's reweave of old
    nodes + model parts."""
    import torch

    rng = random.Random(11)
    bases, slices, new_tx = [], [], []
    for g in range(24):
        n = rng.randint(1, 250)
        nodes = [CA.ROOT_NODE]
        for k in range(n):
            nodes.append(((1 + k, rng.choice([S, T]), 0), rng.choice(nodes[max(0, k - 5):])[0], k))
        vals = nodes[1:]
        nodes += [((400 + k, S, 0), rng.choice(vals)[0], rng.choice([CA.HIDE, CA.H_HIDE])) for k in range(n // 6)]
        bases.append([(f"L{g}", "list", nodes)])
        slices.append(((1 + n // 2, S, 0), None, None if g % 3 else {S}))
        new_tx.append((999, S))
    pk = M.pack_bases(bases, slices, new_tx, tx_bits=G.TX_BITS, refs=False, lists_only=True)
    exp = M.invert_columns(*pk.args())
    res, o, g, _ = device_call(weaver, pk, keep=True)
    M.same(res, exp)
    N, P, D = len(pk.id_key), int(res.part_offsets[-1]), len(pk.doc_offsets) - 1
    assert P > 200
    dev = g[0].device
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    w = {"weave_perm": z(N + P, torch.int32), "visible_bits": z((N + P + 31) // 32 + 1, torch.int32),
         "visible_count": z(D, torch.int32), "status": z(D, torch.int32)}
    src, va, vb = z(N + P, torch.int32), z(N, torch.int64), z(N, torch.int64)
    torch.cuda.synchronize()
    mo = weaver.merge_lists_device(pk.doc_offsets, [t.data_ptr() for t in g] + [va.data_ptr()], res.part_offsets,
                                   [o["inv_id"].data_ptr(), o["inv_cause"].data_ptr(), o["inv_kind"].data_ptr(),
                                    vb.data_ptr()], pk.layout, src.data_ptr(), {k: v.data_ptr() for k, v in w.items()})
    torch.cuda.synchronize()
    assert mo.tolist() == (pk.doc_offsets + exp.part_offsets).tolist()
    h = {k: v.cpu().numpy().view(U32) for k, v in w.items()}
    hsrc = src.cpu().numpy().view(U32)
    assert not h["status"][:D].any()
    for d in range(D):
        (uid, uc, _, uk), order = model_union(pk, exp, d)
        lo, hi = int(mo[d]), int(mo[d + 1])
        np.testing.assert_array_equal(hsrc[lo:hi], order)
        perm, vis, st = oracle.batch_lists(np.array([0, hi - lo], U64), uid, uc, uk, method=oracle.METHOD_LITERAL)
        assert not st.any()
        np.testing.assert_array_equal(h["weave_perm"][lo:hi], perm, err_msg=f"document {d}")
        bits = (h["visible_bits"][np.arange(lo, hi) >> 5] >> (np.arange(lo, hi) & 31).astype(U32)) & 1
        np.testing.assert_array_equal(bits.astype(U8), vis, err_msg=f"document {d}")


def test_chain_into_merge_maps_on_the_device(weaver):
    import torch

    rng = random.Random(12)
    bases, slices, new_tx = [], [], []
    for g in range(24):
        n = rng.randint(1, 120)
        nodes = []
        for k in range(n):
            r = rng.random()
            vals = [x for x in nodes if not CA._special(x[2])]
            if r < 0.15 and vals:
                node = (rng.choice(vals)[0], rng.choice([CA.H_HIDE, CA.H_SHOW]))
            elif r < 0.3:
                node = (rng.choice(G.KEYS), CA.HIDE)
            elif r < 0.35:
                node = (None, k)
            else:
                node = (rng.choice(G.KEYS), k)
            nodes.append(((1 + k, rng.choice([S, T]), 0),) + node)
        bases.append([(f"M{g}", "map", nodes)])
        slices.append(((1 + n // 2, S, 0), None, None if g % 3 else {S}))
        new_tx.append((999, S))
    pk = M.pack_bases(bases, slices, new_tx, tx_bits=G.TX_BITS, refs=False)
    exp = M.invert_columns(*pk.args())
    res, o, g, cii = device_call(weaver, pk, keep=True)
    M.same(res, exp)
    N, P, D = len(pk.id_key), int(res.part_offsets[-1]), len(pk.doc_offsets) - 1
    assert P > 100
    dev = g[0].device
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    cap = N + P
    w = {"seg_offsets": z(cap + 1, torch.int64), "seg_coll": z(cap, torch.int32), "seg_key": z(cap, torch.int64),
         "seg_active": z(cap, torch.int64), "seg_perm": z(N + P + cap, torch.int32), "status": z(D, torch.int32)}
    src, va, vb = z(N + P, torch.int32), z(N, torch.int64), z(N, torch.int64)
    tb = max(1, len(pk.tokens).bit_length())
    torch.cuda.synchronize()
    mo, ns = weaver.merge_maps_device(
        pk.doc_offsets, [g[0].data_ptr(), g[1].data_ptr(), cii.data_ptr(), g[2].data_ptr(), va.data_ptr()],
        res.part_offsets, [o["inv_id"].data_ptr(), o["inv_cause"].data_ptr(), o["inv_cause_is_id"].data_ptr(),
                           o["inv_kind"].data_ptr(), vb.data_ptr()], tb, 0, src.data_ptr(),
        {k: v.data_ptr() for k, v in w.items()}, cap)
    torch.cuda.synchronize()
    assert mo.tolist() == (pk.doc_offsets + exp.part_offsets).tolist()
    hv = lambda k, dt, n: w[k].cpu().numpy().view(dt)[:n]
    mr = abi.MapResult(hv("seg_offsets", U64, ns + 1), hv("seg_coll", U32, ns), hv("seg_key", U64, ns),
                       hv("seg_active", I64, ns), hv("seg_perm", U32, int(mo[-1]) + ns), hv("status", U32, D))
    assert not (mr.status & (abi.STATUS_DUP | abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL)).any()
    unions = [model_union(pk, exp, d)[0] for d in range(D)]
    cat = lambda k: np.concatenate([u[k] for u in unions])
    want = oracle_maps(mo, cat(0), cat(1), cat(2), cat(3))
    got = gpu_maps(mr, D)
    for d in range(D):
        assert got[d] == want[d], f"collection {d}"


# ------------------------------------------------------- base.py end to end ----
def play_txs(txs, seed=0):
    cb = B.new_cb(random.Random(seed))
    for tx in txs:
        cb = B.transact_(cb, [(cb["root_uuid"] if u == "root" else u, CA.ROOT_ID if c == "root-id" else c,
                               CA.HIDE if v == ":causal/hide" else v) for u, c, v in tx])
    return cb


@pytest.mark.parametrize("case", ["undo_redo_map", "undo_redo_list"])
def test_base_undo_and_redo(case):
    g = GOLDEN[case]
    cb = play_txs(g["txs"])

    def read(c):
        edn, c = B.cb_to_edn(c)
        return ({k: edn.get(k) for k in g["start"]} if case.endswith("map") else (edn or [None])[0]), c

    got, cb = read(cb)
    assert got == g["start"]
    for op, want in g["steps"]:
        cb = (B.undo_ if op == "undo" else B.redo_)(cb)
        got, cb = read(cb)
        assert got == want, (op, want)


def test_base_invert_of_the_whole_history():
    g = GOLDEN["invert"]
    cb = play_txs(g["txs"])
    edn, cb = B.cb_to_edn(cb)
    assert edn["a"] == g["a_before"] and len(cb["history"]) == g["history_before"]
    out = B.invert_(cb, cb["history"])
    edn, out = B.cb_to_edn(out)
    assert edn.get("a") is g["a_after"] and len(out["history"]) == g["history_after"]
    model = B.invert_(cb, cb["history"], invert_fn=M.invert_columns)
    assert out["history"] == model["history"]


def test_base_invert_bases_equals_single_calls():
    rng = random.Random(5)
    cbs = []
    for g in range(32):
        cb = B.new_cb(random.Random(100 + g))
        cb = B.transact_(cb, [(None, None, {"a": 1, "l": [1, 2, 3], "m": {"x": 1}})])
        for step in range(rng.randint(1, 6)):
            cb = B.transact_(cb, [(cb["root_uuid"], rng.choice("abcd"), rng.choice([step, CA.HIDE, [step, 7]]))])
        cbs.append(cb)
    slices = [B.subhis(cb, (rng.randint(1, cb["lamport_ts"] - 1), cb["site_id"]), None) for cb in cbs]
    many = B.invert_bases(cbs, slices)
    for cb, sl, got in zip(cbs, slices, many):
        one = B.invert_(cb, sl)
        assert got["history"] == one["history"] and len(got["history"]) > len(cb["history"])
        assert {u: ct["nodes"] for u, ct in got["collections"].items()} == \
            {u: ct["nodes"] for u, ct in one["collections"].items()}
        assert B.cb_to_edn(got)[0] == B.cb_to_edn(one)[0]
