"""cw_render_bases on the GPU (include/causeweave_render_bases.h, renderbase.hip)
against tests/renderbase_model.py: every output array, bit for bit, in host and
device memory, with guard words past the tokens and past the capacity; the
count-only call; the call errors; the chain cw_weave_* -> cw_render_* ->
cw_render_bases in device memory; and cause_amd/base.py's bases_to_edn end to end.
"""
import ctypes as C
import random

import numpy as np
import pytest

from cause_amd import abi, abi_render_bases as A, base as B, pack
from tests import renderbase_gen as G
from tests import renderbase_model as M

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
NONE = A.U32_MAX
TILE = 8192                      # k_rb_compact's tile (RB_TILE)
GUARD = 16
KERNELS = {"k_rb_roots", "k_rb_link", "k_rb_compact", "k_rb_bound", "k_rb_tour", "k_rb_jump", "k_rb_docs",
           "k_rb_size", "k_rb_place", "k_rb_emit"}


@pytest.fixture(scope="module")
def weaver():
    with abi.Weaver(0) as w:
        yield w


def up(x):
    import torch

    signed = {np.dtype(U64): np.int64, np.dtype(U32): np.int32}.get(x.dtype)
    x = np.ascontiguousarray(x)
    if not len(x):
        x = np.zeros(1, x.dtype)
    return torch.from_numpy(x.view(signed) if signed else x).to(torch.device("cuda", 0))


def device_call(w, off, ref, root, tokens=True, optional=True):
    """The device-memory call on torch tensors; a RenderBasesResult of host
    copies.  Every output element starts as 0x55: what lies past the tokens,
    and the guard words past each array's capacity, must stay so."""
    import torch

    off, ref, root = np.asarray(off, U64), np.asarray(ref, U32), np.asarray(root, U32)
    D, Gn, E = len(off) - 1, len(root), len(ref)
    cap = E + 2 * D
    g_ref, g_root = up(ref), up(root)
    z = lambda n, dt: torch.full((n + GUARD,), 0x55, dtype=dt, device=g_ref.device)
    o = {"base_status": z(Gn, torch.int32)}
    if tokens:
        o.update(tok_kind=z(cap, torch.uint8), tok_doc=z(cap, torch.int32), tok_entry=z(cap, torch.int32))
    if optional:
        o.update(doc_base=z(D, torch.int32), doc_open=z(D, torch.int32))
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    bo = A.render_bases_device(w, off, g_ref.data_ptr() if E else None, Gn, g_root.data_ptr() if Gn else None,
                               {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    T = int(bo[-1])
    h = {k: v.cpu().numpy().view(U8 if k == "tok_kind" else U32) for k, v in o.items()}
    sizes = {"base_status": Gn, "tok_kind": T, "tok_doc": T, "tok_entry": T, "doc_base": D, "doc_open": D}
    for k, a in h.items():
        assert (a[sizes[k]:] == 0x55).all(), f"{k} written past its end"
    cut = lambda k: h[k][:sizes[k]] if k in h else None
    return A.RenderBasesResult(bo, cut("tok_kind"), cut("tok_doc"), cut("tok_entry"), cut("base_status"),
                               cut("doc_base"), cut("doc_open"))


def check(w, off, ref, root, exp=None):
    """Host, device and count-only calls against the model; the model's result."""
    exp = exp or M.render_columns(off, ref, root)
    M.same(A.render_bases(w, off, ref, root), exp)
    M.same(device_call(w, off, ref, root), exp)
    M.same(A.render_bases(w, off, ref, root, tokens=False), exp, tokens=False)
    got = device_call(w, off, ref, root, tokens=False, optional=False)
    np.testing.assert_array_equal(got.base_tok_offsets, exp.base_tok_offsets)
    np.testing.assert_array_equal(got.base_status, exp.base_status)
    return exp


def table(docs, root):
    """docs: one list of refs (NONE = a scalar) a document."""
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(U64)
    return off, np.array([x for d in docs for x in d], U32), np.array(root, U32)


# ----------------------------------------------------------------- forests ----
def test_random_forests_and_the_kernel_names(weaver):
    """Thousands of documents in one tile; bases in another order than their documents."""
    rng = random.Random(20261021)
    off, ref, root = M.random_table(rng, 5000, 300, p_wild=0.02)
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        exp = check(weaver, off, ref, root)
        assert KERNELS <= set(weaver.kernel_stats())
    finally:
        weaver.set_profiling(False)
    small = M.render_recursive(off, ref, root)
    M.same(exp, small)
    assert (exp.base_status == 0).sum() > 100 and (exp.base_status != 0).sum() > 10
    assert int(off[-1]) < TILE and int(exp.base_tok_offsets[-1]) > 1000
    weaver.set_async(True)
    try:
        M.same(device_call(weaver, off, ref, root), exp)      # the offsets cached, one wait
    finally:
        weaver.set_async(False)


def test_a_document_across_three_tiles_with_tree_refs_in_each(weaver):
    """Document 1 holds 3 * TILE - 7 entries; children (some with children of
    their own) hang off entries of every tile, the tile's first and last among them."""
    n = 3 * TILE - 7
    big = [NONE] * n
    docs = [[NONE, NONE, NONE], big]
    at = [3, 4, TILE - 1, TILE, TILE + 5, 2 * TILE - 1, 2 * TILE, 2 * TILE + 100, n + 2]      # batch-wide entries
    for p in at:                      # (document 1 starts at entry 3)
        big[p - 3] = len(docs)
        docs.append([NONE] * (p % 3) + [len(docs) + 1] + [NONE] * (p % 2))
        docs.append([] if p % 2 else [NONE, NONE - 1])          # a ref to nothing in some
    off, ref, root = table(docs, [1, 0])
    assert [int(off[1]) + p - 3 for p in at] == [p for p in at] and int(off[2]) == n + 3
    exp = check(weaver, off, ref, root)
    assert not exp.base_status.any() and (exp.doc_base[1:] == 0).all() and exp.doc_base[0] == 1
    assert int(exp.base_tok_offsets[1]) == sum(len(d) + 2 for d in docs[1:]) - 2 * len(at)


def test_empty_documents_everywhere(weaver):
    """Empty documents as root, as child, first, last and adjacent."""
    docs = [[], [], [0, 1, NONE, 6], [], [], [3], [], []]
    exp = check(weaver, *table(docs, [2, 4, 7, 5]))
    assert exp.base_tok_offsets.tolist() == [0, 9, 11, 13, 17] and not exp.base_status.any()
    M.same(exp, M.render_recursive(*table(docs, [2, 4, 7, 5])))


def test_one_document_with_20000_ref_entries(weaver):
    """Sibling links across tiles: every entry of the root is a tree ref."""
    n = 20000
    docs = [list(range(1, n + 1))] + [[NONE] * (k % 3) for k in range(n)]
    exp = check(weaver, *table(docs, [0]))
    assert int(exp.base_tok_offsets[1]) == 2 + 2 * n + sum(k % 3 for k in range(n))
    docs[0][12345] = 7                # one collection referred to twice
    exp = check(weaver, *table(docs, [0]))
    assert exp.base_status.tolist() == [A.STATUS_REF_SHARED] and int(exp.base_tok_offsets[1]) == 0


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 5000])
def test_chains(weaver, n):
    """n nested single-entry documents (tour lengths on both sides of a power of
    two), numbered children first, next to a second base in document order."""
    off = np.arange(2 * n + 1, dtype=U64)
    ref = np.array([NONE] + list(range(n - 1)) + list(range(n + 1, 2 * n)) + [NONE], U32)
    exp = check(weaver, off, ref, [n - 1, n])
    assert exp.base_tok_offsets.tolist() == [0, 2 * n + 1, 4 * n + 2]
    assert exp.doc_open[:n].tolist() == list(range(n - 1, -1, -1))


def test_more_than_130_tiles_with_64_tiles_without_a_ref(weaver):
    """The look-back passes more than one window of tiles that count nothing."""
    E = 134 * TILE + 77
    rng = np.random.default_rng(5)
    ref = np.full(E, NONE, U32)
    n_small = 3000
    sizes = rng.integers(0, 4, n_small)
    big = E - int(sizes.sum())
    off = np.concatenate([[0, big], big + np.cumsum(sizes)]).astype(U64)
    free = list(rng.permutation(np.arange(1, n_small + 1)))
    where = np.concatenate([rng.choice(30 * TILE, 1200, replace=False), 100 * TILE + rng.choice(30 * TILE, 1200,
                                                                                              replace=False)])
    for e in np.sort(where):
        ref[e] = free.pop()
    for e in range(big, E):           # the small documents nest, too
        if free and rng.random() < 0.3:
            ref[e] = free.pop()
    assert (ref[30 * TILE:100 * TILE] == NONE).all()
    exp = check(weaver, off, ref, [0])
    assert exp.base_status.tolist() == [0] and int(exp.base_tok_offsets[1]) > big + 4000


def test_refs_that_name_no_document(weaver):
    """n_docs and UINT32_MAX - 1 are nil, UINT32_MAX is a scalar."""
    docs = [[3, NONE - 1, NONE, 1, 4], [NONE, 3], [NONE]]
    exp = check(weaver, *table(docs, [0, 3, NONE, NONE - 1]))
    assert exp.tok_kind.tolist() == [0, 3, 3, 2, 0, 2, 3, 1, 3, 1]
    assert exp.base_tok_offsets.tolist() == [0, 10, 10, 10, 10] and not exp.base_status.any()
    assert exp.doc_base.tolist() == [0, 0, NONE]


@pytest.mark.parametrize("off,ref,root,status", M.SHARED_CASES)
def test_shared_and_cycles(weaver, off, ref, root, status):
    exp = check(weaver, off, ref, root)
    assert exp.base_status.tolist() == status
    M.same(exp, M.render_recursive(off, ref, root))


def test_an_isolated_cycle_flags_no_one(weaver):
    docs = [[NONE, 3], [2], [1], [NONE]] + [[4 + (k + 1) % 700] for k in range(700)]      # a cycle of 2 and one of 700
    exp = check(weaver, *table(docs, [0]))
    assert exp.base_status.tolist() == [0] and exp.doc_base.tolist() == [0, NONE, NONE, 0] + [NONE] * 700


# ------------------------------------------------------- sizes and contexts ----
def test_empty_batches(weaver):
    z = np.zeros(0, U32)
    for off, ref, root in (([0], z, z), ([0], z, [0, 5]), ([0, 0, 0], z, z), ([0, 0, 0], z, [1, 0, 7]),
                           ([0, 2], [NONE, 5], z)):
        exp = check(weaver, off, ref, root)
        assert int(exp.base_tok_offsets[-1]) == (4 if len(root) == 3 else 0)


def test_growing_and_shrinking_calls_on_one_context():
    rng = random.Random(3)
    with abi.Weaver(0) as w:
        for D, Gn in ((10, 2), (5000, 40), (50, 50), (30000, 500), (1, 1), (30000, 500), (700, 3)):
            off, ref, root = M.random_table(rng, D, Gn, p_wild=0.01)
            exp = M.render_columns(off, ref, root)
            M.same(A.render_bases(w, off, ref, root), exp)
            M.same(device_call(w, off, ref, root), exp)


# -------------------------------------------------------------- call errors ----
def raw_call(w, n_docs, off, ref, n_bases, root, outs, memspace=0, null=()):
    """cw_render_bases on structs built field by field (None = NULL); (rc, error text)."""
    L = A.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    q = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint64))
    b = A.CwRenderBasesBatch(n_docs, q(off), p(ref), n_bases, p(root))
    r = A.CwRenderBasesResult(q(outs[0]), *map(p, outs[1:]))
    rc = L.cw_render_bases(w._h, None if "batch" in null else C.byref(b), None if "result" in null else C.byref(r),
                           memspace)
    return rc, L.cw_last_error(w._h).decode()


def test_call_errors_write_nothing(weaver):
    D, Gn, E = 3, 2, 4
    off, ref, root = np.array([0, 3, 3, 4], U64), np.array([NONE, 2, 9, NONE], U32), np.array([0, 5], U32)
    cap = E + 2 * D
    fresh = lambda: [np.full(Gn + 1, 0x55, U64), np.full(cap, 0x55, U8), np.full(cap, 0x55, U32),
                     np.full(cap, 0x55, U32), np.full(Gn, 0x55, U32), np.full(D, 0x55, U32), np.full(D, 0x55, U32)]
    ok = dict(n_docs=D, off=off, ref=ref, n_bases=Gn, root=root)
    outs = fresh()
    rc, _ = raw_call(weaver, outs=outs, **ok)
    assert rc == 0 and outs[0].tolist() == [0, 7, 7] and outs[4].tolist() == [0, 0]
    drop = lambda xs, k: [None if j == k else x for j, x in enumerate(xs)]
    bad = [dict(null=("batch",)), dict(null=("result",)), dict(off=None), dict(ref=None), dict(root=None),
           dict(off=np.array([1, 3, 3, 4], U64)), dict(off=np.array([0, 3, 2, 4], U64)),
           dict(off=np.array([0, 3, 3, 0xFFFFFFFF - 6], U64)),           # E + 2 * n_docs = 2^32 - 1
           dict(off=np.array([0, 3, 3, 0xFFFFFFFF], U64)),
           dict(n_docs=0x7FFFFFFF), dict(n_bases=0xFFFFFFFF),
           dict(memspace=2), dict(memspace=-1)]
    for change in bad:
        outs = fresh()
        rc, text = raw_call(weaver, outs=outs, **{**ok, **change})
        assert rc < 0 and text, change
        assert all((o == 0x55).all() for o in outs), change
    for ks in ((0,), (4,), (1,), (2, 3), (1, 3)):                     # required outputs; only some token arrays
        outs = fresh()
        given = outs
        for k in ks:
            given = drop(given, k)
        rc, text = raw_call(weaver, outs=given, **ok)
        assert rc < 0 and text, ks
        assert all((o == 0x55).all() for o in outs), ks
    outs = fresh()
    assert raw_call(weaver, outs=drop(drop(outs, 5), 6), **ok)[0] == 0      # doc_base and doc_open may be null
    assert (outs[5] == 0x55).all() and (outs[6] == 0x55).all() and outs[0].tolist() == [0, 7, 7]
    M.same(A.render_bases(weaver, off, ref, root), M.render_recursive(off, ref, root))   # the context lives on


# -------------------------------------------------------------------- chain ----
@pytest.fixture(scope="module")
def cbs():
    """The CPU tests' bases: the reference's known answers, plain nested values,
    undo and redo, a transacted ref (flagged) and a ref to nothing."""
    known = [cb for cb, _ in G.known_answers()]
    cb = B.transact_(G.cb0(3), [[None, None, {"a": [1, 2], "b": {"c": 3}}]])
    inner = [u for u, ct in cb["collections"].items() if ct["type"] == "list"][0]
    twice = B.transact_(cb, [[cb["root_uuid"], "again", B.uuid_to_ref(inner)]])
    gone = B.transact_(cb, [[cb["root_uuid"], "gone", B.uuid_to_ref("no-such-collection")]])
    return known + G.random_bases(7, 40, history=False) + [twice, gone] + G.random_bases(11, 40)


def test_bases_to_edn_equals_cb_to_edn(cbs):
    want = [B.cb_to_edn(cb)[0] for cb in cbs]
    assert B.bases_to_edn(cbs) == want
    assert want[:len(G.known_answers())] == [v for _, v in G.known_answers()]
    seen = []

    def spy(*args):
        seen.append(B._gpu_render_bases(*args))
        M.same(seen[-1], M.render_columns(*args))
        return seen[-1]

    assert B.bases_to_edn(cbs, render_fn=spy) == want
    st = seen[0].base_status
    assert (st != 0).sum() == 1 and len(st) == len(cbs)            # only the transacted ref is flagged


def test_the_chain_in_device_memory(weaver, cbs):
    """cw_weave_lists -> cw_render_lists(value = the ref column), cw_weave_maps ->
    cw_render_maps, then cw_render_bases on the two rendered value columns laid
    one after the other: lists first, then maps, the bases interleaved; no
    array comes to the host in between (the offsets are host arrays by contract)."""
    import torch

    docs, n_lists, index, roots = B._collect_docs(cbs)
    refs = B._ref_column(docs, index)
    exp_off, exp_ref, _, _ = B._gpu_entries(docs, n_lists, refs)      # the host-memory calls
    exp = M.render_columns(exp_off, exp_ref, roots)
    lists, maps = [n for _, _, n in docs[:n_lists]], [n for _, _, n in docs[n_lists:]]
    assert n_lists > 50 and len(maps) > 50
    assert sorted({g for g, _, _ in docs[:n_lists]} & {g for g, _, _ in docs[n_lists:]})      # bases with both kinds
    b, pm = pack.pack_lists(lists), pack.pack_maps(maps)
    NL, NM, D = len(b.id_key), len(pm.id_key), len(docs)
    dev = torch.device("cuda", 0)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    g_ref = up(refs)
    gl = [up(x) for x in (b.id_key, b.cause_key, b.kind)]
    lo = {"weave_perm": z(NL, torch.int32), "visible_bits": z((NL + 31) // 32, torch.int32),
          "visible_count": z(n_lists, torch.int32), "status": z(n_lists, torch.int32)}
    gm = [up(x) for x in (pm.id_key, pm.cause, pm.cause_is_id, pm.kind)]
    mo = {"seg_offsets": z(NM + 1, torch.int64), "seg_coll": z(NM, torch.int32), "seg_key": z(NM, torch.int64),
          "seg_active": z(NM, torch.int64), "seg_perm": z(2 * NM, torch.int32), "status": z(len(maps), torch.int32)}
    ent = z(NL + NM, torch.int32)                                     # the entry table's ref column
    torch.cuda.synchronize()
    weaver.weave_lists_device(b.offsets, *[t.data_ptr() for t in gl], b.layout, {k: v.data_ptr() for k, v in lo.items()})
    l_off = weaver.render_lists_device(b.offsets, lo["weave_perm"].data_ptr(), lo["visible_bits"].data_ptr(),
                                       value_ptr=g_ref.data_ptr(), value_size=4, out_value_ptr=ent.data_ptr())
    RL = int(l_off[-1])
    S = weaver.weave_maps_device(pm.offsets, [t.data_ptr() for t in gm], pm.token_bits, pm.layout.key_bits,
                                 {k: v.data_ptr() for k, v in mo.items()}, max(NM, 1))
    m_off = weaver.render_maps_device(len(maps), S, mo["seg_coll"].data_ptr(), mo["seg_key"].data_ptr(),
                                      mo["seg_active"].data_ptr(), coll_offsets=pm.offsets,
                                      value_ptr=g_ref.data_ptr() + 4 * NL, value_size=4,
                                      out_value_ptr=ent.data_ptr() + 4 * RL)
    ent_off = np.concatenate([l_off, m_off[1:] + l_off[-1]])
    np.testing.assert_array_equal(ent_off, exp_off)
    E = int(ent_off[-1])
    cap = E + 2 * D
    g_root = up(roots)
    o = {"tok_kind": z(cap, torch.uint8), "tok_doc": z(cap, torch.int32), "tok_entry": z(cap, torch.int32),
         "base_status": z(len(cbs), torch.int32), "doc_base": z(D, torch.int32), "doc_open": z(D, torch.int32)}
    bo = A.render_bases_device(weaver, ent_off, ent.data_ptr(), len(cbs), g_root.data_ptr(),
                               {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    T = int(bo[-1])
    h = {k: v.cpu().numpy().view(U8 if k == "tok_kind" else U32) for k, v in o.items()}
    got = A.RenderBasesResult(bo, h["tok_kind"][:T], h["tok_doc"][:T], h["tok_entry"][:T],
                              h["base_status"][:len(cbs)], h["doc_base"][:D], h["doc_open"][:D])
    M.same(got, exp)
    np.testing.assert_array_equal(ent.cpu().numpy().view(U32)[:E], exp_ref)
