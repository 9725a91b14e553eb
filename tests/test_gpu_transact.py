"""cw_transact on the GPU (include/causeweave_transact.h, transact.hip) against
tests/transact_model.py: every output array, bit for bit, in host and device
memory, with 0x55 guards past M, past C and past the capacities; the count-only
call; the async call; the call errors; cw_transact -> cw_weave_lists /
cw_weave_maps in device memory; and cause_amd/base.py's transact_bases end to end.
"""
import random

import numpy as np
import pytest

from cause_amd import abi, abi_transact as A, base as B, pack
from tests import transact_model as M

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
TILE = 2048                      # the kernels' tile (TX_TILE)
GUARD = 16
NIL = M.NIL
LEAF, STR, OPEN_LIST, OPEN_MAP, CLOSE, PART, ROOT_LIST, ROOT_MAP = range(8)
CAP = 4096                       # the default and the most of transact_cap (TX_CAP)
KERNELS = {"k_tx_scan", "k_tx_level", "k_tx_sort_wg", "k_tx_rank", "k_tx_group", "k_tx_count", "k_tx_bases", "k_tx_runs",
           "k_tx_docoff", "k_tx_expand", "k_tx_news"}
LAY = pack.KeyLayout(20, 4, 24)
TORCH = {np.dtype(U8): "uint8", np.dtype(U32): "int32", np.dtype(U64): "int64"}


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


def batch(streams, docs=(), layout=LAY, new_tx=None):
    """streams: one list of (kind, arg, cause, cii[, vkind]) a base; docs: one
    list of doc_is_map a base -> transact's arguments after the Weaver."""
    docs = list(docs) or [[] for _ in streams]
    toks = [tuple(t) + (0,) * (5 - len(t)) for s in streams for t in s]
    col = lambda k, dt: np.array([t[k] for t in toks], dt)
    ntx = [layout.pack(7 + g, g % 16, 0) for g in range(len(streams))] if new_tx is None else new_tx
    return dict(base_doc_offsets=np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(U64),
                doc_is_map=np.array([x for d in docs for x in d], U8), layout=layout, new_tx=np.array(ntx, U64),
                tok_offsets=np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(U64),
                tok_kind=col(0, U8), tok_arg=col(1, U32), tok_cause=col(2, U64), tok_cause_is_id=col(3, U8),
                tok_vkind=col(4, U8))


def device_call(w, b, exp, nodes=True, slack=0, vkind=True):
    """The device-memory call on torch tensors -> a TransactResult of host copies.
    Every output element starts as 0x55: what lies past M, past C and past the
    capacities (the model's counts + slack) must stay so."""
    import torch

    C, Mn = int(exp.base_new_offsets[-1]), int(exp.base_node_offsets[-1])
    G, T = len(b["new_tx"]), len(b["tok_kind"])
    new_cap, node_cap = C + slack, Mn + slack
    dev = torch.device("cuda", 0)
    z = lambda n, dt: torch.full((n + GUARD,), 0x55, dtype=getattr(torch, TORCH[np.dtype(dt)]), device=dev)
    o = {"root_doc": z(G, U32), "base_status": z(G, U32)}
    if nodes:
        o.update({f: z(node_cap, dt) for f, dt in A.NODE_COLUMNS})
        o.update({f: z(new_cap, dt) for f, dt in A.NEW_COLUMNS})
    ins = [up(b[f]) for f in ("tok_kind", "tok_arg", "tok_cause", "tok_cause_is_id", "tok_vkind")]
    g_map, g_tx = up(b["doc_is_map"]), up(b["new_tx"])
    ptrs = [x.data_ptr() if T else None for x in ins]
    if not vkind:
        ptrs[4] = None
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    bn, bm, no = A.transact_device(w, b["base_doc_offsets"], g_map.data_ptr() if len(b["doc_is_map"]) else None,
                                   b["layout"], g_tx.data_ptr() if G else None, b["tok_offsets"], ptrs, new_cap,
                                   node_cap, {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    dts = dict(A.NODE_COLUMNS + A.NEW_COLUMNS + (("root_doc", U32), ("base_status", U32)))
    h = {k: v.cpu().numpy().view(dts[k]) for k, v in o.items()}
    sizes = {**{f: Mn for f, _ in A.NODE_COLUMNS}, **{f: C for f, _ in A.NEW_COLUMNS}, "root_doc": G, "base_status": G}
    for k, a in h.items():
        assert (a[sizes[k]:] == 0x55).all(), f"{k} written past its end"
    assert (no[len(b["doc_is_map"]) + C:] == Mn).all()       # the entries past the last collection repeat M
    cut = lambda k: h[k][:sizes[k]] if k in h else None
    return A.TransactResult(bn, bm, no[:len(b["doc_is_map"]) + C + 1], *[cut(f) for f, _ in A.NODE_COLUMNS],
                            *[cut(f) for f, _ in A.NEW_COLUMNS], cut("root_doc"), cut("base_status"))


def counts_only(exp):
    return A.TransactResult(**{f: None if f.startswith(("node_", "new_")) and f != "node_offsets" else getattr(exp, f)
                               for f in A.TransactResult.__dataclass_fields__})


def check(w, b, exp=None):
    """Host, device and count-only calls against the model; the model's result."""
    exp = exp or M.transact_columns(**b)
    assert M.same(A.transact(w, **b), exp) == []
    assert M.same(device_call(w, b, exp), exp) == []
    assert M.same(device_call(w, b, exp, slack=5), exp) == []
    C = int(exp.base_new_offsets[-1])
    assert M.same(A.transact(w, **b, new_cap=C, nodes=False), counts_only(exp)) == []
    assert M.same(device_call(w, b, exp, nodes=False), counts_only(exp)) == []
    return exp


def leaf(cause=0, cii=1, vkind=0):
    return (LEAF, 0, cause, cii, vkind)


END = (CLOSE, 0, 0, 0)


# ------------------------------------------------------------ random batches ----
def test_random_bases_and_the_kernel_names(weaver):
    rng = random.Random(20261021)
    b = M.random_batch(rng, 2000, budget=60, depth=6, p_bad=0.1)
    assert max(np.diff(b["tok_offsets"])) <= 130
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        exp = check(weaver, b)
        assert KERNELS <= set(weaver.kernel_stats())
    finally:
        weaver.set_profiling(False)
    assert (exp.base_status == 0).sum() > 1500 and (exp.base_status == A.STATUS_TX_MALFORMED).sum() > 50
    assert int(exp.base_node_offsets[-1]) > 10000 and int(exp.base_new_offsets[-1]) > 2000
    assert M.same(M.transact_recursive(**b), exp) == []
    # the async call: the same arrays.  (The library has no counter of its waits, so "one wait" is not
    # observed here: what is checked is that the call's results are complete when it returns its offsets
    # and the stream has been waited for.)
    weaver.set_async(True)
    try:
        assert M.same(device_call(weaver, b, exp), exp) == []
    finally:
        weaver.set_async(False)
    nov = dict(b, tok_vkind=None)
    assert M.same(device_call(weaver, b, M.transact_columns(**nov), vkind=False), M.transact_columns(**nov)) == []


def test_one_base_across_three_tiles(weaver):
    """3 * TILE - 7 tokens: groups that open in one tile and close in another,
    STR tokens at a tile's first and last position."""
    n = 3 * TILE - 7
    toks = [None] * n
    toks[0], toks[n - 1] = (ROOT_LIST, 0, 0, 1), END
    spans = [(5, TILE + 9, OPEN_LIST), (TILE - 2, TILE + 1, OPEN_MAP), (TILE + 20, 2 * TILE + 3, OPEN_MAP),
             (2 * TILE - 1, 2 * TILE, OPEN_LIST), (2 * TILE + 10, n - 2, OPEN_LIST)]
    # (the second and fourth nest inside the first and third)
    for lo, hi, k in spans:
        toks[lo], toks[hi] = (k, 0, 3, 0), END
    for p in (TILE - 1, TILE, 2 * TILE - 2, 2 * TILE + 1, 1, n - 3):
        if toks[p] is None:
            toks[p] = (STR, 3, 4, 0)
    toks = [leaf(9, 0, i % 4) if t is None else t for i, t in enumerate(toks)]
    exp = check(weaver, batch([toks]))
    assert exp.base_status[0] == 0 and int(exp.base_new_offsets[-1]) == 6


@pytest.mark.parametrize("depth", [1, 2, 63, 64, 65, 5000])
def test_nesting_chains(weaver, depth):
    for opener in (OPEN_LIST, OPEN_MAP):
        toks = [(ROOT_MAP, 0, 0, 1)] + [(opener, 0, 5 + k, 0) for k in range(depth)] + [leaf(8, 0)] + [END] * (depth + 1)
        exp = check(weaver, batch([toks, toks[:1] + [END]]))
        assert int(exp.base_new_offsets[-1]) == depth + 2 and (exp.base_status == 0).all()


def test_twenty_thousand_leaves_chain_across_tiles(weaver):
    toks = [(PART, 0, NIL, 1)] + [leaf() for _ in range(20000)] + [END]
    exp = check(weaver, batch([toks], [[0]]))
    np.testing.assert_array_equal(exp.node_cause[1:], exp.node_id[:-1])
    assert exp.node_cause[0] == NIL and exp.node_run.sum() == 1


def test_a_long_string_in_a_list_and_in_a_map(weaver):
    n = 100000
    in_list = [(ROOT_LIST, 0, 0, 1), (STR, 0, 0, 1), leaf(), (STR, n, 0, 1), (STR, 0, 0, 1), leaf(), (STR, 0, 0, 1), END]
    in_map = [(PART, 0, 0, 1), (STR, n, 7, 0), END]
    exp = check(weaver, batch([in_list, in_map], [[], [1]]))
    assert list(exp.base_node_offsets) == [0, n + 3, n + 4]
    np.testing.assert_array_equal(exp.node_sub[3:n + 3], np.arange(n, dtype=U32))   # after the map's node, the root, a leaf


def test_empty_values_and_empty_parts(weaver):
    """[[], {}, nil, ""] as a root, and parts with nothing in them."""
    value = [(ROOT_LIST, 0, 0, 1), (OPEN_LIST, 0, 0, 1), END, (OPEN_MAP, 0, 0, 1), END, (OPEN_LIST, 0, 0, 1), END,
             (STR, 0, 0, 1), END]
    empties = [(PART, 0, 0, 1), END, (PART, 1, 0, 1), END, (ROOT_MAP, 0, 0, 1), END]
    exp = check(weaver, batch([value, empties, []], [[], [0, 1], [1]]))
    assert list(exp.base_new_offsets) == [0, 4, 5, 5] and list(exp.base_node_offsets) == [0, 6, 6, 6]


def test_a_thousand_parts_into_one_document(weaver):
    """Interleaved with parts into two others: the runs in part order, node_run."""
    toks = []
    for k in range(1000):
        toks += [(PART, 1, 100 + k, 1), leaf(), (STR, k % 3, 0, 1), END]
        toks += [(PART, (0, 2)[k % 2], 0, 1), leaf(k, 0), (OPEN_LIST, 0, k, 0), leaf(), END, END]
    exp = check(weaver, batch([toks], [[1, 0, 1]]))
    lo, hi = int(exp.node_offsets[1]), int(exp.node_offsets[2])
    assert exp.node_run[lo:hi].sum() == 1000
    np.testing.assert_array_equal(exp.node_cause[lo:hi][exp.node_run[lo:hi] == 1], np.arange(100, 1100, dtype=U64))
    assert (np.diff(exp.node_id[lo:hi].astype(np.int64)) > 0).all()


def test_both_routes_give_the_same_arrays(weaver):
    """The random batch again with transact_cap at its minimum: every base of two
    tokens or more sends the call through the key sort over all bases."""
    rng = random.Random(20261021)
    b = M.random_batch(rng, 2000, budget=60, depth=6, p_bad=0.1)
    exp = M.transact_columns(**b)
    with abi.Weaver(0, {"transact_cap": 1}) as w:
        w.set_profiling(True)
        try:
            assert M.same(A.transact(w, **b), exp) == []
            assert M.same(device_call(w, b, exp), exp) == []
            names = set(w.kernel_stats())
        finally:
            w.set_profiling(False)
        assert "k_tx_sort_wg" not in names and any(n.startswith("tx_sort") for n in names) and "k_tx_expand" in names
        w.set_option("transact_cap", 4096)       # and back, on the same context
        w.reset_kernel_stats()
        w.set_profiling(True)
        try:
            assert M.same(device_call(w, b, exp), exp) == []
            names = set(w.kernel_stats())
        finally:
            w.set_profiling(False)
        assert "k_tx_sort_wg" in names and not any(n.startswith("tx_sort") for n in names)


@pytest.mark.parametrize("n", [CAP, CAP + 1])
def test_bases_of_cap_and_cap_plus_one_tokens(weaver, n):
    """CAP tokens: the workgroup's LDS sort, full; CAP + 1: the key sort, for the small neighbours too."""
    rng = random.Random(n)
    toks = [(ROOT_LIST, 0, 0, 1)]
    while len(toks) < n - 40:                     # groups of mixed depth, then leaves up to n
        d = rng.randrange(1, 6)
        toks += [(rng.choice((OPEN_LIST, OPEN_MAP)), 0, rng.randrange(9), 0) for _ in range(d)] + \
            [leaf(rng.randrange(9), 0), (STR, rng.randrange(4), 3, 0)] + [END] * d
    toks += [leaf()] * (n - 1 - len(toks)) + [END]
    assert len(toks) == n
    weaver.reset_kernel_stats()
    weaver.set_profiling(True)
    try:
        exp = check(weaver, batch([[(ROOT_LIST, 0, 0, 1), leaf(), leaf(), END], toks, [(ROOT_MAP, 0, 0, 1), leaf(2, 0), END]]))
        names = set(weaver.kernel_stats())
    finally:
        weaver.set_profiling(False)
    assert (exp.base_status == 0).all() and ("k_tx_sort_wg" in names) == (n == CAP)


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_bases_around_a_tile_of_tokens(weaver, n):
    toks = [(ROOT_MAP, 0, 0, 1)] + [leaf(k, 0) for k in range(n - 2)] + [END]
    check(weaver, batch([toks, toks, toks[:5] + [END]]))


BAD = {
    "a CLOSE with no open group": [(ROOT_LIST, 0, 0, 1), leaf(), END, END],
    "a group still open at the end": [(ROOT_LIST, 0, 0, 1), (OPEN_MAP, 0, 0, 1), leaf(), END],
    "a PART inside a group": [(ROOT_LIST, 0, 0, 1), (PART, 0, 0, 1), END, END],
    "a ROOT inside a group": [(PART, 0, 0, 1), (ROOT_MAP, 0, 0, 1), END, END],
    "a LEAF outside any group": [leaf(), (ROOT_LIST, 0, 0, 1), END],
    "a STR outside any group": [(ROOT_LIST, 0, 0, 1), END, (STR, 1 << 31, 0, 1)],
    "an OPEN outside any group": [(OPEN_LIST, 0, 0, 1), END],
    "a target outside the base": [(PART, 0, 0, 1), leaf(), END],
    "a target outside the batch": [(PART, 7, 0, 1), leaf(), END],
    "a target of the next base": [(PART, 2, 0, 1), leaf(), END],
    "a kind out of range": [(ROOT_LIST, 0, 0, 1), (8, 0, 0, 1), END],
    "another kind out of range": [(ROOT_LIST, 0, 0, 1), END, (255, 0, 0, 1)],
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_a_malformed_base_between_two_good_ones(weaver, what):
    good = [(PART, 0, 0, 1), leaf(), (OPEN_MAP, 0, 0, 1), (STR, 2, 5, 0), END, END, (ROOT_MAP, 0, 0, 1), leaf(3, 0), END]
    good2 = [(PART, 2, 0, 1), leaf(), END]
    exp = check(weaver, batch([good, BAD[what], good2], [[0], [0], [0]]))
    assert list(exp.base_status) == [0, A.STATUS_TX_MALFORMED, 0]
    alone = M.transact_columns(**batch([good, [], good2], [[0], [0], [0]]))
    for f in ("node_id", "node_cause", "node_ref", "node_offsets", "new_is_map", "root_doc"):
        np.testing.assert_array_equal(getattr(exp, f), getattr(alone, f))


def test_the_tx_field_holds_eight_nodes_not_nine(weaver):
    lay = pack.KeyLayout(20, 4, 3)
    for n, st in ((8, 0), (9, abi.STATUS_KEY_RANGE)):
        toks = [(PART, 0, 0, 1)] + [leaf()] * (n - 4) + [(STR, 3, 0, 1), (OPEN_LIST, 0, 0, 1), END, END]
        exp = check(weaver, batch([toks, [(PART, 1, 0, 1), leaf(), leaf(), END]], [[0], [0]], layout=lay))
        assert list(exp.base_status) == [st, 0] and int(exp.base_node_offsets[1]) == (0 if st else n + 1)


def test_empty_batches_and_calls_that_grow_and_shrink(weaver):
    check(weaver, batch([]))
    check(weaver, batch([[], []], [[0], []]))
    rng = random.Random(5)
    for n in (3, 700, 40, 1500, 1):
        check(weaver, M.random_batch(rng, n, p_bad=0.05))


def test_every_call_error_leaves_the_outputs_untouched(weaver):
    import ctypes as C

    b = batch([[(ROOT_LIST, 0, 0, 1), leaf(), (OPEN_MAP, 0, 0, 1), END, END]])
    exp = M.transact_columns(**b)
    assert M.same(A.transact(weaver, **b), exp) == []

    def call(edit_b=None, edit_r=None, memspace=abi.CW_MEM_HOST, new_cap=2, node_cap=3, null=None):
        cols = A._token_columns(*(b[f] for f in ("tok_kind", "tok_arg", "tok_cause", "tok_cause_is_id", "tok_vkind")))
        doff, toff, ism = np.array([0, 0, 0], U64), np.array([0, 5, 5], U64), np.zeros(1, U8)
        ntx = np.array([b["new_tx"][0], 0], U64)
        cb = A.CwTransactBatch(0, abi._u64p(doff), abi._ptr(ism), LAY.ts_shift, LAY.site_shift, LAY.site_bits, 0, 1,
                               abi._ptr(ntx), abi._u64p(toff), *map(abi._ptr, cols))
        outs = [np.full(8, 0x55, dt) for dt in (U64, U64, U64)] + [np.full(8, 0x55, dt) for _, dt in A.NODE_COLUMNS] + \
            [np.full(8, 0x55, dt) for _, dt in A.NEW_COLUMNS] + [np.full(8, 0x55, U32), np.full(8, 0x55, U32)]
        cr = A.CwTransactResult(new_cap, node_cap, *map(abi._u64p, outs[:3]), *map(abi._ptr, outs[3:]))
        keep = (doff, toff, ism, cols)
        if edit_b:
            edit_b(cb, keep)
        if edit_r:
            edit_r(cr)
        rc = A.lib().cw_transact(weaver._h, None if null == "batch" else C.byref(cb),
                                 None if null == "result" else C.byref(cr), memspace)
        return rc, outs

    def refused(**kw):
        rc, outs = call(**kw)
        assert rc < 0 and A.lib().cw_last_error(weaver._h)
        for o in outs:
            assert (o == 0x55).all()

    rc, outs = call()
    assert rc == 0 and outs[3][0] == 0 and outs[3][1] == exp.node_id[1]
    null = lambda f: (lambda s, *_: setattr(s, f, None))
    for f in ("base_doc_offsets", "tok_offsets", "tok_kind", "tok_arg", "tok_cause", "tok_cause_is_id", "new_tx"):
        refused(edit_b=null(f))
    for f in ("base_new_offsets", "base_node_offsets", "node_offsets", "root_doc", "base_status", "node_run", "new_open"):
        refused(edit_r=null(f))
    refused(edit_b=lambda s, k: k[1].__setitem__(0, 1))                 # offsets that do not start at 0
    refused(edit_b=lambda s, k: k[1].__setitem__(2, 3) or setattr(s, "n_bases", 2))   # ... that decrease (5, 3)
    refused(edit_b=lambda s, k: setattr(s, "n_docs", 1))                 # base_doc_offsets[n_bases] != n_docs
    refused(edit_b=lambda s, k: setattr(s, "site_bits", 11))
    refused(edit_b=lambda s, k: setattr(s, "site_bits", 0))
    refused(edit_b=lambda s, k: setattr(s, "site_shift", 64))
    refused(edit_b=lambda s, k: setattr(s, "reserved", 1))
    refused(edit_b=lambda s, k: setattr(s, "ts_shift", 64))
    refused(null="batch")
    refused(null="result")

    def one_doc_no_map(s, k):                                            # n_docs > 0 and no doc_is_map
        k[0][1] = k[0][2] = 1
        s.n_docs, s.doc_is_map = 1, None
    refused(edit_b=one_doc_no_map)
    # the limits, through the host offsets alone: no token array is read before they are checked
    refused(edit_b=lambda s, k: k[1].__setitem__(1, (1 << 32) - 1))     # T >= 2^32 - 1
    refused(edit_b=lambda s, k: k[1].__setitem__(1, (1 << 32) - 2))     # the sort key: 32 + 33 bits > 63

    def docs_and_tokens(s, k):                                           # n_docs + T >= 2^32 - 1
        k[0][1] = k[0][2] = 1 << 31
        k[1][1] = k[1][2] = 1 << 31
        s.n_docs = 1 << 31
    refused(edit_b=docs_and_tokens)
    refused(memspace=7)
    refused(new_cap=1)
    refused(node_cap=2)


# ----------------------------------------------------- into the weaves ----
def test_new_collections_go_straight_into_the_weaves(weaver):
    """Root transactions in device memory: the new lists, roots included, are
    cw_weave_lists' documents and the new maps cw_weave_maps' collections, with
    nothing but the host offsets in between; compared with the host-memory route."""
    import torch

    rng = random.Random(77)
    streams = []
    for g in range(40):          # bases 0..19 make lists of lists, 20..39 maps of maps
        m = g >= 20
        s = [(ROOT_MAP if m else ROOT_LIST, 0, 0, 1)]
        for _ in range(rng.randrange(1, 12)):
            key = (rng.randrange(1, 6), 0) if m else (0, 1)
            if rng.random() < 0.3:
                s += [(OPEN_MAP if m else OPEN_LIST, 0) + key] + \
                    [leaf(rng.randrange(1, 6), 0) if m else leaf() for _ in range(rng.randrange(0, 9))] + [END]
            else:
                s.append(leaf(*key) if m or rng.random() < 0.7 else (STR, rng.randrange(4), 0, 1))
        streams.append(s + [END])
    lay = pack.KeyLayout(10, 4, 10)
    b = batch(streams, layout=lay, new_tx=[lay.pack(3 + g, g % 16, 0) for g in range(40)])
    exp = M.transact_columns(**b)
    C, Mn = int(exp.base_new_offsets[-1]), int(exp.base_node_offsets[-1])
    CL = int(exp.base_new_offsets[20])                    # the lists come first
    assert not exp.new_is_map[:CL].any() and exp.new_is_map[CL:].all() and 20 < CL < C - 20
    dev = torch.device("cuda", 0)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=getattr(torch, TORCH[np.dtype(dt)]), device=dev)
    o = {f: z(Mn, dt) for f, dt in A.NODE_COLUMNS}
    o.update({f: z(C, dt) for f, dt in A.NEW_COLUMNS})
    o.update(root_doc=z(40, U32), base_status=z(40, U32))
    ins = [up(b[f]) for f in ("tok_kind", "tok_arg", "tok_cause", "tok_cause_is_id", "tok_vkind")]
    g_tx = up(b["new_tx"])
    torch.cuda.synchronize()
    bn, bm, no = A.transact_device(weaver, b["base_doc_offsets"], None, lay, g_tx.data_ptr(), b["tok_offsets"],
                                   [x.data_ptr() for x in ins], C, Mn, {k: v.data_ptr() for k, v in o.items()})
    np.testing.assert_array_equal(no, exp.node_offsets)
    # the lists: documents [0, CL) of the node columns as they lie
    NL = int(no[CL])
    lo_ = {"weave_perm": z(NL, U32), "visible_bits": z((NL + 31) // 32, U32), "visible_count": z(CL, U32),
           "max_ts": z(CL, U64), "status": z(CL, U32)}
    weaver.weave_lists_device(no[:CL + 1], o["node_id"].data_ptr(), o["node_cause"].data_ptr(),
                              o["node_kind"].data_ptr(), lay, {k: v.data_ptr() for k, v in lo_.items()})
    torch.cuda.synchronize()
    want = weaver.weave_lists(exp.node_offsets[:CL + 1], exp.node_id[:NL], exp.node_cause[:NL], exp.node_kind[:NL], lay,
                              yarns=False)
    assert not want.status.any() and int(want.visible_count.sum()) > 100
    np.testing.assert_array_equal(lo_["weave_perm"].cpu().numpy().view(U32)[:NL], want.weave_perm)
    np.testing.assert_array_equal(lo_["visible_count"].cpu().numpy().view(U32)[:CL], want.visible_count)
    np.testing.assert_array_equal(lo_["status"].cpu().numpy().view(U32)[:CL], want.status)
    # the maps: collections [CL, C), the columns from node NL on, the offsets rebased on the host
    moff, NM, CM = no[CL:C + 1] - no[CL], Mn - NL, C - CL
    mo = {"seg_offsets": z(NM + 1, U64), "seg_coll": z(NM, U32), "seg_key": z(NM, U64), "seg_active": z(NM, U64),
          "seg_perm": z(2 * NM, U32), "status": z(CM, U32)}
    at = lambda f, w: o[f].data_ptr() + NL * w
    S = weaver.weave_maps_device(moff, (at("node_id", 8), at("node_cause", 8), at("node_cause_is_id", 1),
                                        at("node_kind", 1)), 8, lay.key_bits, {k: v.data_ptr() for k, v in mo.items()}, NM)
    torch.cuda.synchronize()
    want = weaver.weave_maps(moff, exp.node_id[NL:], exp.node_cause[NL:], exp.node_cause_is_id[NL:], exp.node_kind[NL:],
                             8, lay.key_bits)
    assert S == len(want.seg_coll) > 50 and not want.status.any()
    for f, dt in (("seg_offsets", U64), ("seg_coll", U32), ("seg_key", U64), ("seg_perm", U32), ("status", U32)):
        n = len(getattr(want, f))
        np.testing.assert_array_equal(mo[f].cpu().numpy().view(dt)[:n], getattr(want, f))


# ------------------------------------------------------------- the host layer ----
def test_transact_bases_on_the_gpu_equals_transact(weaver):
    from tests import test_transact_model as TM

    cbs, txs = TM.seeded_cases(20261021, 60)
    got = B.transact_bases(cbs, txs)
    want = [B.transact_(cb, tx) for cb, tx in zip(TM.seeded_cases(20261021, 60)[0], txs)]
    assert [TM.strip(x) for x in got] == [TM.strip(x) for x in want]
    assert B.bases_to_edn(got) == [B.cb_to_edn(x)[0] for x in want]
