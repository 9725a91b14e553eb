"""cw_insert_lists on the GPU against tests/insert_model.py: every output array
compared in full.

One batch (about 2 * 10^5 nodes; S = 8,192, the kernels' tile) holds the
document sizes, tx sizes, insert positions, refusals and rendering cases of
the scenario table below; the old weaves come from cw_weave_lists.  Then
out-of-domain documents (the model is the literal weave-node), a chain of 20
calls held against the full reweave, both memspaces, NULL outputs, every error
return, and cw_render_lists on the result.

On "a normal node between a target and its hide": weave-node cannot put one
there.  With nr the hide of X, later(nr) is false for a plain nm only when
cause(nr) = id(nm), and then nr hides nm, not X.  The batch holds the cases
that exist: a hide right after its target, an h.show (alone and heading a tx)
between a target and its hide, and a plain node before an orphan hide that
names it.
"""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest

from cause_amd import abi, abi_insert
from tests import insert_model as M

pytestmark = pytest.mark.gpu

S = 8192
TXB, SB = 14, 3
LAY = NS(key_bits=40, ts_shift=TXB + SB, site_shift=TXB, site_bits=SB)
NIL = (1 << 64) - 1
NONE = 0xFFFFFFFF
U8, U32, U64 = np.uint8, np.uint32, np.uint64
NORMAL, HIDE, HHIDE, HSHOW, ROOT = 0, 1, 2, 3, 4


def key(ts, site, tx=0):
    return (int(ts) << LAY.ts_shift) | (int(site) << LAY.site_shift) | int(tx)


def gen_doc(rng, n, wild=False):
    """A document of n nodes, root first: node i has ts i and a site of 1..5, is
    caused by an earlier node (half of them by the one before) and is special
    one time in eight.  wild: some causes are no node (orphans), some name a
    later node (non-Lamport)."""
    idk = np.array([0] + [key(i, s) for i, s in zip(range(1, n), rng.integers(1, 6, n - 1))], U64)
    ci = np.where(rng.random(n) < 0.5, np.arange(n) - 1, (rng.random(n) * np.arange(n)).astype(np.int64))
    if wild:
        ci = np.where(rng.random(n) < 0.15, rng.integers(0, n, n), ci)
        ci = np.where(ci == np.arange(n), np.arange(n) - 1, ci)  # (no node causes itself)
    ck = idk[np.clip(ci, 0, None)]
    if wild:
        ck = np.where(rng.random(n) < 0.1, U64(key(5000, 7)), ck)
    ck[0] = NIL
    kd = np.where(rng.random(n) < 0.125, rng.integers(1, 4, n), 0).astype(U8)
    kd[0] = ROOT
    return [idk, ck.astype(U64), kd]


def comb_doc(L):
    """root; under it a newer child (ts 5) heading a chain of L nodes and an
    older one (ts 2): the weave is root, the chain, the older child, so a tx
    under the root with ts 3 scans the whole chain before it stops."""
    idk = [0, key(2, 1), key(5, 1)] + [key(6 + i, 1) for i in range(L)]
    ck = [NIL, 0, 0] + idk[2:-1]
    return [np.array(idk, U64), np.array(ck, U64), np.array([ROOT] + [0] * (L + 2), U8)]


def hand_doc(nodes):
    """[(id, cause, kind)] -> columns."""
    return [np.array([n[0] for n in nodes], U64), np.array([n[1] for n in nodes], U64),
            np.array([n[2] for n in nodes], U8)]


def run_tx(ts, cause, k, site=6, kinds=None):
    """A tx of k nodes (ts, site, 0..k-1): the first under `cause`, the others chained."""
    ids = [key(ts, site, m) for m in range(k)]
    return [(ids[m], cause if m == 0 else ids[m - 1], kinds[m] if kinds else NORMAL) for m in range(k)]


class Batch:
    """Documents with a woven state and one tx each, as arrays."""

    def __init__(self, weaver, docs, rng):
        self.docs = docs
        self.off = np.zeros(len(docs) + 1, U64)
        self.off[1:] = np.cumsum([len(d[0]) for d in docs])
        self.idk, self.ck, self.kd = (np.concatenate([d[c] for d in docs]) for c in range(3))
        self.val = rng.integers(0, 1 << 40, len(self.idk)).astype(U64)
        w = weaver.weave_lists(self.off, self.idk, self.ck, self.kd, LAY)
        assert not (w.status & (abi.STATUS_DUP | abi.STATUS_INTERNAL)).any()
        self.w, self.txs = w, [[] for _ in docs]
        self.tval = {}

    def weave_ids(self, d):
        lo, hi = int(self.off[d]), int(self.off[d + 1])
        return self.idk[lo:hi][self.w.weave_perm[lo:hi]]

    def arrays(self):
        toff = np.zeros(len(self.docs) + 1, U64)
        toff[1:] = np.cumsum([len(t) for t in self.txs])
        flat = [n for t in self.txs for n in t]
        tid, tca = (np.array([n[c] for n in flat], U64) for c in range(2))
        tkd = np.array([n[2] for n in flat], U8)
        tval = (np.arange(len(flat), dtype=U64) + U64(1 << 41))
        for d, v in self.tval.items():
            tval[int(toff[d])] = v
        return toff, tid, tca, tkd, tval


def model_of(b, tx, yarns=True, values=True):
    toff, tid, tca, tkd, tval = tx
    return M.insert_lists(b.off, b.idk, b.ck, b.kd, b.w.weave_perm, b.w.visible_bits, toff, tid, tca, tkd,
                          LAY.ts_shift, LAY.site_shift, LAY.site_bits, b.w.yarn_perm if yarns else None,
                          b.val if values else None, tval if values else None)


def host_call(weaver, b, tx, yarns=True, values=True, columns=True):
    toff, tid, tca, tkd, tval = tx
    return abi_insert.insert_lists(weaver, (b.off, b.idk, b.ck, b.kd), b.w.weave_perm, b.w.visible_bits,
                                   (toff, tid, tca, tkd, tval if values else None), LAY,
                                   yarn_perm=b.w.yarn_perm if yarns else None,
                                   doc_value=b.val if values else None, columns=columns)


def up(x):
    import torch

    signed = {np.dtype(U64): np.int64, np.dtype(U32): np.int32}.get(x.dtype)
    x = np.ascontiguousarray(x)
    if not len(x):
        x = np.zeros(1, x.dtype)
    return torch.from_numpy(x.view(signed) if signed else x).to(torch.device("cuda", 0))


def device_call(weaver, b, tx, null=()):
    """The device-memory call on torch tensors; returns an InsertResult of host
    copies (None for the outputs named in `null`)."""
    import torch

    toff, tid, tca, tkd, tval = tx
    N, T, D = len(b.idk), len(tid), len(b.docs)
    cap = max(N + T, 1)
    g = [up(x) for x in (b.idk, b.ck, b.kd, b.w.weave_perm, b.w.visible_bits, b.w.yarn_perm, b.val,
                         tid, tca, tkd, tval)]
    z = lambda n, dt: torch.full((max(n, 1),), 0x55, dtype=dt, device=g[0].device)
    o = {"weave_perm": z(cap, torch.int32), "visible_bits": z((cap + 31) // 32, torch.int32),
         "visible_count": z(D, torch.int32), "max_ts": z(D, torch.int64), "status": z(D, torch.int32),
         "yarn_perm": z(cap, torch.int32)}
    pos = z(D, torch.int32)
    cols = [z(cap, torch.int64), z(cap, torch.int64), z(cap, torch.uint8), z(cap, torch.int64)]
    ptr = lambda t, name: None if name in null else t.data_ptr()
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    offs = abi_insert.insert_lists_device(
        weaver, b.off, [t.data_ptr() for t in g[:3]], g[3].data_ptr(), g[4].data_ptr(), toff,
        [t.data_ptr() for t in g[7:10]] + [ptr(g[10], "value")], LAY,
        {k: ptr(v, k) for k, v in o.items()}, pos_ptr=ptr(pos, "insert_pos"),
        yarn_ptr=ptr(g[5], "yarn_perm"), value_ptr=ptr(g[6], "value"),
        col_ptrs=None if "columns" in null else [t.data_ptr() for t in cols[:3]] + [ptr(cols[3], "value")])
    torch.cuda.synchronize()
    m = int(offs[-1])
    host = lambda t, dt, n, name: None if name in null else t.cpu().numpy().view(dt)[:n]
    lr = abi.ListResult(host(o["weave_perm"], U32, m, ""), host(o["visible_bits"], U32, (m + 31) // 32, ""),
                        host(o["visible_count"], U32, D, ""), host(o["max_ts"], U64, D, "max_ts"),
                        host(o["status"], U32, D, ""), host(o["yarn_perm"], U32, m, "yarn_perm"))
    c = "columns"
    return abi_insert.InsertResult(offs, host(pos, U32, D, "insert_pos"), lr, host(cols[0], U64, m, c),
                                   host(cols[1], U64, m, c), host(cols[2], U8, m, c),
                                   host(cols[3], U64, m, "value" if "value" in null else c))


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(at)} of {len(want)} differ, first at {at[0]}: "
                             f"{got[at[0]]} != {want[at[0]]}")


def compare(res, exp, null=()):
    """Every array of an InsertResult against the model's."""
    same(res.offsets, exp.new_offsets, "new_offsets")
    same(res.weave.status, exp.status, "status")
    if "insert_pos" not in null:
        same(res.insert_pos, exp.insert_pos, "insert_pos")
    same(res.weave.weave_perm, exp.weave_perm, "weave_perm")
    same(res.weave.visible_bits, exp.visible_bits, "visible_bits")
    same(res.weave.visible_count, exp.visible_count, "visible_count")
    if "max_ts" not in null:
        same(res.weave.max_ts, exp.max_ts, "max_ts")
    if "yarn_perm" not in null and exp.yarn_perm is not None:
        same(res.weave.yarn_perm, exp.yarn_perm, "yarn_perm")
    if "columns" not in null:
        same(res.id_key, exp.id_key, "id_key")
        same(res.cause_key, exp.cause_key, "cause_key")
        same(res.kind, exp.kind, "kind")
        if "value" not in null and exp.value is not None:
            same(res.value, exp.value, "value")


@pytest.fixture(scope="module")
def weaver():
    with abi.Weaver(0) as w:
        yield w


# ------------------------------------------------------------------- the batch
X, H = key(1, 1), key(2, 2)
RENDER_DOCS = {
    # a hide (newest) lands right after its target X: X stops rendering
    "hide_after_target": ([(0, NIL, ROOT), (X, 0, 0), (key(2, 1), X, 0)], [(key(9, 6), X, HIDE)]),
    # an h.show (newer than the hide H of X) lands between X and H: X renders again
    "hshow_between": ([(0, NIL, ROOT), (X, 0, 0), (H, X, HIDE), (key(3, 1), X, 0)], [(key(9, 6), X, HSHOW)]),
    # a tx headed by an h.show lands there: its last (plain) node is followed by
    # the hide of weave[p]'s predecessor X and keeps rendering
    "tx_before_the_hide": ([(0, NIL, ROOT), (X, 0, 0), (H, X, HHIDE)],
                           run_tx(9, X, 3, kinds=[HSHOW, NORMAL, NORMAL])),
    # an orphan hide that names the tx node (out of domain): the plain node lands
    # before it and does not render
    "hidden_by_an_orphan": ([(0, NIL, ROOT), (X, 0, 0), (key(3, 2), key(9, 6), HIDE)], [(key(9, 6), X, 0)]),
    # a hide of the last node, and a tx whose last node is a hide of the one before
    "hide_at_the_end": ([(0, NIL, ROOT), (X, 0, 0)], [(key(9, 6), X, HHIDE)]),
    "tx_hides_itself": ([(0, NIL, ROOT), (X, 0, 0)], run_tx(9, 0, 2, kinds=[NORMAL, HIDE])),
}
SIZES = [1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S + 5, 2 * S + 5, S + 1]
N_SMALL = 3000


@pytest.fixture(scope="module")
def big(weaver):
    rng = np.random.default_rng(11)
    docs = [comb_doc(S), comb_doc(2 * S)]            # documents 0, 1: at global offsets 0 and S + 3
    docs += [gen_doc(rng, n) for n in SIZES]          # 2 .. 12
    names = list(RENDER_DOCS)
    docs += [hand_doc(RENDER_DOCS[k][0]) for k in names]
    first_small = len(docs)
    docs += [gen_doc(rng, int(n)) for n in rng.integers(1, 41, N_SMALL)]
    docs += [gen_doc(rng, 2 * S + 5), gen_doc(rng, 5000)]  # after the small ones: not tile-aligned
    b = Batch(weaver, docs, rng)
    n_of = lambda d: len(docs[d][0])
    top = lambda d: n_of(d) + 5                       # a ts above every node of d
    b.note = {}
    # the scan crosses one tile and two tiles after a
    for d in (0, 1):
        b.txs[d] = run_tx(3, 0, 1 + d)
        b.note[d] = "comb"
    # sizes 1 .. 2S+5: conj and cons
    for d in range(2, 2 + len(SIZES)):
        last = int(b.weave_ids(d)[-1])
        b.txs[d] = run_tx(top(d), last if d % 2 == 0 else 0, [1, 2, 64][d % 3])
    d_old, d_edge, d_big = 2 + SIZES.index(2 * S + 5), 2 + SIZES.index(2 * S + 5) + 1, 2 + len(SIZES) - 1
    # an old-timestamp node under the root of a document whose nodes are all younger: p = n
    b.txs[d_old] = [(key(0, 6), 0, NORMAL)]
    # a cause at the last position of a tile: a falls on the tile boundary
    lo = int(b.off[d_edge])
    at = (-(lo + 1)) % S + S
    assert (lo + at) % S == S - 1 and at < n_of(d_edge)
    b.txs[d_edge] = run_tx(top(d_edge), int(b.weave_ids(d_edge)[at]), 2)
    b.note["edge"] = (d_edge, at)
    b.txs[d_big] = run_tx(top(d_big), int(b.weave_ids(d_big)[S // 2]), S + 100)
    for i, k in enumerate(names):
        b.txs[first_small - len(names) + i] = list(RENDER_DOCS[k][1])
    b.note["render"] = {k: first_small - len(names) + i for i, k in enumerate(names)}
    # the small documents: every tx size, Lamport and non-Lamport ids, every kind; refusals among them
    b.note["refused"] = {}
    for d in range(first_small, first_small + N_SMALL):
        n, lo = n_of(d), int(b.off[d])
        cause = int(docs[d][0][rng.integers(0, n)])
        ts = top(d) if rng.random() < 0.7 else int(rng.integers(0, n + 5))
        k = int(rng.choice([0, 1, 1, 2, 2, 64]))
        kinds = [int(x) for x in np.where(rng.random(max(k, 1)) < 0.2, rng.integers(1, 4, max(k, 1)), 0)]
        b.txs[d] = run_tx(ts, cause, k, kinds=kinds) if k else []
        r = d % 10
        if r in (3, 4, 5, 6) and n > 1:
            j = int(rng.integers(1, n))
            i0, c0, k0 = (int(docs[d][c][j]) for c in range(3))
            b.tval[d] = b.val[lo + j]
            if r == 3:    # the same body: skipped, the node behind it too
                b.txs[d] = [(i0, c0, k0), (i0 + 1, i0, NORMAL)]
            elif r == 4:  # another cause
                b.txs[d] = [(i0, int(docs[d][0][0]) if c0 != 0 else i0, k0)]
            elif r == 5:  # another kind
                b.txs[d] = [(i0, c0, (k0 + 1) % 4)]
            else:         # another value token
                b.txs[d] = [(i0, c0, k0)]
                b.tval[d] = b.val[lo + j] + U64(1)
            b.note["refused"][d] = 0 if r == 3 else abi.STATUS_DUP
        elif r == 7:      # a cause that is no node
            b.txs[d] = run_tx(top(d), key(9000, 7), 2)
            b.note["refused"][d] = abi.STATUS_ORPHAN
        elif r == 8:      # a nil cause
            b.txs[d] = run_tx(top(d), NIL, 1)
            b.note["refused"][d] = abi.STATUS_ORPHAN
    b.txs[-2] = run_tx(top(len(docs) - 2), int(b.weave_ids(len(docs) - 2)[S + 7]), 64)
    b.txs[-1] = run_tx(2500, int(docs[-1][0][17]), 2)
    b.tx = b.arrays()
    b.exp = model_of(b, b.tx)
    return b


def test_the_batch_holds_the_cases_it_names(big):
    exp, off = big.exp, big.off.astype(np.int64)
    assert 150_000 < int(off[-1]) + len(big.tx[1]) < 250_000
    pos = exp.insert_pos.astype(np.int64)
    # the comb documents: a = 1 and the stop one tile and two tiles later
    for d, tiles in ((0, 1), (1, 2)):
        assert (off[d] + pos[d]) // S - (off[d] + 1) // S == tiles and pos[d] == off[d + 1] - off[d] - 1
    d_old = 2 + SIZES.index(2 * S + 5)
    assert pos[d_old] == 2 * S + 5                       # crossed every tile: p = n
    d_edge, at = big.note["edge"]
    assert (off[d_edge] + at) % S == S - 1 and pos[d_edge] >= at + 1
    for d in range(2, 2 + len(SIZES)):
        n = int(off[d + 1] - off[d])
        if d not in (d_old, d_edge, 2 + len(SIZES) - 1):
            lo = int(off[d])
            wk = big.kd[lo:lo + n][big.w.weave_perm[lo:lo + n]] & 3
            if d % 2 == 0:   # conj
                assert pos[d] == n
            else:            # cons: right behind the root's special children
                assert pos[d] >= 1 and (wk[1:pos[d]] != 0).all() and (pos[d] == n or wk[pos[d]] == 0)
    assert int(np.diff(big.tx[0].astype(np.int64)).max()) == S + 100
    assert set(np.diff(big.tx[0].astype(np.int64)).tolist()) >= {0, 1, 2, 64, S + 100}
    # the refusals: status, nothing inserted, and the layout compacts over them
    ref = big.note["refused"]
    assert len(ref) > 1000 and {0, abi.STATUS_DUP, abi.STATUS_ORPHAN} == set(ref.values())
    for d, st in ref.items():
        assert int(exp.status[d]) == st and pos[d] == NONE
        assert exp.new_offsets[d + 1] - exp.new_offsets[d] == off[d + 1] - off[d]
    assert int(exp.new_offsets[-1]) < int(off[-1]) + len(big.tx[1])
    grew = np.diff(exp.new_offsets.astype(np.int64)) - np.diff(off)
    assert ((grew == 0) | (grew == np.diff(big.tx[0].astype(np.int64)))).all()
    assert (grew[[d for d in range(len(pos)) if d not in ref and pos[d] != NONE]] > 0).all()
    # rendering
    vis = lambda d: exp.visible[int(exp.new_offsets[d]):int(exp.new_offsets[d + 1])].tolist()
    r = big.note["render"]
    assert vis(r["hide_after_target"]) == [0, 0, 0, 1]
    assert vis(r["hshow_between"]) == [0, 1, 0, 0, 1]
    assert vis(r["tx_before_the_hide"]) == [0, 1, 0, 1, 1, 0]
    assert vis(r["hidden_by_an_orphan"]) == [0, 1, 0, 0]
    assert vis(r["hide_at_the_end"]) == [0, 0, 0]
    assert vis(r["tx_hides_itself"]) == [0, 0, 0, 1]


def test_host_call_equals_the_model(weaver, big):
    compare(host_call(weaver, big, big.tx), big.exp)


def test_device_call_equals_the_model_and_the_host_call(weaver, big):
    dev = device_call(weaver, big, big.tx)
    compare(dev, big.exp)
    host = host_call(weaver, big, big.tx)
    for f in ("weave_perm", "visible_bits", "visible_count", "max_ts", "status", "yarn_perm"):
        same(getattr(dev.weave, f), getattr(host.weave, f), f)
    for f in ("offsets", "insert_pos", "id_key", "cause_key", "kind", "value"):
        same(getattr(dev, f), getattr(host, f), f)


def test_async_device_call(big):
    import torch

    with abi.Weaver(0) as w:
        w.set_async(True)
        compare(device_call(w, big, big.tx), big.exp)
        compare(device_call(w, big, big.tx), big.exp)  # the cached layout, the next look-back epoch
    torch.cuda.synchronize()


@pytest.mark.parametrize("null", [("max_ts",), ("yarn_perm",), ("insert_pos",), ("columns",), ("value",),
                                  ("max_ts", "yarn_perm", "insert_pos", "columns", "value")])
def test_optional_outputs_null(weaver, big, null):
    exp = big.exp if "value" not in null else model_of(big, big.tx, values=False)
    compare(device_call(weaver, big, big.tx, null), exp, null)


def test_host_call_without_yarns_values_and_columns(weaver, big):
    exp = model_of(big, big.tx, yarns=False, values=False)
    res = host_call(weaver, big, big.tx, yarns=False, values=False, columns=False)
    assert res.weave.yarn_perm is None and res.id_key is None and res.value is None
    compare(res, exp, ("yarn_perm", "columns"))
    # without value tokens "another value token" is the same body
    d = next(d for d in big.note["refused"] if d % 10 == 6)
    assert int(big.exp.status[d]) == abi.STATUS_DUP and int(res.weave.status[d]) == 0


def test_render_of_the_result(weaver, big):
    res = host_call(weaver, big, big.tx, columns=False)
    r = weaver.render_lists(res.offsets, res.weave.weave_perm, res.weave.visible_bits)
    exp = big.exp
    same(r.src, exp.weave_perm[exp.visible.astype(bool)], "rendered_src")
    bounds = np.concatenate([[0], np.cumsum(exp.visible)])[exp.new_offsets.astype(np.int64)]
    same(r.offsets, bounds.astype(U64), "rendered_offsets")


# ------------------------------------------------------- out-of-domain documents
def test_out_of_domain_documents(weaver):
    rng = np.random.default_rng(5)
    docs = [gen_doc(rng, int(n), wild=True) for n in rng.integers(2, 60, 400)] + [gen_doc(rng, S + 50, wild=True)]
    b = Batch(weaver, docs, rng)
    bad = abi.STATUS_ORPHAN | abi.STATUS_NON_LAMPORT
    assert ((b.w.status & bad) != 0).sum() > 300 and b.w.status[-1] & bad
    for d, doc in enumerate(docs):
        n = len(doc[0])
        # under a node or under an orphan's missing cause (then the orphans' e2 positions are asap)
        cause = int(doc[0][rng.integers(0, n)])
        ts = n + 5 if rng.random() < 0.5 else int(rng.integers(0, n + 5))
        k = int(rng.choice([1, 1, 2, 5]))
        kinds = [int(x) for x in np.where(rng.random(k) < 0.3, rng.integers(1, 4, k), 0)]
        b.txs[d] = run_tx(ts, cause, k, kinds=kinds)
        if d % 7 == 0:  # the id orphans of this batch name: it is their cause from now on
            b.txs[d] = [(key(5000, 7), cause, kinds[0])]
        if d % 7 == 3:  # that id under a cause that is no node: refused, though the orphans give asap positions
            b.txs[d] = [(key(5000, 7), key(6000, 7), kinds[0])]
    tx = b.arrays()
    exp = model_of(b, tx)
    named = [d for d in range(3, len(docs), 7) if (docs[d][1] == U64(key(5000, 7))).any()]
    assert len(named) > 30 and (exp.status[3::7] == abi.STATUS_ORPHAN).all()
    assert (exp.insert_pos[3::7] == NONE).all() and (exp.insert_pos != NONE).sum() > 300
    compare(host_call(weaver, b, tx), exp)
    compare(device_call(weaver, b, tx), exp)


# ------------------------------------------------------------------- the chain
def test_a_chain_of_twenty_calls_equals_the_full_reweave(weaver):
    """64 in-domain documents, 20 calls, each fed the previous call's columns and
    weave: single nodes of any kind and typed runs of three plain nodes, Lamport
    ids.  The end state equals cw_weave_lists of the final columns bit for bit."""
    rng = np.random.default_rng(21)
    docs = [gen_doc(rng, int(n)) for n in rng.integers(1, 300, 63)] + [gen_doc(rng, S - 20)]
    b = Batch(weaver, docs, rng)
    assert not b.w.status.any()
    off, idk, ck, kd, val = b.off, b.idk, b.ck, b.kd, b.val
    perm, bits, yarn = b.w.weave_perm, b.w.visible_bits, b.w.yarn_perm
    for step in range(20):
        txs = []
        for d in range(64):
            ids = idk[int(off[d]):int(off[d + 1])]
            ts = (int(ids.max()) >> LAY.ts_shift) + 1
            k = 3 if rng.random() < 0.4 else 1
            kinds = [0, 0, 0] if k == 3 else [int(rng.choice([0, 0, 0, 1, 2, 3]))]
            txs.append(run_tx(ts, int(ids[rng.integers(0, len(ids))]), k, site=int(rng.integers(1, 7)),
                              kinds=kinds) if (step + d) % 9 else [])
        toff = np.zeros(65, U64)
        toff[1:] = np.cumsum([len(t) for t in txs])
        flat = [n for t in txs for n in t]
        tid, tca = (np.array([n[c] for n in flat], U64) for c in range(2))
        tkd, tval = np.array([n[2] for n in flat], U8), np.arange(len(flat), dtype=U64)
        args = dict(yarn_perm=yarn, doc_value=val)
        exp = M.insert_lists(off, idk, ck, kd, perm, bits, toff, tid, tca, tkd, LAY.ts_shift, LAY.site_shift,
                             LAY.site_bits, yarn, val, tval)
        res = abi_insert.insert_lists(weaver, (off, idk, ck, kd), perm, bits, (toff, tid, tca, tkd, tval), LAY,
                                      **args)
        compare(res, exp)
        assert not res.weave.status.any()
        off, idk, ck, kd, val = res.offsets, res.id_key, res.cause_key, res.kind, res.value
        perm, bits, yarn = res.weave.weave_perm, res.weave.visible_bits, res.weave.yarn_perm
    assert int(off[-1]) > int(b.off[-1]) + 64 * 20
    full = weaver.weave_lists(off, idk, ck, kd, LAY)
    assert not full.status.any()
    same(perm, full.weave_perm, "weave_perm")
    same(bits, full.visible_bits, "visible_bits")
    same(res.weave.visible_count, full.visible_count, "visible_count")
    same(res.weave.max_ts, full.max_ts, "max_ts")
    same(yarn, full.yarn_perm, "yarn_perm")


# ------------------------------------------------------------------ edge batches
def test_no_documents_and_empty_documents(weaver):
    e64, e32, e8 = np.zeros(0, U64), np.zeros(0, U32), np.zeros(0, U8)
    res = abi_insert.insert_lists(weaver, ([0], e64, e64, e8), e32, e32, ([0], e64, e64, e8), LAY)
    assert res.offsets.tolist() == [0] and len(res.weave.weave_perm) == 0
    # three empty documents: a tx into one of them has no cause to hang under
    res = abi_insert.insert_lists(weaver, ([0, 0, 0, 0], e64, e64, e8), e32, e32,
                                  ([0, 0, 1, 1], np.array([key(1, 1)], U64), np.array([0], U64),
                                   np.zeros(1, U8)), LAY)
    assert res.offsets.tolist() == [0, 0, 0, 0]
    assert res.weave.status.tolist() == [0, abi.STATUS_ORPHAN, 0]
    assert res.insert_pos.tolist() == [NONE] * 3 and res.weave.visible_count.tolist() == [0, 0, 0]


def test_documents_whose_txs_are_all_empty_are_copied(weaver):
    """D > 0, N > 0, T = 0: no tx node at all, every document copied as it is."""
    rng = np.random.default_rng(8)
    b = Batch(weaver, [gen_doc(rng, n) for n in (1, 70, S + 3)], rng)
    tx = b.arrays()
    assert tx[0].tolist() == [0, 0, 0, 0] and len(tx[1]) == 0
    exp = model_of(b, tx)
    same(exp.weave_perm, b.w.weave_perm, "weave_perm")
    assert exp.insert_pos.tolist() == [NONE] * 3 and not exp.status.any()
    compare(host_call(weaver, b, tx), exp)
    compare(device_call(weaver, b, tx), exp)


def test_many_tiny_documents_cross_the_look_back_windows(weaver):
    rng = np.random.default_rng(2)
    docs = [gen_doc(rng, int(n)) for n in rng.integers(1, 4, 5000)]
    b = Batch(weaver, docs, rng)
    for d, doc in enumerate(docs):
        b.txs[d] = run_tx(9, int(doc[0][-1]), d % 3)
    tx = b.arrays()
    compare(host_call(weaver, b, tx), model_of(b, tx))


# ---------------------------------------------------------------------- errors
def small_call():
    """A valid host call on two documents as raw structs, and what keeps them alive."""
    off, toff = np.array([0, 2, 3], U64), np.array([0, 1, 1], U64)
    idk, ck, kd = np.array([0, key(1, 1), 0], U64), np.array([NIL, 0, NIL], U64), np.array([4, 0, 4], U8)
    perm, bits, yarn = np.array([0, 1, 0], U32), np.array([2], U32), np.array([0, 1, 0], U32)
    val = np.array([1, 2, 3], U64)
    tid, tca, tkd, tval = np.array([key(2, 1)], U64), np.array([key(1, 1)], U64), np.zeros(1, U8), np.array([9], U64)
    lb = abi.CwListBatch(2, abi._u64p(off), abi._ptr(idk), abi._ptr(ck), abi._ptr(kd), LAY.key_bits,
                         LAY.ts_shift, LAY.site_shift, LAY.site_bits)
    b = abi_insert.CwInsertBatch(lb, abi._ptr(perm), abi._ptr(bits), abi._ptr(yarn), abi._ptr(val),
                                 abi._u64p(toff), abi._ptr(tid), abi._ptr(tca), abi._ptr(tkd), abi._ptr(tval))
    noff, pos = np.full(3, 77, U64), np.full(2, 77, U32)
    out, wr = abi._new_list_result(4, 1, 2, True)
    cols = [np.full(4, 77, U64), np.full(4, 77, U64), np.full(4, 77, U8), np.full(4, 77, U64)]
    r = abi_insert.CwInsertResult(abi._u64p(noff), abi._ptr(pos), wr, *map(abi._ptr, cols))
    keep = (off, toff, idk, ck, kd, perm, bits, yarn, val, tid, tca, tkd, tval, noff, pos, out, cols)
    return b, r, keep


def set_path(s, path, value):
    *head, last = path.split(".")
    for p in head:
        s = getattr(s, p)
    setattr(s, last, value)


BAD = [
    ("b", "docs.doc_offsets", None, "required"), ("b", "tx_offsets", None, "required"),
    ("r", "new_offsets", None, "required"),
    ("b", "docs.doc_offsets", [1, 2, 3], "must be 0"), ("b", "docs.doc_offsets", [0, 3, 2], "monotone"),
    ("b", "tx_offsets", [1, 1, 1], "must be 0"), ("b", "tx_offsets", [0, 2, 1], "monotone"),
    ("b", "weave_perm", None, "null input"), ("b", "visible_bits", None, "null input"),
    ("b", "docs.id_key", None, "null input"), ("b", "docs.cause_key", None, "null input"),
    ("b", "docs.kind", None, "null input"),
    ("b", "tx_id", None, "null tx"), ("b", "tx_cause", None, "null tx"), ("b", "tx_kind", None, "null tx"),
    ("b", "doc_value", None, "go together"), ("b", "tx_value", None, "go together"),
    ("b", "yarn_perm", None, "yarn_perm"), ("b", "docs.site_bits", 0, "yarn_perm"),
    ("r", "id_key", None, "all three or none"), ("r", "kind", None, "all three or none"),
    ("r", "weave.weave_perm", None, "null output"), ("r", "weave.visible_bits", None, "null output"),
    ("r", "weave.visible_count", None, "null output"), ("r", "weave.status", None, "null output"),
    ("m", None, 2, "memspace"), ("nb", None, None, "null batch"), ("nr", None, None, "null batch"),
]


@pytest.mark.parametrize("which,path,value,text", BAD, ids=[f"{w}-{p}-{i}" for i, (w, p, _, _) in enumerate(BAD)])
def test_error_returns_write_nothing_and_the_context_lives_on(weaver, which, path, value, text):
    L = abi_insert.lib()
    b, r, keep = small_call()
    if isinstance(value, list):
        value = np.array(value, U64)
        keep += (value,)
        value = abi._u64p(value)
    if which in ("b", "r"):
        set_path(b if which == "b" else r, path, value)
    rc = L.cw_insert_lists(weaver._h, None if which == "nb" else C.byref(b), None if which == "nr" else C.byref(r),
                           value if which == "m" else abi.CW_MEM_HOST)
    assert rc < 0 and text in L.cw_last_error(weaver._h).decode()
    noff, pos, out, cols = keep[13], keep[14], keep[15], keep[16]
    assert (noff == 77).all() and (pos == 77).all() and not out.weave_perm.any() and (cols[0] == 77).all()
    # ... and the same structs, untouched, are a valid call
    b, r, keep = small_call()
    assert L.cw_insert_lists(weaver._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST) == 0
    assert keep[13].tolist() == [0, 3, 4] and keep[14].tolist() == [2, NONE]
    assert keep[15].weave_perm[:4].tolist() == [0, 1, 2, 0]


def test_a_value_output_without_doc_value_is_an_error(weaver):
    L = abi_insert.lib()
    b, r, keep = small_call()
    b.doc_value = b.tx_value = None
    assert L.cw_insert_lists(weaver._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST) < 0
    assert "doc_value" in L.cw_last_error(weaver._h).decode()


# ------------------------------------------------------- the Python-level calls
def test_causal_insert_lists_and_list_weave_node():
    import random

    from cause_amd import causal as K
    from oracle import causal_ref as R

    rng = random.Random(4)
    sites = [R.new_site_id(rng) for _ in range(4)]
    ref = R.new_list_ct(site_id=sites[0], uuid="u" * 21)
    ct = K.new_list_ct(site_id=sites[0], uuid="u" * 21)
    conv = lambda v: {R.HIDE: K.HIDE, R.H_HIDE: K.H_HIDE, R.H_SHOW: K.H_SHOW}.get(v, v) \
        if isinstance(v, R.Keyword) else v
    for step in range(40):
        site = rng.choice(sites)
        cause = rng.choice(list(ref["nodes"]))
        yarn = ref["yarns"].get(site)
        ts = 1 + max(cause[0], yarn[-1][0][0] if yarn else 0)
        k = rng.choice([1, 1, 3])
        vals = [rng.choice(["a", "b", " ", R.HIDE, R.H_SHOW])] if k == 1 else list("xyz")
        tx = [((ts, site, m), cause if m == 0 else (ts, site, m - 1), vals[m]) for m in range(k)]
        ref = R.insert(R.list_weave, ref, tx[0], tx[1:])
        ktx = [(i, c, conv(v)) for i, c, v in tx]
        if step % 2:
            ct = K.insert(K.list_weave_node, ct, ktx[0], ktx[1:])
        else:
            ct = K.insert_lists([(ct, ktx[0], ktx[1:])])[0]
        assert [(n[0], n[1]) for n in ct["weave"]] == [(n[0], n[1]) for n in ref["weave"]]
        assert K.causal_list_to_edn(ct) == [conv(v) for v in R.causal_list_to_edn(ref)]
        assert {s: [n[0] for n in y] for s, y in ct["yarns"].items()} == \
            {s: [n[0] for n in y] for s, y in ref["yarns"].items()}
        assert ct["lamport_ts"] == ref["lamport_ts"] and set(ct["nodes"]) == set(ref["nodes"])
    again = ct["weave"][3]
    assert K.insert_lists([(ct, again, None)])[0] is ct
    with pytest.raises(K.CauseError) as e:
        K.insert_lists([(ct, (again[0], again[1], "other"), None)])
    assert "edits-not-allowed" in e.value.causes
    with pytest.raises(K.CauseError) as e:
        K.insert_lists([(ct, ((99, sites[1], 0), (98, sites[1], 0), "q"), None)])
    assert "cause-must-exist" in e.value.causes
    ct2 = K.append(K.list_weave_node, ct, K.ROOT_ID, "!")
    assert K.causal_list_to_edn(ct2)[0] == "!" and len(ct2["weave"]) == len(ct["weave"]) + 1
