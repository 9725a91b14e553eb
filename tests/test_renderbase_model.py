"""tests/renderbase_model.py (no GPU): the contract of cw_render_bases as the
header states it (the recursive form) against the path renderbase.hip takes
(the column form), and both against cause_amd/base.py: bases_to_edn with the
model as render_fn and the CPU reference's weaves must give what cb_to_edn gives.
"""
import random

import numpy as np
import pytest

from cause_amd import abi_render_bases as A, base as B, causal as C
from tests import renderbase_gen as G
from tests import renderbase_model as M

U32, U64 = np.uint32, np.uint64
NONE = A.U32_MAX
O, X, L, N = A.TOK_OPEN, A.TOK_CLOSE, A.TOK_LEAF, A.TOK_NIL


def both(off, ref, root):
    a = M.render_recursive(off, ref, root)
    M.same(M.render_columns(off, ref, root), a)
    return a


def toks(r):
    return list(zip(r.tok_kind.tolist(), r.tok_doc.tolist(), r.tok_entry.tolist()))


def test_a_worked_example():
    """doc 0 = [s, ->1, s, ->2], doc 1 = [], doc 2 = [->9 (dangling), s]; doc 3 unclaimed."""
    off, ref = [0, 4, 4, 6, 7], [NONE, 1, NONE, 2, 9, NONE, NONE]
    r = both(off, ref, [0, 7])
    assert toks(r) == [(O, 0, NONE), (L, 0, 0), (O, 1, 1), (X, 1, 1), (L, 0, 2), (O, 2, 3), (N, 2, 4), (L, 2, 5),
                       (X, 2, 3), (X, 0, NONE)]
    assert r.base_tok_offsets.tolist() == [0, 10, 10] and r.base_status.tolist() == [0, 0]
    assert r.doc_base.tolist() == [0, 0, 0, NONE] and r.doc_open.tolist()[:3] == [0, 2, 5]


def test_empty_root_and_no_root():
    r = both([0, 0], [], [0, 1, NONE])
    assert toks(r) == [(O, 0, NONE), (X, 0, NONE)] and r.base_tok_offsets.tolist() == [0, 2, 2, 2]
    assert r.base_status.tolist() == [0, 0, 0]


@pytest.mark.parametrize("off,ref,root,status", M.SHARED_CASES)
def test_shared_and_cycles(off, ref, root, status):
    r = both(off, ref, root)
    assert r.base_status.tolist() == status
    for g, st in enumerate(status):
        if st:
            assert r.base_tok_offsets[g] == r.base_tok_offsets[g + 1] and g not in r.doc_base.tolist()


def test_an_isolated_cycle_has_no_base():
    r = both([0, 1, 2, 3], [NONE, 2, 1], [0])
    assert r.doc_base.tolist() == [0, NONE, NONE] and len(r.tok_kind) == 3


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 3000])
def test_chains(n):
    """n nested single-entry documents, the numbering reversed (children first)."""
    off = np.arange(n + 1, dtype=U64)
    ref = np.array([NONE] + list(range(n - 1)), U32)        # document d holds a ref to d - 1
    r = both(off, ref, [n - 1])
    assert len(r.tok_kind) == 2 * n + 1 and r.tok_kind.tolist() == [O] * n + [L] + [X] * n
    assert r.doc_open.tolist() == list(range(n - 1, -1, -1))
    assert M.rounds_for(512) == 10 and M.rounds_for(513) == 11 and M.rounds_for(1) == 1


def test_random_tables():
    rng = random.Random(20261021)
    bases = flagged = cycles = nils = 0
    for _ in range(4000):
        D, Gn = rng.randint(0, 16), rng.randint(0, 5)
        off, ref, root = M.random_table(rng, D, Gn)
        r = both(off, ref, root)
        bases += Gn
        flagged += int((r.base_status != 0).sum())
        nils += int((r.tok_kind == N).sum())
        cl = M.claims_of(off.astype(np.int64), ref.astype(np.int64), root.astype(np.int64), D)
        cycles += int(((cl == 1) & (r.doc_base == NONE)).any()) if D else 0
        T = int(r.base_tok_offsets[-1])
        assert T <= len(ref) + 2 * D and T == len(r.tok_kind)
    assert bases > 8000 and flagged > 1500 and bases - flagged > 4000 and cycles > 500 and nils > 300


# ------------------------------------------------------------- base.py ----
def edn_both_ways(cbs):
    """bases_to_edn through the model (both forms) and cb_to_edn, all on CPU weaves."""
    woven = [G.cpu_weave_all(cb) for cb in cbs]
    want = [B.cb_to_edn(cb)[0] for cb in woven]
    seen = []

    def model(off, ref, root):
        seen.append(both(off, ref, root))
        return seen[-1]

    got = B.bases_to_edn(woven, render_fn=model, entries_fn=G.cpu_entries)
    assert got == want
    return got, seen[0]


def test_the_references_known_answers():
    cases = G.known_answers()
    got, res = edn_both_ways([cb for cb, _ in cases])
    assert got == [want for _, want in cases]
    assert not res.base_status.any()
    assert got[0] is None and res.base_tok_offsets[1] == 0


def test_plain_nested_values_are_never_flagged():
    cbs = G.random_bases(7, 60, history=False)
    got, res = edn_both_ways(cbs)
    assert not res.base_status.any()                     # transact_ of plain values makes trees
    assert sum(isinstance(v, (list, dict)) for v in got) == 60
    depth = lambda v: 1 + max([depth(x) for x in (v.values() if isinstance(v, dict) else v)] + [0]) \
        if isinstance(v, (list, dict)) else 0
    assert max(depth(v) for v in got) >= 4
    unreached = sum(1 for d in res.doc_base.tolist() if d == NONE)
    assert unreached > 10                                # replaced and hidden subtrees are not rendered


def test_undo_and_redo_hide_and_show_subtrees():
    cbs = G.random_bases(11, 60)
    got, res = edn_both_ways(cbs)
    assert not res.base_status.any()
    assert sum(len(cb["collections"]) for cb in cbs) == len(res.doc_base)
    assert (res.doc_base == NONE).sum() > 20


def test_a_transacted_ref_is_flagged_and_takes_the_host_route():
    cb = B.transact_(G.cb0(3), [[None, None, {"a": [1, 2], "b": {"c": 3}}]])
    inner = [u for u, ct in cb["collections"].items() if ct["type"] == "list"][0]
    twice = B.transact_(cb, [[cb["root_uuid"], "again", B.uuid_to_ref(inner)]])
    plain = G.random_bases(5, 3, history=False)
    got, res = edn_both_ways([plain[0], twice, plain[1], cb, plain[2]])
    assert res.base_status.tolist() == [0, A.STATUS_REF_SHARED, 0, 0, 0]
    assert got[1] == {"a": [1, 2], "again": [1, 2], "b": {"c": 3}} and got[3] == {"a": [1, 2], "b": {"c": 3}}


def test_a_ref_to_a_collection_the_base_lacks_is_nil():
    cb = B.transact_(G.cb0(4), [[None, None, {"a": 1}]])
    cb = B.transact_(cb, [[cb["root_uuid"], "gone", B.uuid_to_ref("no-such-collection")]])
    got, res = edn_both_ways([cb])
    assert got == [{"a": 1, "gone": None}] and not res.base_status.any() and (res.tok_kind == N).sum() == 1


def test_a_reference_cycle_raises_as_cb_to_edn_does():
    cb = B.transact_(G.cb0(5), [[None, None, {"a": [1]}]])
    cb = G.cpu_weave_all(B.transact_(cb, [[cb["root_uuid"], "self", B.uuid_to_ref(cb["root_uuid"])]]))
    with pytest.raises(C.CauseError):
        B.cb_to_edn(cb)
    with pytest.raises(C.CauseError):
        B.bases_to_edn([cb], render_fn=M.render_columns, entries_fn=G.cpu_entries)
