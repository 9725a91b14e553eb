"""tests/transact_model.py (no GPU): the rules of include/causeweave_transact.h in
their two forms agree on seeded token streams, malformed ones included; and
cause_amd/base.py's transact_bases, with the model standing in for the GPU,
returns what transact_ returns -- on the known answers that tests/test_base.py
holds from the reference, on seeded bases, on follow-up transactions with
several parts into one collection, after undo_, and for the validation errors.
"""
import copy
import random

import numpy as np
import pytest

from cause_amd import abi, abi_transact as A, base as B, causal as C
from tests import invert_model
from tests import renderbase_gen as RG
from tests import transact_model as M

K = RG.K


def strip(cb):
    """A base as transact_ and transact_bases must agree on it: everything but the rng."""
    return {k: v for k, v in cb.items() if k != "_rng"}


def both(cb, tx, fn=M.transact_columns):
    """transact_ and transact_bases on twins of one base (same rng state)."""
    a, b = copy.deepcopy(cb), copy.deepcopy(cb)
    want = B.transact_(a, tx)
    got = B.transact_bases([b], [tx], transact_fn=fn)[0]
    assert strip(got) == strip(want)
    assert list(got["collections"]) == list(want["collections"]) and got["history"] == want["history"]
    assert got["_rng"].random() == want["_rng"].random()      # as many uuids drawn
    return want


def follow_up(rng, cb):
    """A transaction of several parts, some into one collection twice."""
    tx = []
    for _ in range(rng.randint(1, 4)):
        uuid = rng.choice(list(cb["collections"]))
        ct = cb["collections"][uuid]
        v = rng.choice([RG.random_value(rng, 1), RG.random_value(rng, 2), "str", None, C.HIDE, 5])
        if ct["type"] == "map":
            cause = rng.choice([None, rng.choice("abg"), K("k")])
            if cause is None and not isinstance(v, dict):
                v = {rng.choice("ab"): v}
        else:
            cause = rng.choice(list(ct["nodes"]))
            if (v is C.HIDE or v == 5 or isinstance(v, dict)) and cause == C.ROOT_ID and v is C.HIDE:
                v = 7
        tx.append([uuid, cause, v])
        if rng.random() < 0.5:
            tx.append([uuid, cause, RG.random_value(rng, 2)] if ct["type"] == "list" else [uuid, "z", 1])
    return tx


def seeded_cases(seed, n):
    """-> (bases, transactions): seeded bases of tests/renderbase_gen.py, each with a follow-up."""
    rng = random.Random(seed)
    cbs = RG.random_bases(seed, n, history=False)
    return cbs, [follow_up(rng, cb) for cb in cbs]


# ------------------------------------------------------------ the two forms ----
@pytest.mark.parametrize("part", range(8))
def test_the_two_forms_agree_on_seeded_streams(part):
    """4,032 streams in 504 batches of eight: half of the batches with malformed streams,
    a quarter with a tx field of three bits."""
    seen = {0: 0, A.STATUS_TX_MALFORMED: 0, abi.STATUS_KEY_RANGE: 0}
    streams = 0
    for seed in range(part * 63, part * 63 + 63):
        rng = random.Random(seed)
        b = M.random_batch(rng, 8, p_bad=0.3 if seed % 2 else 0.0, site_shift=3 if seed % 4 == 0 else 12)
        x, y = M.transact_recursive(**b), M.transact_columns(**b)
        assert M.same(x, y) == [], seed
        assert M.same(M.transact_recursive(**b, nodes=False), M.transact_columns(**b, nodes=False)) == []
        for st in x.base_status.tolist():
            seen[st] += 1
        streams += len(x.base_status)
    assert streams >= 500 and seen[0] > 200 and seen[A.STATUS_TX_MALFORMED] > 20 and seen[abi.STATUS_KEY_RANGE] > 5


def test_the_rules_on_a_stream_by_hand():
    """{:a [1 "hi" {}] :b "hi"} as a root, then "yo" and 7 into the list: ids,
    causes, documents, refs, runs."""
    L, S, OL, OM, CL, P, RL, RM = range(8)
    lay = M.random_batch(random.Random(0), 0)["layout"]
    toks = [(RM, 0, 0, 2), (OL, 0, 1, 0), (L, 0, 0, 1), (S, 2, 0, 1), (OM, 0, 0, 1), (CL, 0, 0, 0), (CL, 0, 0, 0),
            (S, 2, 2, 0), (CL, 0, 0, 0),
            (P, 0, 77, 1), (S, 2, 0, 1), (L, 0, 0, 1), (CL, 0, 0, 0)]
    col = lambda k, dt: np.array([t[k] for t in toks], dt)
    args = dict(base_doc_offsets=[0, 1], doc_is_map=[0], layout=lay, new_tx=[1000], tok_offsets=[0, len(toks)],
                tok_kind=col(0, np.uint8), tok_arg=col(1, np.uint32), tok_cause=col(2, np.uint64),
                tok_cause_is_id=col(3, np.uint8))
    for fn in (M.transact_recursive, M.transact_columns):
        r = fn(**args)
        assert r.base_status.tolist() == [0] and r.root_doc.tolist() == [1]
        assert r.new_is_map.tolist() == [1, 0, 1] and r.new_open.tolist() == [0, 1, 4]
        assert r.node_offsets.tolist() == [0, 3, 5, 10, 10]
        # document 0 (the existing list): "y" "o" 7 chained from the part's cause
        assert r.node_id[:3].tolist() == [1006, 1007, 1008] and r.node_cause[:3].tolist() == [77, 1006, 1007]
        assert r.node_run[:3].tolist() == [1, 0, 0] and r.node_sub[:3].tolist() == [0, 1, 0]
        # the root map: the ref to the list under key 1, made by the list's CLOSE; "hi" kept whole
        assert r.node_id[3:5].tolist() == [1004, 1005] and r.node_cause[3:5].tolist() == [1, 2]
        assert r.node_ref[3:5].tolist() == [2, A.U32_MAX] and r.node_src[3:5].tolist() == [6, 7]
        # the list: root, 1, "h", "i", the ref to the empty map
        assert r.node_id[5:].tolist() == [0, 1000, 1001, 1002, 1003]
        assert r.node_cause[5:].tolist() == [M.NIL, 0, 1000, 1001, 1002] and r.node_kind[5:].tolist() == [4, 0, 0, 0, 0]
        assert r.node_ref[5:].tolist() == [A.U32_MAX] * 4 + [3] and r.node_run[5:].tolist() == [0, 1, 0, 0, 0]


# --------------------------------------------------------------- the host layer ----
def test_the_known_answers_of_the_reference():
    """base/core_test.cljc:8-15, :60-83, as tests/test_base.py pins transact_."""
    nested = [K("div"), {K("foo"): "bar"}, "wat", [K("p"), "baz"]]
    both(RG.cb0(), [[None, None, nested]])
    cb = both(RG.cb0(), [[None, None, {K("a"): 1}]])
    r = cb["root_uuid"]
    for tx in ([[r, K("a"), "hi"]], [[r, None, {K("a"): 2, K("b"): 3}]], [[r, K("b"), {K("c"): 2}]],
               [[r, K("a"), C.HIDE], [r, None, {K("b"): 2, K("c"): "hi"}], [r, None, {K("b"): C.HIDE}]]):
        both(cb, tx)
    cb = both(RG.cb0(), [[None, None, [1, 2]]])
    r = cb["root_uuid"]
    for v in (0, [0], [-2, -1, 0], "hi", ["hi"], [["hi"]], None, [None, "", [], {}]):
        both(cb, [[r, C.ROOT_ID, v]])
        both(cb, [[r, C.ROOT_ID, v]], fn=M.transact_recursive)
    for value, _, _ in ([{K("a"): {K("aa"): 1, K("bb"): 2, K("cc"): 3}}, 4, 2], [[1, [2, [3]]], 5, 3],
                        [[1, "hello", "world"], 11, 1]):
        both(RG.cb0(), [[None, None, value]])
    both(RG.cb0(), [[None, K("k"), {K("a"): 1}]])      # a root with a key cause: the value nests under it


def test_seeded_bases_follow_ups_and_undo():
    cbs, txs = seeded_cases(20261021, 40)
    want = [B.transact_(cb, tx) for cb, tx in zip(copy.deepcopy(cbs), txs)]
    got = B.transact_bases(copy.deepcopy(cbs), txs, transact_fn=M.transact_columns)
    assert [strip(x) for x in got] == [strip(x) for x in want]
    assert sum(len(tx) for tx in txs) > 80 and sum(len(x["collections"]) for x in want) > 150
    # after undo_: the markers are cleared, the undone nodes stay
    rng = random.Random(3)
    for cb in want[:15]:
        cb = B.undo_(cb, invert_fn=invert_model.invert_columns)
        assert cb["last_undo_lamport_ts"] is not None
        done = both(cb, follow_up(rng, cb))
        assert done["last_undo_lamport_ts"] is None and done["first_undo_lamport_ts"] is None


def test_many_bases_in_one_call():
    calls = []

    def fn(*args):
        calls.append(args)
        return M.transact_columns(*args)

    cbs = [RG.cb0(g) for g in range(5)]
    txs = [[[None, None, [g, "ab", {"k": [g]}]]] for g in range(5)]
    got = B.transact_bases(copy.deepcopy(cbs), txs, transact_fn=fn)
    assert len(calls) == 1 and len(calls[0][3]) == 5
    assert [strip(x) for x in got] == [strip(B.transact_(cb, tx)) for cb, tx in zip(cbs, txs)]
    assert B.transact_bases([], [], transact_fn=fn) == []


def test_the_validation_errors():
    """base/core.cljc:217-227, raised as transact_ raises them, before any call."""
    refuse = lambda *a: pytest.fail("the call was made")
    root = B.transact_(RG.cb0(), [[None, None, [1]]])
    for cb, tx in ((RG.cb0(), [["nope", None, [1]]]), (root, [["nope", None, [1]]]), (RG.cb0(), [[None, None, 5]]),
                   (RG.cb0(), [[None, None, "text"]])):
        with pytest.raises(C.CauseError) as want:
            B.transact_(copy.deepcopy(cb), tx)
        with pytest.raises(C.CauseError) as got:
            B.transact_bases([copy.deepcopy(cb)], [tx], transact_fn=refuse)
        assert str(got.value) == str(want.value)
    # a root first, then a part into it by uuid: the uuid is not known before the transaction
    with pytest.raises(C.CauseError):
        B.tokenize_tx(RG.cb0(), [[None, None, [1]], ["nope", None, [2]]])
    # what s/insert refuses is refused by the insert that follows the call
    for tx in ([[root["root_uuid"], None, 5]], [[root["root_uuid"], (9, "x" * 13, 0), 5]]):
        with pytest.raises(C.CauseError) as want:
            B.transact_(copy.deepcopy(root), tx)
        with pytest.raises(C.CauseError) as got:
            B.transact_bases([copy.deepcopy(root)], [tx], transact_fn=M.transact_columns)
        assert str(got.value) == str(want.value)


def test_a_flagged_base_raises():
    def key_range(*args):
        r = M.transact_columns(*args)
        r.base_status[0] = abi.STATUS_KEY_RANGE
        return r

    with pytest.raises(C.CauseError) as e:
        B.transact_bases([RG.cb0()], [[[None, None, [1]]]], transact_fn=key_range)
    assert e.value.causes == {"key-range"}
