"""cause_amd/base.py's undo machinery on the CPU: tx_id_indexes, subhis,
get_next_tx_id, the undo markers and the reference's undo / redo sequences
(tests/golden/invert_cases.json), with tests/invert_model.invert_columns
injected in place of the cw_invert call and the CPU reference (oracle/
causal_ref.py) reweaving the collections to read the values."""
import json
import os
import random

import pytest

from cause_amd import base as B, causal as C
from oracle import causal_ref as R
from tests import invert_model as M

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "invert_cases.json")))
MODEL = M.invert_columns
R_KW = {C.HIDE: R.HIDE, C.H_HIDE: R.H_HIDE, C.H_SHOW: R.H_SHOW}


def value_of(v):
    if v == ":causal/hide":
        return C.HIDE
    return v


def play_txs(txs, seed=0):
    """The golden txs transacted into a new base."""
    cb = B.new_cb(random.Random(seed))
    for tx in txs:
        parts = []
        for uuid, cause, value in tx:
            parts.append((cb["root_uuid"] if uuid == "root" else uuid,
                          C.ROOT_ID if cause == "root-id" else cause, value_of(value)))
        cb = B.transact_(cb, parts)
    return cb


def cpu_edn(cb, uuid=None):
    """The collection's value by the CPU reference's full reweave, refs resolved."""
    ct = cb["collections"][uuid or cb["root_uuid"]]
    rct = {"type": ct["type"], "lamport_ts": 0, "uuid": ct["uuid"], "site_id": ct["site_id"], "weave": None,
           "nodes": {i: (c, R_KW.get(v, v) if isinstance(v, C.Keyword) else v) for i, (c, v) in ct["nodes"].items()}}
    deref = lambda v: cpu_edn(cb, B.ref_to_uuid(v)) if B.is_ref(v) else v
    if ct["type"] == "list":
        return [deref(v) for v in R.causal_list_to_edn(R.list_weave(rct))]
    return {k: deref(v) for k, v in R.causal_map_to_edn(R.map_weave(rct)).items()}


def test_new_cb_and_transact_keep_the_markers_clear():
    cb = play_txs(GOLDEN["get_next_tx_id"]["txs"])
    assert (cb["first_undo_lamport_ts"], cb["last_undo_lamport_ts"], cb["last_redo_lamport_ts"]) == (None,) * 3
    cb = dict(cb, first_undo_lamport_ts=2, last_undo_lamport_ts=2, last_redo_lamport_ts=1)
    cb = B.transact_(cb, [(cb["root_uuid"], "z", 1)])
    assert (cb["first_undo_lamport_ts"], cb["last_undo_lamport_ts"], cb["last_redo_lamport_ts"]) == (None,) * 3
    old = {k: v for k, v in cb.items() if not k.endswith("_lamport_ts") or k == "lamport_ts"}
    assert B.get_next_tx_id(old, old.get("last_undo_lamport_ts")) == (3, cb["site_id"])   # a dict without them


def test_tx_id_indexes():
    g = GOLDEN["tx_id_indexes"]
    cb = play_txs(g["txs"])
    last = cb["history"][-1][0][:2]
    assert list(B.tx_id_indexes(cb, last)) == g["last_tx"]
    assert all(rp[0][0] == 2 for rp in B._sorted_history(cb)[2:5])
    assert list(B.tx_id_indexes(cb, (1, "bad site-id"))) == g["bad_site"]
    assert B.tx_id_indexes(cb, None) == (None, None)


def test_subhis():
    g = GOLDEN["subhis"]
    cb = play_txs(g["txs"])
    hist = B._sorted_history(cb)
    names = {"last": hist[-1][0][:2], "first": hist[0][0][:2]}
    counts = []
    for call in g["calls"]:
        args = [names.get(a, a) if isinstance(a, str) else None if a is None else (a[0], cb["site_id"])
                for a in call]
        counts.append(len(B.subhis(cb, *args)))
    assert counts == g["counts"]
    shuffled = dict(cb, history=list(reversed(cb["history"])))       # a merged history is not in order
    assert B.subhis(shuffled, names["last"]) == B.subhis(cb, names["last"])


def test_get_next_tx_id():
    cb = play_txs(GOLDEN["get_next_tx_id"]["txs"])
    for last_undo, ts in GOLDEN["get_next_tx_id"]["last_undo_then_ts"]:
        got = B.get_next_tx_id(dict(cb, last_undo_lamport_ts=last_undo), last_undo)
        assert (got[0] if got else None) == ts and (got is None or got[1] == cb["site_id"])


def test_invert_path():
    g = GOLDEN["invert_path"]
    u, cause, value = B.invert_path({"uuid": g["uuid"], "node": (tuple(g["node"][0]), g["node"][1], g["node"][2])})
    assert [u, list(cause), repr(value)] == g["expect"]


def test_invert_of_the_whole_history():
    g = GOLDEN["invert"]
    cb = play_txs(g["txs"])
    assert cpu_edn(cb)["a"] == g["a_before"] and len(cb["history"]) == g["history_before"]
    ts = cb["lamport_ts"]
    out = B.invert_(cb, cb["history"], invert_fn=MODEL)
    assert cpu_edn(out).get("a") is g["a_after"] and len(out["history"]) == g["history_after"]
    assert out["lamport_ts"] == ts + 1 and len(cb["history"]) == g["history_before"]
    new = out["history"][g["history_before"]:]
    assert [i for i, _ in new] == [(ts, cb["site_id"], k) for k in range(5)]
    assert {u for _, u in new} == {cb["root_uuid"]}      # the nested list made no parts
    assert all(ct.get("_dirty") for u, ct in out["collections"].items() if u == cb["root_uuid"])
    with pytest.raises(ValueError):
        B.invert_(cb, cb["history"][::2], invert_fn=MODEL)


@pytest.mark.parametrize("case", ["undo_redo_map", "undo_redo_list"])
def test_undo_and_redo(case):
    g = GOLDEN[case]
    cb = play_txs(g["txs"])
    read = (lambda c: {k: cpu_edn(c).get(k) for k in g["start"]}) if case.endswith("map") else \
        (lambda c: (cpu_edn(c) or [None])[0])
    assert read(cb) == g["start"]
    undone = 0
    for op, want in g["steps"]:
        before = cb
        cb = (B.undo_ if op == "undo" else B.redo_)(cb, invert_fn=MODEL)
        assert read(cb) == want, (op, want)
        if op == "undo":
            undone += 1
            assert cb["first_undo_lamport_ts"] == len(g["txs"]) and cb["last_redo_lamport_ts"] is None
            assert cb["last_undo_lamport_ts"] == len(g["txs"]) - undone + 1
        elif cb is not before:
            assert cb["last_redo_lamport_ts"] is not None and cb["first_undo_lamport_ts"] == len(g["txs"])
    if case.endswith("list"):
        assert cb is before                      # the fourth redo has nothing left: the same base


def test_undo_with_nothing_to_undo_and_redo_without_an_undo():
    cb = B.new_cb(random.Random(1))
    assert B.undo_(cb, invert_fn=MODEL) is cb and B.redo_(cb, invert_fn=MODEL) is cb
    cb = play_txs(GOLDEN["undo_redo_map"]["txs"])
    assert B.redo_(cb, invert_fn=MODEL) is cb


def test_reset_and_invert_bases():
    g = GOLDEN["undo_redo_map"]
    cb = play_txs(g["txs"])
    out = B.reset_(cb, (1, cb["site_id"]), [cb["site_id"]], invert_fn=MODEL)
    assert cpu_edn(out) == {} and len(out["history"]) == 6
    assert B.reset_(cb, (2, cb["site_id"]), ["another site"], invert_fn=MODEL)["history"] == cb["history"]
    cbs = [play_txs(GOLDEN[c]["txs"], seed) for seed, c in enumerate(["undo_redo_map", "undo_redo_list", "invert"])]
    slices = [B.subhis(c, (2, c["site_id"])) for c in cbs]
    many = B.invert_bases(cbs, slices, invert_fn=MODEL)
    for c, sl, got in zip(cbs, slices, many):
        one = B.invert_(c, sl, invert_fn=MODEL)
        assert got["history"] == one["history"] and got["lamport_ts"] == one["lamport_ts"]
        assert {u: ct["nodes"] for u, ct in got["collections"].items()} == \
            {u: ct["nodes"] for u, ct in one["collections"].items()}
