"""tests/render_model.py (the numpy model cw_render_lists / cw_render_maps are
tested against on the GPU) pinned to the reference's own answers, on the CPU:
the weave and the hide? flags come from oracle/causal_ref.py, the model
renders them, and the result is causal_ref's causal-list->edn / count
(list.cljc:57-77) and causal-map->edn / count- (map.cljc:68-73, 94-103) for
the fixtures of tests/golden/edge_cases.json.  Also: the header declares the
two calls and the ctypes structs have the header's layout."""
import ctypes
import random

import numpy as np

from cause_amd import abi
from oracle import causal_ref as R
from tests import render_model as M
from tests.test_golden import EDGE, case_nodes, _edn_json


def list_arrays(cts):
    """A batch of woven reference cts as the arrays of a cw_list_result: the
    offsets, weave_perm (indices into each ct's node list), the hide? flags
    (list.cljc:48-55) and a value table with one token per node."""
    off, perm, vis, tokens, values = [0], [], [], [], []
    for ct in cts:
        nodes = list(ct["nodes"])
        where = {i: k for k, i in enumerate(nodes)}
        w = ct["weave"]
        perm += [where[n[0]] for n in w]
        vis += [0 if R.hide_q(n, w[k + 1] if k + 1 < len(w) else None) else 1 for k, n in enumerate(w)]
        tokens += list(range(len(values), len(values) + len(nodes)))
        values += [ct["nodes"][i][1] for i in nodes]
        off.append(len(perm))
    return (np.array(off, np.uint64), np.array(perm, np.uint32), np.array(vis, np.uint8),
            np.array(tokens, np.uint32), values)


def check_lists(cts):
    off, perm, vis, tokens, values = list_arrays(cts)
    r = M.render_lists(off, perm, M.pack_bits(vis, ones_above=True), tokens)
    assert len(r.offsets) == len(cts) + 1 and r.offsets[0] == 0
    for d, ct in enumerate(cts):
        lo, hi = int(r.offsets[d]), int(r.offsets[d + 1])
        want = R.causal_list_to_edn(ct)
        assert [values[t] for t in r.value[lo:hi]] == want
        assert hi - lo == len(want)  # (count list), list.cljc:77
        nodes = list(ct["nodes"])
        assert [nodes[s] for s in r.src[lo:hi]] == [n[0] for n in R.causal_list_to_list(ct)]


def test_list_edn_of_the_edge_cases():
    cts = []
    for ci, c in enumerate(EDGE["cases"]):
        nodes = case_nodes(c)
        random.Random(ci).shuffle(nodes)
        ct = R.new_list_ct()
        ct["nodes"] = {n[0]: (n[1], n[2]) for n in nodes}
        ct = R.list_weave(ct)
        assert R.causal_list_to_edn(ct) == c["edn"]
        cts.append(ct)
    cts.insert(3, R.new_list_ct())  # a document that renders nothing (the root alone)
    check_lists(cts)


def test_list_edn_through_hide_and_show():
    want = EDGE["known_answers"]["list_hide_show"]["edn_after_each"]
    ct = R.new_list_ct(rng=random.Random(3))
    for v in "abc":
        ct = R.list_conj(ct, v)
    a_id = ct["weave"][1][0]
    cts = [ct]
    for v in (R.HIDE, R.H_SHOW, R.HIDE, R.H_SHOW):
        ct = R.append(R.list_weave, ct, a_id, v)
        cts.append(ct)
    assert [R.causal_list_to_edn(c) for c in cts] == want
    check_lists(cts)


def map_arrays(cts):
    """A batch of woven reference map cts as seg_coll / seg_key / seg_active of
    a cw_map_result (key weaves per collection in key-token order), with the
    key table, coll_offsets and a value table."""
    keys, coll, key, act, co, tokens, values = [], [], [], [], [0], [], []
    for d, ct in enumerate(cts):
        nodes = list(ct["nodes"])
        where = {i: k for k, i in enumerate(nodes)}
        for k in sorted(ct["weave"], key=repr):
            if k not in keys:
                keys.append(k)
            n = R.active_node(k, ct["weave"][k])
            coll.append(d)
            key.append(keys.index(k))
            act.append(-1 if n is R.BLANK else where[n[0]])
        tokens += list(range(len(values), len(values) + len(nodes)))
        values += [ct["nodes"][i][1] for i in nodes]
        co.append(len(tokens))
    return (np.array(coll, np.uint32), np.array(key, np.uint64), np.array(act, np.int64),
            np.array(co, np.uint64), np.array(tokens, np.uint32), keys, values)


def check_maps(cts):
    coll, key, act, co, tokens, keys, values = map_arrays(cts)
    r = M.render_maps(len(cts), coll, key, act, co, tokens)
    assert len(r.offsets) == len(cts) + 1 and r.offsets[0] == 0
    for d, ct in enumerate(cts):
        lo, hi = int(r.offsets[d]), int(r.offsets[d + 1])
        got = {keys[k]: values[t] for k, t in zip(r.key[lo:hi].tolist(), r.value[lo:hi].tolist())}
        assert got == R.causal_map_to_edn(ct)
        assert hi - lo == R.map_count(ct)  # count-, map.cljc:68-73
        nodes = list(ct["nodes"])
        assert sorted(nodes[s] for s in r.src[lo:hi]) == sorted(n[0] for n in R.causal_map_to_list(ct))


def test_map_edn_through_hide_and_show():
    ka = EDGE["known_answers"]
    foo, fizz, a = R.Keyword(None, "foo"), R.Keyword(None, "fizz"), R.Keyword(None, "a")
    ct = R.map_assoc(R.map_assoc(R.new_map_ct(rng=random.Random(5)), foo, "bar"), fizz, "buzz")
    cts = [R.new_map_ct(rng=random.Random(6)), ct]  # (an empty collection first)
    for v in (R.HIDE, R.H_SHOW, R.HIDE, R.H_SHOW):
        ct = R.append(R.map_weave, ct, foo, v)
        cts.append(ct)
    for v in ("boo", R.H_SHOW, R.H_SHOW):
        ct = R.append(R.map_weave, ct, foo, v)
    cts.append(ct)
    assert [_edn_json(R.causal_map_to_edn(c)) for c in cts[1:]] == ka["map_hide_show"]["edn_after_each"]
    # every key blank, then the F8a quirk
    gone = R.map_dissoc(R.map_assoc(R.new_map_ct(rng=random.Random(5)), a, 1), a)
    assert R.map_count(gone) == 0 and gone["weave"]
    cts.append(gone)
    quirk = R.map_assoc(gone, a, 2)
    assert _edn_json(R.causal_map_to_edn(quirk)) == ka["map_quirk_f8a"]["edn"]
    cts += [quirk, R.new_map_ct(rng=random.Random(7))]
    check_maps(cts)


def test_model_bounds_and_ignored_bits():
    """An out-of-range weave_perm entry gets value 0; bits past N do not count."""
    off = np.array([0, 0, 3, 3, 5], np.uint64)
    perm = np.array([0, 7, 2, 1, 0], np.uint32)
    vis = np.array([0, 1, 1, 1, 0], np.uint8)
    val = np.array([10, 11, 12, 20, 21], np.uint16)
    for above in (False, True):
        r = M.render_lists(off, perm, M.pack_bits(vis, ones_above=above), val)
        assert r.offsets.tolist() == [0, 0, 2, 2, 3]
        assert r.src.tolist() == [7, 2, 1] and r.value.tolist() == [0, 12, 21]
    m = M.render_maps(3, [0, 0, 2], [5, 6, 5], [1, -1, 9], [0, 2, 2, 4], np.array([1, 2, 3, 4], np.uint8))
    assert m.offsets.tolist() == [0, 1, 1, 2] and m.key.tolist() == [5, 5]
    assert m.src.tolist() == [1, 9] and m.value.tolist() == [2, 0]


def test_header_declares_the_render_calls():
    names = abi.header_functions()
    assert "cw_render_lists" in names and "cw_render_maps" in names
    L = abi.lib()
    assert hasattr(L, "cw_render_lists") and hasattr(L, "cw_render_maps")
    # pointers and u64 are 8 bytes, naturally aligned on x86-64
    assert ctypes.sizeof(abi.CwRenderBatch) == 8 * 4 + 4 * 2 + 8
    assert ctypes.sizeof(abi.CwRenderResult) == 8 * 3
    assert ctypes.sizeof(abi.CwMapRenderBatch) == 8 * 6 + 8 + 8
    assert abi.CwMapRenderBatch.value.offset == 56 and abi.CwRenderBatch.value.offset == 40
    assert ctypes.sizeof(abi.CwMapRenderResult) == 8 * 4
