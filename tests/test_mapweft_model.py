"""The CPU model of the map weft (tests/mapweft_model.py) against the restatement
R.weft, the conditions on the inputs of tests/test_gpu_map_weft.py, and the ABI
surface of cw_weft_maps -- no GPU.

R.map_weave unpacks ``i, cause, v = node`` and cannot take weft's one-element
node [id].  The reference's map weave destructures it (map.cljc:30) to cause nil
and value nil, so these tests hand R.weft a weave-fn (mapweft_model.
padded_map_weave) that pads a body () to (None, None) for the fold and restores
``nodes`` afterwards; oracle/ is unchanged.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from cause_amd import abi, causal, pack
from oracle import causal_ref as R
from tests import jvm_twins
from tests import mapweft_model as M


def _mv(v):
    return causal.Keyword(v.ns, v.name) if isinstance(v, R.Keyword) else v


def _mnode(n):
    return n if len(n) == 1 else (n[0], n[1], _mv(n[2]))


def mirror_ct(ref):
    ct = causal.new_map_ct(site_id=ref["site_id"], uuid=ref["uuid"])
    ct["nodes"] = {i: (c, _mv(v)) for i, (c, v) in ref["nodes"].items()}
    ct["lamport_ts"] = ref["lamport_ts"]
    return ct


def check_mirror(items, got):
    """got[k] (causal.weft_maps of the items) == R.weft per item; -> (checked,
    gibberish, with an [id] node)."""
    assert len(got) == len(items)
    gibberish = bogus = 0
    for (ref, ids), g in zip(items, got):
        want = M.reference_weft(ref, ids)
        kept = set(want["nodes"])
        gibberish += any(len(b) and R.valid_id(b[0]) and b[0] not in kept for b in want["nodes"].values())
        bogus += any(len(b) == 0 for b in want["nodes"].values())
        assert g["weave"] == {k: [_mnode(n) for n in kw] for k, kw in want["weave"].items()}
        assert g["nodes"] == {i: tuple(_mv(x) for x in b) for i, b in want["nodes"].items()}
        assert g["yarns"] == {s: [_mnode(n) for n in y] for s, y in want["yarns"].items()}
        assert g["lamport_ts"] == want["lamport_ts"]
        assert (g["site_id"], g["uuid"]) == (ref["site_id"], ref["uuid"])
        assert causal.causal_map_to_edn(g) == {k: _mv(v) for k, v in R.causal_map_to_edn(want).items()}
        for k in list(want["weave"]) + ["a", "never"]:
            assert causal.map_get(g, k) == _mv(R.map_get(want, k)), k
    return len(items), gibberish, bogus


class ModelWeaver:
    """Stands in for abi.Weaver: weft_maps answers with the model's arrays."""

    calls = 0

    def weft_maps(self, offsets, id_key, cause, cause_is_id, kind, token_bits, site_shift,
                  site_bits, cut, key_bits=0):
        self.calls += 1
        e = M.weft_maps_expected(offsets, id_key, cause, cause_is_id, kind, site_shift, site_bits, cut)
        assert not e.dup.any()
        so, sc, sk, sa, sp = [0], [], [], [], []
        for d, fold in enumerate(e.folds):
            for key in sorted(fold):  # per collection in ascending seg_key order
                act, members = fold[key]
                sc.append(d)
                sk.append(key)
                sa.append(act)
                sp += [0xFFFFFFFF] + members
                so.append(len(sp))
        maps = abi.MapResult(np.array(so, np.uint64), np.array(sc, np.uint32), np.array(sk, np.uint64),
                             np.array(sa, np.int64), np.array(sp, np.uint32),
                             e.weft.astype(np.uint32))
        return abi.MapWeftResult(e.offsets, e.src, maps)


def test_mirror_through_the_model(monkeypatch):
    """causal.weft_maps over the model's arrays == R.weft, all items in ONE batch
    call (site ranks and cut rows differ per collection)."""
    stand_in = ModelWeaver()
    monkeypatch.setattr(causal, "weaver", lambda: stand_in)
    items = M.mirror_items()
    got = causal.weft_maps([(mirror_ct(ref), ids) for ref, ids in items])
    assert stand_in.calls == 1
    checked, gibberish, bogus = check_mirror(items, got)
    assert checked > 30 and gibberish > 3 and bogus > 3, (checked, gibberish, bogus)


def test_select_by_hand():
    """Four collections, every array spelled out: a cut at a node, a cut id that
    is no node, a cut that loses a cause, no site named."""
    s1, s2 = "aaaaaaaaaaaaa", "bbbbbbbbbbbbb"
    doc = [((1, s1, 0), "k", "x"), ((2, s2, 0), (1, s1, 0), causal.H_HIDE), ((3, s1, 0), "k", "y")]
    pm = pack.pack_maps([doc, doc, doc, doc], min_site_bits=2)
    lay, S = pm.layout, 4
    rk = pm.ranks[0]
    assert lay.site_bits == 2 and rk == {"0": 0, s1: 1, s2: 2}
    cut = np.zeros(4 * S, np.uint64)
    cut[0 * S + rk[s1]] = lay.pack(1, rk[s1], 0)
    cut[1 * S + rk[s1]] = lay.pack(5, rk[s1], 0)          # no node with that id
    cut[1 * S + rk[s2]] = lay.pack(2, rk[s2], 0)
    cut[2 * S + rk[s2]] = lay.pack(2, rk[s2], 0)          # the undo node without its cause
    ko, kid, kca, kci, kkd, ksrc, weft = M.weft_select_maps(
        pm.offsets, pm.id_key, pm.cause, pm.cause_is_id, pm.kind, lay.site_shift, lay.site_bits, cut)
    assert list(ko) == [0, 1, 5, 6, 6]
    assert list(ksrc) == [0, 0, 1, 2, M.NO_SRC, 1]
    assert list(kid[1:5]) == list(pm.id_key[:3]) + [lay.pack(5, rk[s1], 0)]
    assert (kca[4], kci[4], kkd[4]) == (0, 2, 0)
    assert list(weft) == [0, abi.STATUS_WEFT, 0, 0]
    e = M.weft_maps_expected(pm.offsets, pm.id_key, pm.cause, pm.cause_is_id, pm.kind,
                             lay.site_shift, lay.site_bits, cut)
    nil = (1 << 64) - 1
    tok = int(pm.cause[0])
    assert e.folds[0] == {tok: (0, [0])}
    assert e.folds[1] == {tok: (2, [2, 0, 1]), nil: (3, [3])}   # [id] woven under the nil key
    assert e.folds[2] == {nil: (-1, [0])}                       # its cause was cut away
    assert e.folds[3] == {}
    assert M.status_classes(e, (pm.offsets,)) == dict(plain=1, weft=1, emptied=1, gibberish=1)


def test_select_refuses_a_cut_word_of_another_site():
    a = list(M.case("small")[:8])
    a[7] = a[7].copy()
    a[7][2] = (3 << a[6]) | 5  # rank 2's word holds an id of rank 5
    with pytest.raises(ValueError):
        M.weft_select_maps(*a)


@pytest.mark.parametrize("name", list(M.CASES))
def test_no_kept_collection_of_a_gpu_input_repeats_an_id(name):
    """The weave of a collection with CW_STATUS_DUP is unspecified: no kept
    collection of any GPU case has one, so the GPU comparison skips none."""
    e = M.expected(name)
    assert not e.dup.any()
    off = M.case(name)[0]
    assert len(e.folds) == len(off) - 1 == len(e.weft)


def test_inputs_reach_the_edges_they_are_for():
    sizes = lambda name: np.diff(M.case(name)[0].astype(np.int64))
    kept = lambda name: np.diff(M.expected(name).offsets.astype(np.int64))
    n = sizes("boundaries")
    assert len(n) >= 60 and set(M.BOUNDARY_SIZES) <= set(n.tolist()) and M.case("boundaries")[6] == 4
    cls = M.status_classes(M.expected("boundaries"), M.case("boundaries"))
    assert all(v > 0 for v in cls.values()), cls
    assert [int(sizes(f"pack{k}").max()) for k in (512, 1024, 2048)] == [512, 1024, 2048]
    n = sizes("lookback")
    assert len(n) == 2500 and n.min() >= 40 and n.max() <= 60 and n.sum() / 512 > 200
    assert M.case("bits1")[6] == 1 and M.case("bits10")[6] == 10
    a = M.case("all_ranks_absent")
    assert a[6] == 10 and int(M.expected("all_ranks_absent").offsets[-1]) == len(a[1]) + 1024
    rows = M.case("upper_words")[7].reshape(-1, 1024)
    assert not rows[:, :32].any() and rows[:, 32:].any(axis=1).all()
    assert sizes("kept_over_2048")[1] == 2048 and kept("kept_over_2048")[1] == 2048 + 16
    assert sizes("oversize").max() == 2049
    e = M.expected("empty_named")
    assert kept("empty_named").tolist() == [0, 1, 0] and e.weft.tolist() == [0, abi.STATUS_WEFT, 0]
    assert e.src.tolist() == [M.NO_SRC]
    assert kept("all_empty").tolist() == [0, 0, 0] and len(M.expected("d0").folds) == 0


# ------------------------------------------------------------------ the ABI surface
def _header_layout(name):
    """[(field, size, offset)] and the size of typedef `name` of the header; a
    field whose type is another typedef of the header takes that struct's size
    (8-byte aligned, as every struct of the header is)."""
    src = open(jvm_twins.HEADER).read()
    flat = jvm_twins.header_structs(src)
    size_of = lambda fields: (fields[-1][3] + fields[-1][2] + 7) // 8 * 8
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;",
                     jvm_twins._strip_c_comments(src)).group(1)
    out, off = [], 0
    for decl in filter(str.strip, body.split(";")):
        typ, fname = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*\*?\s*(\w+)\s*", decl).groups()
        if typ in flat and "*" not in decl:
            size, align = size_of(flat[typ]), 8
        else:
            size = align = jvm_twins._c_field(decl)[2]
        off = (off + align - 1) // align * align
        out.append((fname, size, off))
        off += size
    return out, (off + 7) // 8 * 8


@pytest.mark.parametrize("cname, cls", [("cw_map_weft_batch", "CwMapWeftBatch"),
                                        ("cw_map_weft_result", "CwMapWeftResult")])
def test_ctypes_structs_match_the_header(cname, cls):
    fields, size = _header_layout(cname)
    st = getattr(abi, cls)
    assert ctypes.sizeof(st) == size
    assert [(f, getattr(st, f).size, getattr(st, f).offset) for f, _ in st._fields_] == fields


def test_cw_weft_maps_is_declared_bound_and_exported():
    assert "cw_weft_maps" in abi.header_functions()
    assert "cw_weft_maps" in jvm_twins.header_functions(open(jvm_twins.HEADER).read())
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("libcauseweave.so not built")
    L = abi.lib()
    assert L.cw_weft_maps.restype is ctypes.c_int and len(L.cw_weft_maps.argtypes) == 4
    assert hasattr(abi.Weaver, "weft_maps") and hasattr(abi.Weaver, "weft_maps_device")


def test_pack_maps_defaults_are_unchanged():
    """pack_maps with the new arguments left out, or given their defaults,
    returns what it did: compared field by field on one batch with the arrays
    spelled out."""
    s1, s2 = "aaaaaaaaaaaaa", "bbbbbbbbbbbbb"
    docs = [[((1, s1, 0), "k", "x"), ((2, s2, 0), (1, s1, 0), causal.H_HIDE), ((3, s1, 1), None, 4)],
            [], [((7, s2, 0), "j", causal.HIDE)]]
    a, b = pack.pack_maps(docs), pack.pack_maps(docs, extra_ids=None, min_site_bits=0)
    for f in ("offsets", "id_key", "cause", "cause_is_id", "kind"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("layout", "token_bits", "keys", "docs", "ranks"):
        assert getattr(a, f) == getattr(b, f), f
    lay = a.layout
    assert (lay.ts_bits, lay.site_bits, lay.tx_bits, a.token_bits) == (3, 2, 1, 1)
    assert a.offsets.tolist() == [0, 3, 3, 4] and a.keys == ["k", "j"]
    assert a.ranks == [{"0": 0, s1: 1, s2: 2}, {"0": 0}, {"0": 0, s2: 1}]
    assert a.id_key.tolist() == [lay.pack(1, 1, 0), lay.pack(2, 2, 0), lay.pack(3, 1, 1), lay.pack(7, 1, 0)]
    assert a.cause.tolist() == [0, lay.pack(1, 1, 0), 0, 1]
    assert a.cause_is_id.tolist() == [0, 1, 2, 0] and a.kind.tolist() == [0, 2, 0, 1]
    # a cut id of a site with no node is ranked and widens the layout
    x = (40, "ccccccccccccc", 0)
    c = pack.pack_maps(docs, extra_ids=[[x], [], []], min_site_bits=1)
    assert c.ranks[0] == {"0": 0, s1: 1, s2: 2, x[1]: 3} and c.layout.ts_bits == 6
    assert pack.pack_maps([[]], min_site_bits=1).layout.site_bits == 1
