"""The CPU model of weft (tests/weft_model.py) against the restatement R.weft,
and the conditions on the inputs of tests/test_gpu_weft.py -- no GPU.

The GPU file compares cw_weft_lists with the model array for array; these
tests make the model something independent to compare with: the host mirror
fed with the model's arrays reproduces R.weft, and on the kept documents of
every GPU input the literal and the general fold of the oracle agree with no
CW_STATUS_DUP, so no document's output is unspecified.
"""
import numpy as np
import pytest

import oracle
from cause_amd import abi, causal
from tests import weft_model as M


class ModelWeaver:
    """Stands in for abi.Weaver: weft_lists answers with the model's arrays."""

    calls = 0

    def weft_lists(self, offsets, id_key, cause_key, kind, layout, cut, yarns=True):
        self.calls += 1
        e = M.weft_expected(offsets, id_key, cause_key, kind, layout, cut)
        w = abi.ListResult(e.weave_perm, e.visible_bits, e.visible_count, e.max_ts, e.status,
                           e.yarn_perm if yarns else None)
        return abi.MergeResult(e.offsets, e.src, w)


def test_mirror_through_the_model(monkeypatch):
    """causal.weft_lists over the model's arrays == R.weft, all items in ONE
    batch call (site ranks differ per document)."""
    stand_in = ModelWeaver()
    monkeypatch.setattr(causal, "weaver", lambda: stand_in)
    items = M.mirror_items(seed=21)
    cts = []
    for ref, ids, _ in items:
        ct = causal.new_list_ct(site_id=ref["site_id"], uuid=ref["uuid"])
        ct["nodes"] = dict(ref["nodes"])
        cts.append((ct, ids))
    got = causal.weft_lists(cts)
    assert stand_in.calls == 1
    checked, gibberish, bogus = M.check_mirror(items, got)
    assert checked > 60 and gibberish > 5 and bogus > 5, (checked, gibberish, bogus)


def test_select_by_hand():
    """The three documents of test_weft_status_bits, every array spelled out."""
    from cause_amd import pack
    from oracle import causal_ref as R

    s1, s2 = "aaaaaaaaaaaaa", "bbbbbbbbbbbbb"
    doc = [R.ROOT_NODE, ((1, s1, 0), R.ROOT_ID, "x"), ((2, s2, 0), (1, s1, 0), "y")]
    b = pack.pack_lists([doc, doc, doc, []], min_site_bits=2)
    lay, S = b.layout, 4
    rk = b.docs[0].site_rank
    cut = np.zeros(4 * S, np.uint64)
    cut[0 * S + rk[s1]] = lay.pack(1, rk[s1], 0)
    cut[1 * S + rk[s1]] = lay.pack(5, rk[s1], 0)          # no node with that id
    cut[2 * S + rk[s2]] = lay.pack(2, rk[s2], 0)          # b2 without its cause
    e = M.weft_expected(b.offsets, b.id_key, b.cause_key, b.kind, lay, cut)
    assert list(e.offsets) == [0, 2, 5, 7, 7]
    assert list(e.src) == [0, 1, 0, 1, M.NO_SRC, 0, 2]
    assert list(e.kept[0][2:5]) == [b.id_key[0], b.id_key[1], lay.pack(5, rk[s1], 0)]
    assert e.kept[1][4] == pack.NIL and e.kept[2][4] == 0
    assert e.status[0] == 0
    assert e.status[1] & abi.STATUS_WEFT and e.status[1] == e.oracle_status[1] | abi.STATUS_WEFT
    assert e.status[2] == abi.STATUS_ORPHAN
    assert e.status[3] == abi.STATUS_ROOT
    assert list(e.max_ts) == [1, 5, 2, 0]
    assert list(e.visible_count) == [1, int(e.visible[2:5].sum()), int(e.visible[5:7].sum()), 0]
    assert len(e.visible_bits) == 1
    assert int(e.visible_bits[0]) == sum(int(v) << i for i, v in enumerate(e.visible))


def test_select_refuses_a_cut_word_of_another_site():
    off, idk, ck, kd, lay, cut = M.case_small()
    cut = cut.copy()
    cut[2] = lay.pack(3, 5, 0)  # rank 2's word holds an id of rank 5
    with pytest.raises(ValueError):
        M.weft_select(off, idk, ck, kd, lay, cut)


@pytest.mark.parametrize("name", [n for n in M.CASES if n not in M.GIANT_CASES])
def test_literal_equals_general_on_gpu_inputs(name):
    _literal_equals_general(name)


@pytest.mark.slow
@pytest.mark.parametrize("name", M.GIANT_CASES)
def test_literal_equals_general_on_giant_gpu_inputs(name):
    _literal_equals_general(name)


def _literal_equals_general(name):
    args = M.CASES[name]()
    lit = M.expected(name)
    gen = M.weft_expected(*args, method=oracle.METHOD_GENERAL)
    assert not (lit.oracle_status & abi.STATUS_DUP).any(), lit.oracle_status
    for f in ("offsets", "src", "weave_perm", "visible", "visible_bits", "visible_count",
              "max_ts", "status", "yarn_perm", "oracle_status"):
        assert np.array_equal(getattr(lit, f), getattr(gen, f)), (name, f)


def test_inputs_reach_the_edges_they_are_for():
    """The shapes the GPU cases rely on, asserted on the reference side."""
    sizes = lambda e: np.diff(e.offsets.astype(np.int64))
    # tiles: every boundary size is there, D >= 40, and all four status classes
    off = M.case_tiles()[0]
    n = np.diff(off.astype(np.int64))
    assert len(n) >= 40 and set(M.TILE_SIZES) <= set(n.tolist())
    M.assert_status_classes(M.expected("tiles"), M.case_tiles())
    M.assert_status_classes(M.expected("bits10"), M.case_bits10())
    # kept size == the capacity N + (D << site_bits), D = 1
    a = M.case_all_ranks_absent()
    assert a[4].site_bits == 10 and int(M.expected("all_ranks_absent").offsets[-1]) == 5001 + 1024
    assert M.case_bits1()[4].site_bits == 1 and M.case_tiles()[4].site_bits == 4
    a = M.case_upper_words()
    assert not a[5].reshape(-1, 1024)[:, :32].any() and a[5].reshape(-1, 1024)[:, 32:].any(axis=1).all()
    # beyond the fused kernel: kept sizes on both sides of 65,536, orphans in the third
    whole, closed, gib = (M.expected(k) for k in ("giant_whole", "giant_closed", "giant_gibberish"))
    assert sizes(whole)[0] == M.GIANT_N and whole.status[0] == 0
    assert sizes(closed)[0] < 65536 and closed.status[0] == 0
    assert sizes(gib)[0] > 65535 and gib.status[0] == abi.STATUS_ORPHAN
    assert list(sizes(M.expected("giant_batch"))) == [sizes(whole)[0], sizes(closed)[0], sizes(gib)[0]]
