"""tests/invert_model.py (no GPU): the tuple form against the reference's known
answers (tests/golden/invert_cases.json), the columns form against the tuple
form on seeded bases, the array-map order at 8 and 9 parts, and the dedup cases
of include/causeweave_invert.h."""
import json
import os
import random

import pytest

from cause_amd import causal as C, pack
from tests import invert_gen as G
from tests import invert_model as M

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "invert_cases.json")))
S, T = "QeVBlHoQFZSx0", "ZZremoteSite1"
KW = {":causal/hide": C.HIDE, ":causal/h.hide": C.H_HIDE, ":causal/h.show": C.H_SHOW}


def both(base, sl, new_tx, **kw):
    """The tx of one base by the tuple form and by the columns form, as nodes."""
    colls = G.collections_of(base)
    want = M.transact_parts(M.invert_tx(colls, M.slice_of(colls, *sl)), *new_tx)
    pk = M.pack_bases([base], [sl], [new_tx], **{"tx_bits": G.TX_BITS, **kw})
    parts = M.invert_columns(*pk.args())
    return want, M.unpack_parts(pk, parts)[0], pk, parts


def test_invert_path_is_the_references():
    g = GOLDEN["invert_path"]
    node = (tuple(g["node"][0]), g["node"][1], g["node"][2])
    u, cause, value = M.invert_path(g["uuid"], node)
    assert [u, list(cause), repr(value)] == g["expect"]
    assert M.invert_path("u", ((2, S, 0), "a", C.HIDE)) == ("u", "a", C.H_SHOW)
    assert M.invert_path("u", ((2, S, 0), (1, S, 0), C.H_HIDE)) == ("u", (1, S, 0), C.H_SHOW)
    assert M.invert_path("u", ((2, S, 0), (1, S, 0), C.H_SHOW)) == ("u", (1, S, 0), C.H_HIDE)


def test_invert_of_the_whole_history_8_entries_become_13():
    """test-invert-: {:a 1 :b 2}, :a 3, :c [1 2 3], :c hide; the list's three
    nodes are nested in a collection about to be hidden and make no parts."""
    g = GOLDEN["invert"]
    root = [((1, S, 0), "a", 1), ((1, S, 1), "b", 2), ((2, S, 0), "a", 3), ((3, S, 3), "c", M.ref("L")),
            ((4, S, 0), "c", C.HIDE)]
    lst = [C.ROOT_NODE, ((3, S, 0), C.ROOT_ID, 1), ((3, S, 1), (3, S, 0), 2), ((3, S, 2), (3, S, 1), 3)]
    base = [("R", "map", root), ("L", "list", lst)]
    assert len(G.all_ids(base)) == g["history_before"]
    want, got, _, parts = both(base, (None, None, None), (5, S))
    assert want == got and len(G.all_ids(base)) + len(want) == g["history_after"]
    assert [n for _, n in want] == [((5, S, 0), "c", C.H_SHOW), ((5, S, 1), (3, S, 3), C.H_HIDE),
                                    ((5, S, 2), (2, S, 0), C.H_HIDE), ((5, S, 3), (1, S, 1), C.H_HIDE),
                                    ((5, S, 4), (1, S, 0), C.H_HIDE)]
    assert {u for u, _ in want} == {"R"} and parts.base_parts.tolist() == [5]


@pytest.mark.parametrize("seed", range(6))
def test_columns_form_equals_tuple_form(seed):
    rng = random.Random(seed)
    bases, slices, new_tx = G.gen_batch(rng, 20, max_nodes=60)
    pk = M.pack_bases(bases, slices, new_tx, tx_bits=G.TX_BITS)
    parts = M.invert_columns(*pk.args())
    got = M.unpack_parts(pk, parts)
    assert not parts.status.any()
    total = 0
    for g, base in enumerate(bases):
        colls = G.collections_of(base)
        want = M.transact_parts(M.invert_tx(colls, M.slice_of(colls, *slices[g])), *new_tx[g])
        assert got[g] == want, (seed, g)
        assert int(parts.base_parts[g]) == len(want)
        total += len(want)
    assert total == int(parts.part_offsets[-1]) and (seed != 0 or total > 50)


@pytest.mark.parametrize("n", [8, 9])
def test_array_map_order(n):
    """n keys over two maps, each dissoc'ed twice: the older dissocs ascend with
    k, the newer ones descend.  The tx order is each key's first appearance
    newest first = descending id of its newest node (k ascending); the part's
    source is the older dissoc.  8 keys: the reference's array map; 9: the same
    rule, the library's choice."""
    colls = {"A": [], "B": []}
    for k in range(n):
        colls["AB"[k % 2]] += [((1 + k, S, 0), f"k{k}", C.HIDE), ((40 - k, T, 0), f"k{k}", C.HIDE)]
    base = [("A", "map", colls["A"]), ("B", "map", colls["B"])]
    want, got, _, parts = both(base, (None, None, None), (60, S))
    assert want == got == [("AB"[k % 2], ((60, S, k), f"k{k}", C.H_SHOW)) for k in range(n)]
    assert parts.inv_src.tolist() == [2 * j for j in range((n + 1) // 2)] + [2 * j for j in range(n // 2)]
    assert parts.base_parts.tolist() == [n]


def test_a_value_node_and_its_hide():
    """[id c v] and [id2 id :causal/hide] share the key [u id]: the part comes
    from the older one, the value node: h.hide, ordered by the hide's id."""
    base = [("L", "list", [C.ROOT_NODE, ((1, S, 0), C.ROOT_ID, "x"), ((2, S, 0), (1, S, 0), C.HIDE),
                           ((3, S, 0), C.ROOT_ID, "y")])]
    want, got, _, parts = both(base, (None, None, None), (4, S), lists_only=True)
    assert want == got == [("L", ((4, S, 0), (3, S, 0), C.H_HIDE)), ("L", ((4, S, 1), (1, S, 0), C.H_HIDE))]
    assert parts.inv_src.tolist() == [3, 1] and parts.inv_cause_is_id is None


def test_hide_show_chains_under_one_cause():
    v = (1, S, 0)
    chain = [((2, S, 0), v, C.H_HIDE), ((3, S, 0), v, C.H_SHOW), ((4, S, 0), v, C.H_HIDE)]
    base = [("M", "map", [(v, "a", 1)] + chain)]
    want, got, _, parts = both(base, ((2, S, 0), (4, S, 0), None), (5, S))
    assert want == got == [("M", ((5, S, 0), v, C.H_SHOW))] and parts.inv_src.tolist() == [1]
    want, got, _, parts = both(base, ((3, S, 0), (4, S, 0), None), (5, S))
    assert want == got == [("M", ((5, S, 0), v, C.H_HIDE))] and parts.inv_src.tolist() == [2]
    want, got, _, _ = both(base, (None, None, None), (5, S))
    assert want == got == [("M", ((5, S, 0), v, C.H_HIDE))]   # from the value node itself


def test_token_and_id_with_the_same_word_are_two_keys():
    """A dissoc of the key with token 0 ... and an id cause that packs to the same word."""
    base = [("M", "map", [((1, S, 0), "a", 1), ((2, S, 0), "a", C.HIDE), ((3, S, 0), (1, S, 0), C.H_HIDE)])]
    pk = M.pack_bases([base], [((2, S, 0), (3, S, 0), None)], [(4, S)])
    word = int(pk.id_key[0])
    pk.cause[1] = word                        # the token of "a" made equal to the id's word
    pk.tokens = {word: "a"}
    assert pk.cause_is_id.tolist() == [0, 0, 1] and int(pk.cause[2]) == word
    parts = M.invert_columns(*pk.args())
    assert parts.inv_cause.tolist() == [word, word] and parts.inv_cause_is_id.tolist() == [1, 0]
    assert parts.inv_kind.tolist() == [pack.KIND_HSHOW, pack.KIND_HSHOW] and parts.inv_src.tolist() == [2, 1]
    colls = G.collections_of(base)
    want = M.transact_parts(M.invert_tx(colls, M.slice_of(colls, (2, S, 0), (3, S, 0), None)), 4, S)
    assert M.unpack_parts(pk, parts)[0] == want


def test_the_nil_key():
    base = [("M", "map", [((1, S, 0), None, 1), ((2, S, 0), None, C.HIDE), ((3, S, 0), None, C.HIDE)])]
    want, got, pk, parts = both(base, ((2, S, 0), (3, S, 0), None), (4, S))
    assert want == got == [("M", ((4, S, 0), None, C.H_SHOW))]
    pk.cause[1:] = [7, 9]                      # the cause word of a nil key is ignored
    again = M.invert_columns(*pk.args())
    M.same(parts, again)
    assert again.inv_cause.tolist() == [0] and again.inv_cause_is_id.tolist() == [2]


def test_key_range_status_and_no_parts():
    nodes = [((1 + k, S, 0), f"k{k}", k) for k in range(9)]
    small = [("N", "map", [((1, S, 0), "a", 1)])]
    pk = M.pack_bases([small, [("M", "map", nodes), ("E", "list", [C.ROOT_NODE])], small],
                      [(None, None, None)] * 3, [(12, S)] * 3, tx_bits=3)
    parts = M.invert_columns(*pk.args())
    assert parts.status.tolist() == [0, M.STATUS_KEY_RANGE, M.STATUS_KEY_RANGE, 0]
    assert parts.base_parts.tolist() == [1, 0, 1] and parts.part_offsets.tolist() == [0, 1, 1, 1, 2]
