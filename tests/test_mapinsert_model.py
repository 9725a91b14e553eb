"""tests/mapinsert_model.py (the statement of cw_insert_maps) against
oracle.causal_ref.insert(map_weave, ...), step by step (CPU only).

Every step of every history compares the whole result -- ::nodes, every key
weave, active-node of every key -- with the reference's; a refusal of the model
(DUP, ORPHAN) must be a throw of the reference with the matching :causes, and
the skipped re-insert must return the ct unchanged.
"""
import random

import numpy as np
import pytest

from oracle import causal_ref as R
from tests import mapinsert_gen as G
from tests import mapinsert_model as M


def check_step(ct, tx, reweave=False):
    """One insert through the model and through the reference; returns the new ct."""
    b = M.batch_of([(ct, tx)])
    res = M.run(b)
    st = int(res.status[0])
    if st:
        with pytest.raises(R.CauseError) as e:
            R.insert(R.map_weave, ct, tx[0], tx[1:])
        want = "edits-not-allowed" if st == M.STATUS_DUP else "cause-must-exist"
        assert want in e.value.causes and st in (M.STATUS_DUP, M.STATUS_ORPHAN)
        new = ct
    else:
        new = R.insert(R.map_weave, ct, tx[0], tx[1:])
    nodes, weave, act = M.doc_view(b, res, 0)
    assert nodes == new["nodes"]
    assert weave == new["weave"]
    assert act == {k: R.active_node(k, w) for k, w in new["weave"].items()}
    grew = len(new["nodes"]) - len(ct["nodes"])
    assert int(res.new_offsets[1]) == len(new["nodes"]) and grew in (0, len(tx))
    for j, nd in enumerate(tx):
        if grew:
            s, p = int(res.tx_seg[j]), int(res.tx_pos[j])
            kw = weave[M.key_of(b, 0, int(res.seg_key[s]))]
            assert kw[p][0] == nd[0]
        else:
            assert int(res.tx_seg[j]) == M.NONE and int(res.tx_pos[j]) == M.NONE
    if reweave and not st:
        assert R.map_weave(new)["weave"] == new["weave"]
    return new


@pytest.mark.parametrize("seed", range(8))
def test_random_histories_match_the_reference_step_by_step(seed):
    rng = random.Random(3000 + seed)
    steps = 0
    for _ in range(10):
        sites = [R.new_site_id(rng) for _ in range(4)]
        ct = R.new_map_ct(rng=rng)
        for _ in range(rng.randint(5, 30)):
            tx = G.rand_tx(ct, rng, sites, rng.randint(1, 4), lamport=rng.random() >= 0.3,
                           first_ok=rng.random() >= 0.15)
            ct = check_step(ct, tx)
            steps += 1
            r = rng.random()
            if r < 0.08 and ct["nodes"]:    # the same node again: skipped, the whole tx with it
                i, body = rng.choice(list(ct["nodes"].items()))
                check_step(ct, [(i,) + body, ((i[0], i[1], i[2] + 50), "k0", "y")])
            elif r < 0.16 and ct["nodes"]:  # an id of the collection with another body
                i, body = rng.choice(list(ct["nodes"].items()))
                check_step(ct, [rng.choice([(i, body[0], "?"), (i, "other", body[1])])])
            elif r < 0.24:  # a first node caused by its own tx
                ts, site = G.free_id(ct, rng, sites)
                check_step(ct, [((ts, site, 0), (ts, site, 1), "x"), ((ts, site, 1), "k1", "y")])
    assert steps > 50


def test_the_refusals():
    rng = random.Random(7)
    sites = [R.new_site_id(rng) for _ in range(2)]
    ct = G.history(rng, 12, sites)
    ts, site = G.free_id(ct, rng, sites)
    for cause in [(ts + 3, site, 0), R.ROOT_ID, None]:
        b = M.batch_of([(ct, [((ts, site, 0), cause, "v")])])
        assert int(M.run(b).status[0]) == M.STATUS_ORPHAN
        check_step(ct, [((ts, site, 0), cause, "v")])
    # an empty collection takes a key cause and refuses the others
    empty = R.new_map_ct(rng=rng)
    check_step(empty, [((1, site, 0), (1, site, 1), "v"), ((1, site, 1), "k0", "w")])
    new = check_step(empty, [((1, site, 0), "k0", "v")])
    assert R.map_get(new, "k0") == "v"
    # a key token >= 2^62
    b = M.batch_of([(ct, [((ts, site, 0), "k0", "v"), ((ts, site, 1), "k1", "v")])])
    b.tca = b.tca.copy()
    b.tca[1] = np.uint64(1 << 62)
    r = M.run(b)
    assert int(r.status[0]) == M.STATUS_MAP_KEY and int(r.new_offsets[1]) == len(ct["nodes"])
    assert np.array_equal(r.seg_perm, b.seg_perm) and np.array_equal(r.seg_active, b.seg_active)


def test_assoc_after_dissoc_and_undo_shapes():
    rng = random.Random(11)
    site = R.new_site_id(rng)
    ct = R.new_map_ct(site_id=site, rng=rng)
    ct = check_step(ct, [((1, site, 0), "k", "v1")], True)
    ct = check_step(ct, [((2, site, 0), "k", R.HIDE)], True)          # dissoc
    ct = check_step(ct, [((3, site, 0), "k", "v2")], True)            # assoc after it
    ct = check_step(ct, [((4, site, 0), (3, site, 0), R.H_HIDE)], True)  # undo
    ct = check_step(ct, [((5, site, 0), (4, site, 0), R.H_SHOW)])        # redo, under the h.hide
    ct = check_step(ct, [((6, site, 0), (3, site, 0), R.H_SHOW)], True)
    # the any-hide-follows quirk: a hide of ANOTHER node behind the active node
    ct = check_step(ct, [((7, site, 0), "k", "v3"), ((7, site, 1), (1, site, 0), R.HIDE)])
    check_step(ct, [((8, site, 0), "j", R.HIDE), ((8, site, 1), "j", "w")])


@pytest.mark.parametrize("seed", range(3))
def test_the_gpu_reweave_generator_is_base_shaped(seed):
    """mapinsert_gen.gen_coll / gen_tx with wild=False feed the GPU 'equals the
    full reweave' comparison and its chain of calls.  Counted here: in every
    collection they yield, with its tx, every id cause names a key-caused node,
    so that comparison skips no collection; and for the same rows as reference
    nodes the reference's insert (and the model) equals the reference's full
    reweave, before and after the tx."""
    rng = random.Random(31 + seed)
    colls = ids = 0
    for n in (0, 3, 40, 100, 40, 3, 100, 20):
        rows = G.gen_coll(rng, n, wild=False)
        tx = G.gen_tx(rng, rows, rng.choice([1, 2, 3, 8]), 2000, wild=False)
        body = {r[0]: r for r in rows + tx}
        for i, cause, ci, kd in rows + tx:
            assert ci in (0, 1)
            if ci == 1:
                ids += 1
                assert cause in body and body[cause][2] == 0, "an id cause names no key-caused node"
        ct = R.new_map_ct(rng=rng)
        for nd in G.ref_nodes(rows):
            ct = R.insert(R.map_weave, ct, nd)
        assert R.map_weave(ct)["weave"] == ct["weave"]
        nodes = G.ref_nodes(tx)
        new = check_step(ct, nodes, True)
        assert len(new["nodes"]) == n + len(tx)
        colls += 1
    assert colls == 8 and ids > 20


@pytest.mark.parametrize("seed", range(3))
def test_base_shaped_histories_equal_the_full_reweave(seed):
    """CausalBase-shaped histories through the reference (mapinsert_gen.base_tx):
    every id cause names a key-caused node, and insert equals the full reweave."""
    rng = random.Random(4000 + seed)
    colls = ids = 0
    for _ in range(8):
        sites = [R.new_site_id(rng) for _ in range(4)]
        ct = R.new_map_ct(rng=rng)
        for _ in range(rng.randint(5, 25)):
            ct = check_step(ct, G.base_tx(ct, rng, sites, rng.randint(1, 4)), True)
        for i, (cause, _) in ct["nodes"].items():
            if R.valid_id(cause):
                ids += 1
                assert cause in ct["nodes"] and not R.valid_id(ct["nodes"][cause][0])
        colls += 1
    assert colls == 8 and ids > 0


def test_model_weave_equals_the_reference_fold():
    rng = random.Random(5)
    sites = [R.new_site_id(rng) for _ in range(3)]
    cts = [G.history(rng, n, sites) for n in (0, 1, 9, 20)]
    b = M.batch_of([(ct, []) for ct in cts])
    order = np.concatenate([int(b.off[d]) + np.argsort(b.idk[int(b.off[d]):int(b.off[d + 1])], kind="stable")
                            for d in range(len(cts))] + [np.zeros(0, np.int64)]).astype(np.int64)
    w = M.weave_maps(b.off, b.idk[order], b.ca[order], b.ci[order], b.kd[order])
    assert np.array_equal(w.seg_key, b.seg_key) and np.array_equal(w.seg_coll, b.seg_coll)
    for s in range(len(w.seg_key)):
        d, o = int(w.seg_coll[s]), int(b.off[int(w.seg_coll[s])])
        got = [int(b.idk[order[o + x]]) for x in w.seg_perm[int(w.seg_offsets[s]) + 1:int(w.seg_offsets[s + 1])]]
        want = [int(b.idk[o + x]) for x in b.seg_perm[int(b.seg_off[s]) + 1:int(b.seg_off[s + 1])]]
        assert got == want
