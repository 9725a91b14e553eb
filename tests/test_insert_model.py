"""tests/insert_model.py (the statement of cw_insert_lists) against
oracle.causal_ref.insert(list_weave, ...), step by step (CPU only).

Every step of every history compares the whole result -- weave, hide? flags,
yarns, lamport-ts -- with the reference's; a refusal of the model (DUP, ORPHAN)
must be a throw of the reference with the matching :causes, and the skipped
re-insert must return the ct unchanged.
"""
import json
import os
import random

import numpy as np
import pytest

from oracle import causal_ref as R
from tests import insert_model as M
from tests import refgen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_tx(ct, rng, sites, lamport, k, run=False):
    """A tx of k nodes: the first under a random node, the others chained to it.
    lamport = False: the ts may lie below the cause's (a non-Lamport id).
    run = True: a tx of several nodes holds plain values only (a typed run)."""
    for _ in range(100):
        site = rng.choice(sites)
        cause = rng.choice(list(ct["nodes"]))
        yarn = ct["yarns"].get(site)
        top = max(i[0] for i in ct["nodes"])
        ts = 1 + max(cause[0], yarn[-1][0][0] if yarn else 0) if lamport else rng.randint(1, top + 1)
        if not any(i[0] == ts and i[1] == site for i in ct["nodes"]):
            break
    else:
        raise AssertionError("no free id")
    values = "abcdefg " if run and k > 1 else G.SIMPLE_VALUES + [R.H_SHOW]
    tx = [((ts, site, 0), cause, rng.choice(values))]
    for m in range(1, k):
        tx.append(((ts, site, m), tx[-1][0], rng.choice(values)))
    return tx


def check_step(ct, tx, in_domain=False):
    """One insert through the model and through the reference; returns the new ct."""
    b = M.batch_of([(ct, tx)])
    res = M.run(b)
    st = int(res.status[0])
    if st:
        with pytest.raises(R.CauseError) as e:
            R.insert(R.list_weave, ct, tx[0], tx[1:])
        want = "edits-not-allowed" if st == M.STATUS_DUP else "cause-must-exist"
        assert want in e.value.causes and st in (M.STATUS_DUP, M.STATUS_ORPHAN)
        new = ct
    else:
        new = R.insert(R.list_weave, ct, tx[0], tx[1:])
    weave, vis, yarns, max_ts = M.doc_view(b, res, 0)
    w = new["weave"]
    assert weave == w
    assert vis == [not R.hide_q(n, w[j + 1] if j + 1 < len(w) else None) for j, n in enumerate(w)]
    assert int(res.visible_count[0]) == sum(vis)
    assert yarns == new["yarns"]
    assert max_ts == R.refresh_ts(new)["lamport_ts"]
    grew = len(w) - len(ct["weave"])
    assert int(res.new_offsets[1]) == len(w) and grew in (0, len(tx))
    if grew:
        p = int(res.insert_pos[0])
        assert w[p:p + len(tx)] == tx and not st
    else:
        assert int(res.insert_pos[0]) == M.NONE
    if in_domain and not st:
        assert R.list_weave(new)["weave"] == w
    return new


@pytest.mark.parametrize("seed", range(8))
def test_random_histories_match_the_reference_step_by_step(seed):
    rng = random.Random(1000 + seed)
    for _ in range(12):
        sites = [R.new_site_id(rng) for _ in range(5)]
        ct = R.new_list_ct(rng=rng)
        for _ in range(rng.randint(5, 40)):
            tx = rand_tx(ct, rng, sites, rng.random() >= 0.3, rng.choice([1, 1, 3]))
            ct = check_step(ct, tx)
            r = rng.random()
            if r < 0.08:    # the same node again: skipped, the whole tx with it
                again = rng.choice(list(ct["nodes"].items()))
                (ts, site, x), body = again
                check_step(ct, [(again[0],) + body, ((ts, site, x + 50), again[0], "y")])
            elif r < 0.16:  # an id of the tree with another body
                i, body = rng.choice(list(ct["nodes"].items()))
                other = [(i, body[0], "?"), (i, R.ROOT_ID if body[0] != R.ROOT_ID else i, body[1])]
                check_step(ct, [rng.choice(other)])
            elif r < 0.24:  # a cause that is no node, a nil cause
                tx = rand_tx(ct, rng, sites, True, 1)
                check_step(ct, [(tx[0][0], rng.choice([(99, sites[0], 7), None]), "x")])


@pytest.mark.parametrize("seed", range(4))
def test_in_domain_histories_equal_the_full_reweave(seed):
    """Lamport histories of single nodes (any value) and typed runs.  (A tx whose
    later nodes hang under a special node of the same tx is outside: s/insert
    splices the tx as one block, the fold would defer the plain nodes behind the
    special one's other children -- the random histories above hold the model to
    the block splice there.)"""
    rng = random.Random(2000 + seed)
    for _ in range(10):
        sites = [R.new_site_id(rng) for _ in range(5)]
        ct = R.new_list_ct(rng=rng)
        for _ in range(rng.randint(5, 40)):
            ct = check_step(ct, rand_tx(ct, rng, sites, True, rng.choice([1, 3]), run=True), in_domain=True)


def golden_cases():
    j = json.load(open(os.path.join(ROOT, "tests", "golden", "edge_cases.json")))
    val = lambda v: R.Keyword(*v["kw"].split("/")) if isinstance(v, dict) else v
    return [[(tuple(i), tuple(c), val(v)) for i, c, v in case["nodes"]] for case in j["cases"]]


def test_the_nine_edge_cases_built_by_successive_inserts():
    cases = golden_cases()
    assert len(cases) == 9
    for nodes in cases:
        ct = R.new_list_ct(rng=random.Random(0))
        for nd in nodes:
            ct = check_step(ct, [nd])
        assert len(ct["weave"]) == len(nodes) + 1
        # (the edge cases are idempotent-insert cases: again, in any order, nothing moves)
        for nd in reversed(nodes):
            assert check_step(ct, [nd]) is ct


def test_place_is_weave_node_on_out_of_domain_weaves():
    """Weaves that hold orphans and non-Lamport causes (any permutation of a
    node set is a weave weave-node may be handed): the formula is the loop."""
    rng = random.Random(7)
    for _ in range(300):
        sites = [R.new_site_id(rng) for _ in range(3)]
        ids = {(rng.randint(1, 9), rng.choice(sites), 0) for _ in range(rng.randint(1, 12))}
        pool = sorted(ids, key=R.id_key) + [(77, sites[0], 0)]
        nodes = [R.ROOT_NODE] + [(i, rng.choice(pool + [R.ROOT_ID]), rng.choice(G.SIMPLE_VALUES))
                                 for i in ids]
        rng.shuffle(nodes)
        ct = dict(R.new_list_ct(rng=rng), nodes={n[0]: (n[1], n[2]) for n in nodes}, weave=nodes)
        ct = R.spin(dict(ct, yarns={}))
        nm = ((rng.randint(1, 10), rng.choice(sites), 1), rng.choice(nodes)[0],
              rng.choice(G.SIMPLE_VALUES))
        b = M.batch_of([(ct, [nm])])
        res = M.run(b)
        assert int(res.status[0]) == 0
        assert M.doc_view(b, res, 0)[0] == R.weave_node(nodes, nm)


def orphaned_ct(rng, sites, nodes):
    """A ct whose weave is `nodes` as they stand (orphans included)."""
    ct = dict(R.new_list_ct(rng=rng), nodes={n[0]: (n[1], n[2]) for n in nodes}, weave=list(nodes))
    return R.spin(dict(ct, yarns={}))


def test_a_missing_cause_is_refused_though_an_orphan_names_the_tx_id():
    """An orphan of the document whose cause is the tx node's id gives the tx an
    asap position (id(nm) = cause(weave[i])), yet s/insert looks for the tx
    node's own cause among the nodes first (shared.cljc:175-178)."""
    rng = random.Random(9)
    s = R.new_site_id(rng)
    q = (5, s, 0)
    ct = orphaned_ct(rng, [s], [R.ROOT_NODE, ((1, s, 0), R.ROOT_ID, "a"), ((6, s, 0), q, "b")])
    b = M.batch_of([(ct, [(q, (77, s, 0), "x")])])
    res = M.run(b)
    assert int(res.status[0]) == M.STATUS_ORPHAN and int(res.insert_pos[0]) == M.NONE
    assert check_step(ct, [(q, (77, s, 0), "x")]) is ct
    # ... and under a cause that is a node it is accepted (the younger orphan stays ahead: later)
    new = check_step(ct, [(q, (1, s, 0), "x")])
    assert [n[0] for n in new["weave"]] == [R.ROOT_ID, (1, s, 0), (6, s, 0), q]
    # random weaves with orphans of (77, site, 0): that id under a present and under a missing cause
    for _ in range(200):
        sites = [R.new_site_id(rng) for _ in range(3)]
        ids = {(rng.randint(1, 9), rng.choice(sites), 0) for _ in range(rng.randint(1, 12))}
        missing = (77, sites[0], 0)
        pool = sorted(ids, key=R.id_key) + [missing, missing]
        nodes = [R.ROOT_NODE] + [(i, rng.choice(pool + [R.ROOT_ID]), rng.choice(G.SIMPLE_VALUES)) for i in ids]
        rng.shuffle(nodes)
        ct = orphaned_ct(rng, sites, nodes)
        gone = rng.random() < 0.5
        nm = (missing, (88, sites[1], 0) if gone else rng.choice(nodes)[0], rng.choice(G.SIMPLE_VALUES))
        b = M.batch_of([(ct, [nm])])
        assert int(M.run(b).status[0]) == (M.STATUS_ORPHAN if gone else 0)
        check_step(ct, [nm])


def test_offsets_compact_over_refused_and_empty_documents():
    rng = random.Random(3)
    sites = [R.new_site_id(rng) for _ in range(3)]
    cts, txs = [], []
    for d in range(12):
        ct = R.new_list_ct(rng=rng)
        for _ in range(rng.randint(0, 9)):
            tx = rand_tx(ct, rng, sites, True, 1)
            ct = R.insert(R.list_weave, ct, tx[0])
        tx = rand_tx(ct, rng, sites, True, 1 + d % 3)
        if d % 4 == 1:
            tx = []
        if d % 4 == 2:
            tx = [(tx[0][0], (50, sites[0], 0), "x")]
        cts.append(ct), txs.append(tx)
    b = M.batch_of(list(zip(cts, txs)))
    res = M.run(b)
    grow = [len(t) if d % 4 in (0, 3) else 0 for d, t in enumerate(txs)]
    assert np.array_equal(np.diff(res.new_offsets.astype(np.int64)),
                          [len(c["weave"]) + g for c, g in zip(cts, grow)])
    assert [int(s) for s in res.status] == [M.STATUS_ORPHAN if d % 4 == 2 else 0 for d in range(12)]
    for d, (ct, tx) in enumerate(zip(cts, txs)):
        want = R.insert(R.list_weave, ct, tx[0], tx[1:]) if grow[d] else ct
        assert M.doc_view(b, res, d)[0] == want["weave"]
        assert len(res.id_key) == int(res.new_offsets[-1])
