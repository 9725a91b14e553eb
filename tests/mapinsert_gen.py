"""Generators of map transactions for the cw_insert_maps tests (CPU and GPU).

* ``rand_tx`` -- a tx of k nodes over every kind of cause: keys, ids of the
  collection, the root id, absent ids, nil, earlier and later nodes of the
  same tx; specials; Lamport or out-of-order ids.
* ``base_tx`` -- CausalBase-shaped txs: assoc (a key-caused value), dissoc (a
  key-caused hide) and undo / redo (an h.hide or h.show under a key-caused
  value node).  Every id cause names a key-caused node, so s/insert equals the
  full reweave.
* ``gen_coll`` / ``gen_tx`` -- collections and txs as columns, rows of (id,
  cause, cause_is_id, kind) with ids ts << 12 | site << 8 | tx and small
  integers as key tokens: what the GPU tests feed the library.  ``wild=False``
  is the generator of the GPU "equals the full reweave" comparison;
  ``ref_nodes`` turns its rows into reference nodes, so that the CPU tests can
  hold it against the reference.
"""
from __future__ import annotations

from oracle import causal_ref as R

KEYS = ["k0", "k1", "k2", "k3", "k4", "k5"]
VALUES = ["a", "b", "c", "d", 1, 2, R.HIDE, R.H_HIDE, R.H_SHOW]


def free_id(ct, rng, sites, lamport=True):
    """(ts, site) of a tx that is not in the collection."""
    top = max([i[0] for i in ct["nodes"]] + [ct["lamport_ts"], 0])
    for _ in range(200):
        site = rng.choice(sites)
        ts = top + 1 if lamport else rng.randint(1, top + 1)
        if not any(i[0] == ts and i[1] == site for i in ct["nodes"]):
            return ts, site
    raise AssertionError("no free id")


def rand_tx(ct, rng, sites, k, lamport=True, first_ok=True):
    ts, site = free_id(ct, rng, sites, lamport)
    ids = [(ts, site, m) for m in range(k)]
    old = list(ct["nodes"])
    tx = []
    for m in range(k):
        r = rng.random()
        if r < 0.40 or (m == 0 and first_ok and not old):
            cause = rng.choice(KEYS)
        elif r < 0.70 and old:
            cause = rng.choice(old)
        elif r < 0.78 and not (m == 0 and first_ok):
            cause = R.ROOT_ID
        elif r < 0.84 and not (m == 0 and first_ok):
            cause = (ts + 7, sites[0], 9)       # an absent id
        elif r < 0.90 and not (m == 0 and first_ok):
            cause = None
        elif m > 0 and r < 0.96:
            cause = ids[rng.randrange(m)]       # an earlier node of the tx
        elif m > 0 and m + 1 < k:
            cause = ids[rng.randrange(m + 1, k)]  # a later one
        else:
            cause = rng.choice(KEYS)
        tx.append((ids[m], cause, rng.choice(VALUES)))
    return tx


def base_tx(ct, rng, sites, k):
    ts, site = free_id(ct, rng, sites)
    values = [i for i, b in ct["nodes"].items() if not R.valid_id(b[0]) and not R.is_special(b[1])]
    tx = []
    for m in range(k):
        r = rng.random()
        if r < 0.55 or not values:
            tx.append(((ts, site, m), rng.choice(KEYS), rng.choice("abcdef")))
        elif r < 0.70:
            tx.append(((ts, site, m), rng.choice(KEYS), R.HIDE))
        else:
            tx.append(((ts, site, m), rng.choice(values), rng.choice([R.H_HIDE, R.H_SHOW])))
    return tx


def history(rng, steps, sites, gen=base_tx, ks=(1, 1, 2, 3)):
    """A map ct grown by `steps` txs through the reference's insert."""
    ct = R.new_map_ct(rng=rng)
    for _ in range(steps):
        tx = gen(ct, rng, sites, rng.choice(ks))
        try:
            ct = R.insert(R.map_weave, ct, tx[0], tx[1:])
        except R.CauseError:
            pass
    return ct


# ------------------------------------------------------------- as columns
NORMAL, HIDE, HHIDE, HSHOW = 0, 1, 2, 3
KINDS = [NORMAL] * 6 + [HIDE, HHIDE, HSHOW]


def key(ts, site, tx=0):
    return ts << 12 | site << 8 | tx


def gen_coll(rng, n, keys=12, hot=0.0, wild=True):
    """n nodes in id order: (id, cause, cause_is_id, kind) rows.  wild: id causes
    may name id-caused nodes, the root id, absent ids; nil causes."""
    rows, plain = [], []
    for s in range(n):
        i = key(s + 1, rng.randrange(4))
        r = rng.random()
        if r < 0.6 or not rows:
            tok = 2 * rng.randrange(keys) + 1 if rng.random() >= hot else 1
            row = (i, tok, 0, rng.choice(KINDS[:7]))
            if row[3] == NORMAL:
                plain.append(i)
        elif r < 0.85 and plain:
            row = (i, rng.choice(plain), 1, rng.choice([HHIDE, HSHOW, NORMAL]))
        elif not wild:
            row = (i, 2 * rng.randrange(keys) + 1, 0, NORMAL)
            plain.append(i)
        elif r < 0.94:
            row = (i, rng.choice(rows)[0], 1, rng.choice(KINDS))
        elif r < 0.97:
            row = (i, 0, 2, rng.choice(KINDS))
        else:
            row = (i, rng.choice([0, key(9999, 5)]), 1, rng.choice(KINDS))
        rows.append(row)
    return rows


def gen_tx(rng, rows, k, ts, keys=12, wild=True):
    """k tx rows over every kind of cause; the first one is acceptable."""
    ids = [key(ts, 7, m) for m in range(k)]
    plain = [r[0] for r in rows if r[2] == 0 and r[3] == NORMAL]
    tx = []
    for m in range(k):
        r = rng.random()
        if r < 0.45 or not rows:
            row = (ids[m], rng.randrange(2 * keys + 2), 0, rng.choice(KINDS))  # even tokens: new key weaves
        elif r < 0.70 and plain:
            row = (ids[m], rng.choice(plain), 1, rng.choice([HHIDE, HSHOW, NORMAL]))
        elif not wild:
            row = (ids[m], rng.randrange(2 * keys + 2), 0, NORMAL)
        elif r < 0.80:
            row = (ids[m], rng.choice(rows)[0], 1, rng.choice(KINDS))
        elif m and r < 0.88:
            row = (ids[m], ids[rng.randrange(m)], 1, rng.choice(KINDS))
        elif m and m + 1 < k and r < 0.93:
            row = (ids[m], ids[rng.randrange(m + 1, k)], 1, rng.choice(KINDS))
        elif m and r < 0.96:
            row = (ids[m], rng.choice([0, key(9999, 5)]), 1, rng.choice(KINDS))
        elif m:
            row = (ids[m], 0, 2, rng.choice(KINDS))
        else:
            row = (ids[m], rng.randrange(2 * keys + 2), 0, rng.choice(KINDS))
        tx.append(row)
    return tx


def ref_nodes(rows):
    """Rows of gen_coll / gen_tx as reference nodes (id, cause, value): site s is
    the 13-character site id "s00000000000s" (the sites sort as their numbers),
    token t the key "t", the kinds the special keywords or a plain value."""
    ident = lambda w: R.ROOT_ID if w == 0 else (w >> 12, "s%012d" % ((w >> 8) & 15), w & 255)
    value = {NORMAL: "v", HIDE: R.HIDE, HHIDE: R.H_HIDE, HSHOW: R.H_SHOW}
    return [(ident(i), ident(c) if ci == 1 else None if ci == 2 else "t%d" % c, value[kd])
            for i, c, ci, kd in rows]
