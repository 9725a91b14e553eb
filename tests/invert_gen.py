"""Seeded bases for the cw_invert tests: a few sites transact into the lists and
maps of a base, with dissocs, hides, h.hide / h.show under value nodes, id and
nil keys, and refs between the collections of the base.  A base is
[(uuid, "list" | "map", [node, ...]), ...] as tests/invert_model.pack_bases takes
it; ids are unique across the base."""
from __future__ import annotations

from cause_amd import causal as C
from tests import invert_model as M

TX_BITS = 10
KEYS = ["a", "b", "c", "d", "e", "f"]


def _uid(rng, n):
    return C._uid(rng, n)


def gen_base(rng, sizes, n_sites=3, ref_rate=0.03):
    """One base with a collection of sizes[k] nodes each (a list's root not counted).
    A ref names a later collection of the base, so the first one is never nested."""
    sites = [_uid(rng, 13) for _ in range(n_sites)]
    colls = []
    for k, _ in enumerate(sizes):
        typ = "list" if rng.random() < 0.5 else "map"
        colls.append((_uid(rng, 21), typ, [C.ROOT_NODE] if typ == "list" else []))
    left = list(sizes)
    vals = [[] for _ in sizes]      # each collection's value nodes
    ts = 0
    while any(left):
        ts += 1
        site = rng.choice(sites)
        for tx in range(rng.randint(1, 4)):
            open_ = [k for k, n in enumerate(left) if n]
            if not open_:
                break
            k = rng.choice(open_)
            uuid, typ, nodes = colls[k]
            values = vals[k]
            others = [u for u, _, _ in colls[k + 1:]]
            r = rng.random()
            if r < 0.12 and values:
                node = (rng.choice(values)[0], rng.choice([C.H_HIDE, C.H_SHOW]))
            elif typ == "map":
                if r < 0.22:
                    node = (rng.choice(KEYS), C.HIDE)
                elif r < 0.27:
                    node = (None, rng.randint(0, 99))
                elif r < 0.32 and values:
                    node = (rng.choice(values)[0], rng.randint(0, 99))
                elif 0.32 <= r < 0.32 + ref_rate and others:
                    node = (rng.choice(KEYS), M.ref(rng.choice(others)))
                else:
                    node = (rng.choice(KEYS), rng.randint(0, 99))
            else:
                cause = rng.choice(values)[0] if values and rng.random() < 0.8 else C.ROOT_ID
                if r < 0.22 and values:
                    node = (rng.choice(values)[0], C.HIDE)
                elif 0.22 <= r < 0.22 + ref_rate and others:
                    node = (cause, M.ref(rng.choice(others)))
                else:
                    node = (cause, rng.randint(0, 99))
            nodes.append(((ts, site, tx),) + node)
            if not C._special(node[1]):
                values.append(nodes[-1])
            left[k] -= 1
    return colls, sites


def collections_of(base):
    return {u: {n[0]: (n[1], n[2]) for n in nodes} for u, _, nodes in base}


def all_ids(base):
    return sorted((n[0] for _, _, nodes in base for n in nodes if n[0] != C.ROOT_ID), key=M.id_key)


SLICE_KINDS = ("one_tx", "range", "everything", "nothing", "no_sites")


def gen_slice(rng, base, sites, kind):
    """(lo id, hi id, sites) in tuple ids."""
    ids = all_ids(base)
    s0 = sites[0]
    if kind == "nothing" or not ids:
        return ((2, s0, 0), (1, s0, 0), None) if kind != "no_sites" else (None, None, set())
    if kind == "no_sites":
        return (None, None, set())
    if kind == "everything":
        return (None, None, None)
    if kind == "one_tx":
        ts, site, _ = rng.choice(ids)
        return ((ts, site, 0), (ts, site, (1 << TX_BITS) - 1), {site})
    a, b = sorted((rng.randrange(len(ids)), rng.randrange(len(ids))))
    return (ids[a], ids[b], None)


def gen_batch(rng, n_bases, max_colls=5, max_nodes=300, kinds=SLICE_KINDS):
    """(bases, slices, new_tx) for pack_bases: n_bases bases of 1..max_colls
    collections of 0..max_nodes nodes, some empty; slice kinds in rotation."""
    bases, slices, new_tx = [], [], []
    for g in range(n_bases):
        sizes = [0 if rng.random() < 0.15 else rng.randint(1, max_nodes) for _ in range(rng.randint(1, max_colls))]
        base, sites = gen_base(rng, sizes, rng.randint(1, 4))
        bases.append(base)
        slices.append(gen_slice(rng, base, sites, kinds[g % len(kinds)]))
        top = max([i[0] for i in all_ids(base)] + [0])
        new_tx.append((top + 1, sites[0]))
    return bases, slices, new_tx
