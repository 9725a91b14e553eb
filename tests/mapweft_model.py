"""CPU model of cw_weft_maps at array level (a helper, not a test).

Plain numpy, one collection at a time, written from include/causeweave.h and
oracle/causal_ref.py (weft, shared.cljc:268-293; map_weave, map.cljc:21-45); it
shares no code with the kernels of mapweft.hip.  tests/test_mapweft_model.py
pins it to the restatement R.weft, tests/test_gpu_map_weft.py compares the
library with it array for array.

Also the input builders of both files: ragged batches of generator collections,
cut tables by the recipes of tests/weft_model.make_cuts, and random map
histories with their cut ids for the mirror.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import oracle
from cause_amd import abi, gen
from cause_amd.pack import KeyLayout
from tests import weft_model as W

NO_SRC = 0xFFFFFFFF  # kept_src of an [id] node


def weft_select_maps(offsets, id_key, cause, cis, kind, site_shift, site_bits, cut):
    """-> (kept_offsets u64[D+1], id u64[M], cause u64[M], cause_is_id u8[M], kind
    u8[M], src u32[M], weft u32[D]): per collection each named site's ids <= its
    cut (the cut is a node) or whole yarn (it is not), in input order; then one
    [id] node per cut that is no node (cause 0, cause_is_id 2, kind 0), by site
    rank.  A map has no root node; nothing is kept of a site that is not named."""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    idk, ck = np.asarray(id_key, np.uint64), np.asarray(cause, np.uint64)
    ci, kd = np.asarray(cis, np.uint8), np.asarray(kind, np.uint8)
    cut = np.asarray(cut, np.uint64)
    D, S = len(off) - 1, 1 << site_bits
    assert len(cut) == D * S
    shift, mask = np.uint64(site_shift), np.uint64(S - 1)
    ko = np.zeros(D + 1, np.uint64)
    parts = [[] for _ in range(5)]
    weft = np.zeros(D, np.uint32)
    for d in range(D):
        lo, hi = off[d], off[d + 1]
        ids, dc = idk[lo:hi], cut[d * S:(d + 1) * S]
        named = np.nonzero(dc)[0]
        # the ABI's contract: the word at rank r is an id of the site of rank r
        if np.any(((dc[named] >> shift) & mask) != named.astype(np.uint64)):
            raise ValueError(f"collection {d}: a cut word is not an id of its own site rank")
        is_node = np.zeros(S, bool)
        is_node[named] = np.isin(dc[named], ids)
        site = ((ids >> shift) & mask).astype(np.int64)
        c = dc[site]
        k = np.nonzero((c != 0) & (~is_node[site] | (ids <= c)))[0]
        extra = named[~is_node[named]]  # ascending site rank
        e = len(extra)
        for p, kept, bogus in zip(parts, (ids[k], ck[lo:hi][k], ci[lo:hi][k], kd[lo:hi][k], k),
                                  (dc[extra], np.zeros(e), np.full(e, 2), np.zeros(e),
                                   np.full(e, NO_SRC))):
            p += [kept, bogus]
        ko[d + 1] = ko[d] + np.uint64(len(k) + e)
        weft[d] = abi.STATUS_WEFT if e else 0
    cat = lambda p, dt: np.concatenate(p).astype(dt) if p else np.zeros(0, dt)
    return (ko,) + tuple(cat(p, dt) for p, dt in zip(parts, (np.uint64, np.uint64, np.uint8, np.uint8,
                                                             np.uint32))) + (weft,)


@dataclasses.dataclass
class MapWeftExpected:
    offsets: np.ndarray   # uint64[D+1] kept offsets
    src: np.ndarray       # uint32[M]
    kept: tuple           # (id, cause, cause_is_id, kind) of the kept nodes
    weft: np.ndarray      # uint32[D]: CW_STATUS_WEFT where the collection got an [id] node
    dup: np.ndarray       # bool[D]: a kept collection repeats an id (its weave is unspecified)
    folds: list           # per collection {key: (active, [kept index in weave order])}


def weft_maps_expected(offsets, id_key, cause, cis, kind, site_shift, site_bits, cut) -> MapWeftExpected:
    """The model's select, then the C oracle's literal map fold of every kept
    collection, in the form of tests/test_gpu_maps.gpu_maps."""
    from tests.test_gpu_maps import oracle_maps

    ko, kid, kca, kci, kkd, ksrc, weft = weft_select_maps(offsets, id_key, cause, cis, kind,
                                                          site_shift, site_bits, cut)
    b = ko.astype(np.int64)
    dup = np.array([len(set(kid[b[d]:b[d + 1]].tolist())) != b[d + 1] - b[d]
                    for d in range(len(b) - 1)], bool)
    return MapWeftExpected(ko, ksrc, (kid, kca, kci, kkd), weft, dup,
                           oracle_maps(ko, kid, kca, kci, kkd))


# ------------------------------------------------------------------ inputs ----
def ragged_maps(n_sites, sizes, seed, p_bad=0.03, n_keys=7):
    """Collections of ``sizes`` nodes (0 = empty): id-order prefixes of generator
    collections -- causally closed, causes are older -- each then permuted.
    -> (offsets, id_key, cause, cause_is_id, kind, KeyLayout, token_bits); the
    site rank of an id is its low site_bits bits (site_shift 0)."""
    rng = np.random.default_rng(seed)
    spec = gen.MapSpec(nodes_per_coll=max(max(sizes, default=1), 1), n_sites=n_sites, n_keys=n_keys,
                       p_bad=p_bad, seed=seed)
    lay, tb = spec.layout()
    off, *cols = gen.generate_maps(spec, 0, len(sizes), nthreads=4)
    parts = []
    for d, n in enumerate(sizes):
        lo, hi = int(off[d]), int(off[d + 1])
        parts.append(rng.permutation(lo + np.argsort(cols[0][lo:hi], kind="stable")[:n]))
    cat = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    o = np.zeros(len(sizes) + 1, np.uint64)
    o[1:] = np.cumsum(sizes)
    return (o,) + tuple(c[cat] for c in cols) + (lay, tb)


MODES = ("random", "closed", "nodes", "none", "whole", "absent")  # of weft_model.make_cuts


def _case(n_sites, sizes, modes, seed, **kw):
    """-> the arguments of weft_select_maps / Weaver.weft_maps order, plus token_bits:
    (off, id, cause, cis, kind, site_shift, site_bits, cut, token_bits)."""
    off, idk, ck, ci, kd, lay, tb = ragged_maps(n_sites, list(sizes), seed, **kw)
    cut = W.make_cuts(off, idk, lay, np.random.default_rng(seed + 1), list(modes))
    return off, idk, ck, ci, kd, lay.site_shift, lay.site_bits, cut, tb


def _cycle(n, first=0):
    return [MODES[(first + d) % len(MODES)] for d in range(n)]


BOUNDARY_SIZES = (0, 1, 2, 63, 0, 64, 65, 511, 512, 0, 513, 1023, 1024, 0, 1025, 2047, 2048)


def case_boundaries():
    """Pack boundaries in a ragged batch of 60 collections, empty ones
    interleaved; site_bits = 4; the cut modes cycle."""
    rng = np.random.default_rng(200)
    sizes = list(BOUNDARY_SIZES) + [int(x) for x in rng.integers(3, 601, 40)] + [0, 600, 0]
    return _case(8, sizes, _cycle(len(sizes)), 201)


def case_pack(limit):
    """Largest collection == limit (512 / 1,024 / 2,048): that pack size."""
    rng = np.random.default_rng(limit)
    sizes = [int(x) for x in rng.integers(1, limit + 1, 12)] + [limit, 0, limit - 1, 3]
    return _case(8, sizes, _cycle(len(sizes), 1), 210 + limit)


def case_lookback():
    """2,500 collections of 40 to 60 nodes: more than 200 packs of 512 nodes, so
    a workgroup has more than 64 predecessors."""
    rng = np.random.default_rng(220)
    sizes = [int(x) for x in rng.integers(40, 61, 2500)]
    return _case(8, sizes, _cycle(len(sizes)), 221)


def case_bits1():
    """site_bits = 1: one site (rank 1; rank 0 has no node)."""
    sizes = (1, 2, 3, 0, 300, 1500, 2048, 700, 64, 1025, 0, 17)
    return _case(1, sizes, _cycle(len(sizes), 2), 230)


def case_bits10():
    """site_bits = 10, 1,000 sites: the slot budget caps a pack's collections
    well below what its nodes would allow."""
    sizes = (300, 0, 2048, 100, 700, 5, 1500, 64, 0, 40, 41, 42, 43, 44, 45)
    return _case(1000, sizes, _cycle(len(sizes)), 240)


def case_all_ranks_absent():
    """Every one of the 1,024 ranks named with an id that is no node: the kept
    size is n + 1,024 = N + (D << site_bits), the capacity of the kept arrays."""
    off, idk, ck, ci, kd, sh, sb, _, tb = _case(1000, (600,), ("none",), 250)
    top = int(idk.max()) >> sb
    cut = np.array([((top + 1 + r % 5) << sb) | r for r in range(1 << sb)], np.uint64)
    return off, idk, ck, ci, kd, sh, sb, cut, tb


def case_upper_words():
    """Only ranks >= 32 named (the upper words of the found bits), three collections."""
    a = _case(1000, (900, 1500, 30), ("random", "whole", "absent"), 260)
    a[7].reshape(-1, 1 << a[6])[:, :32] = 0
    return a


def case_kept_over_2048():
    """A 2,048-node collection whose every rank is named with an id that is no
    node: the fused select keeps 2,048 + 16 nodes, and cw_weave_maps takes its
    general path for the batch."""
    sizes = (50, 2048, 7, 0, 300)
    return _case(8, sizes, ("closed", "absent", "random", "absent", "nodes"), 270)


def case_oversize():
    """A 2,049-node collection in the batch: the whole call takes the general route."""
    sizes = (40, 0, 2049, 512, 3, 700)
    return _case(8, sizes, ("random", "absent", "random", "closed", "whole", "nodes"), 280)


def case_small():
    """The small batch of the reuse sequence."""
    return _case(8, (40, 0, 300, 1, 100), ("random", "none", "closed", "whole", "nodes"), 290)


def case_all_empty():
    """Every collection empty, none named."""
    return _case(8, (0, 0, 0), ("none",) * 3, 300)


def case_empty_named():
    """An empty collection with one cut named (one [id] node, WEFT) between a
    collection cut to nothing and an empty one."""
    a = _case(8, (5, 0, 0), ("none",) * 3, 310)
    a[7][(1 << a[6]) + 3] = (7 << a[6]) | 3
    return a


def case_d0():
    z = lambda dt: np.zeros(0, dt)
    return (np.zeros(1, np.uint64), z(np.uint64), z(np.uint64), z(np.uint8), z(np.uint8), 0, 4,
            z(np.uint64), 3)


CASES = {
    "boundaries": case_boundaries, "pack512": lambda: case_pack(512),
    "pack1024": lambda: case_pack(1024), "pack2048": lambda: case_pack(2048),
    "lookback": case_lookback, "bits1": case_bits1, "bits10": case_bits10,
    "all_ranks_absent": case_all_ranks_absent, "upper_words": case_upper_words,
    "kept_over_2048": case_kept_over_2048, "oversize": case_oversize, "small": case_small,
    "all_empty": case_all_empty, "empty_named": case_empty_named, "d0": case_d0,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """CASES[name](), built once a process; callers leave it unchanged."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name) -> MapWeftExpected:
    """The model's answer for CASES[name], computed once a process."""
    return weft_maps_expected(*case(name)[:8])


def status_classes(e: MapWeftExpected, args):
    """Counts of the collections of each class: kept nonempty with no [id] node
    and every id cause kept ("plain"), with an [id] node ("weft"), nonempty cut
    to nothing ("emptied"), and with an id cause that names no kept node
    ("gibberish")."""
    off = np.asarray(args[0]).astype(np.int64)
    b = e.offsets.astype(np.int64)
    kid, kca, kci, _ = e.kept
    out = dict(plain=0, weft=0, emptied=0, gibberish=0)
    for d in range(len(b) - 1):
        lo, hi = b[d], b[d + 1]
        idc = kci[lo:hi] == 1
        lost = bool((idc & ~np.isin(kca[lo:hi], kid[lo:hi][e.src[lo:hi] != NO_SRC])).any())
        out["gibberish"] += int(lost)
        out["weft"] += int(bool(e.weft[d]))
        out["emptied"] += int(hi == lo and off[d + 1] > off[d])
        out["plain"] += int(hi > lo and not e.weft[d] and not lost)
    return out


# ------------------------------------------------------------------ mirror ----
def mirror_items(seed=41):
    """Random map histories (R.map_assoc / R.map_dissoc from several sites, undo
    and redo nodes inserted under value nodes) and cut ids by the recipe of
    weft_model.mirror_items: consistent, an arbitrary node, an id that is no
    node, a site with no node.  -> [(reference map ct, ids)]."""
    import random

    from oracle import causal_ref as R

    rng = random.Random(seed)
    items = []
    for steps in (4, 12, 30, 60):
        for _ in range(12):
            sites = [R.new_site_id(rng) for _ in range(rng.randint(1, 4))]
            ct = R.new_map_ct(rng=rng)
            values = []
            for _ in range(steps):
                ct = dict(ct, site_id=rng.choice(sites))
                r, k = rng.random(), rng.choice(["a", "b", "c", "d"])
                before = ct["lamport_ts"]
                if r < 0.55:
                    ct = R.map_assoc(ct, k, rng.randint(0, 99))
                    if ct["lamport_ts"] != before:
                        values.append((ct["lamport_ts"], ct["site_id"], 0))
                elif r < 0.7:
                    ct = R.map_dissoc(ct, k)
                elif values:
                    ct = R.append(R.map_weave, ct, rng.choice(values), rng.choice([R.H_HIDE, R.H_SHOW]))
            if not ct["nodes"]:
                continue
            T = rng.randint(1, ct["lamport_ts"])
            ids = []
            for s in sorted(ct["yarns"]):
                r = rng.random()
                if r < 0.2:
                    ids.append(rng.choice(ct["yarns"][s])[0])   # arbitrary cut
                elif r < 0.3:
                    ids.append((rng.randint(1, T + 3), s, 7))    # no such node
                elif r < 0.9:  # consistent cut: the site's state at time T
                    older = [n for n in ct["yarns"][s] if n[0][0] <= T]
                    if older:
                        ids.append(older[-1][0])
            if rng.random() < 0.2:
                ids.append((T, R.new_site_id(rng), 0))           # a site with no node
            if rng.random() < 0.2:
                ids.insert(0, R.ROOT_ID)                          # filtered out
            if rng.random() < 0.15 and ids:
                i = rng.choice(ids)                               # a site named twice: the last wins
                ids.insert(0, (max(i[0] - 1, 1), i[1], i[2]))
            if any(i != R.ROOT_ID for i in ids):
                items.append((ct, ids))
    return items


def padded_map_weave(ct, node=None, more=None):
    """R.map_weave for a ct that may hold one-element nodes: R.map_weave unpacks
    ``i, cause, v = node``, Clojure's destructuring of [id] (map.cljc:30) gives
    cause nil and value nil -- so a body () is padded to (None, None) for the
    fold, and ``nodes`` is restored afterwards."""
    from oracle import causal_ref as R

    padded = dict(ct, nodes={i: b if len(b) else (None, None) for i, b in ct["nodes"].items()})
    return dict(R.map_weave(padded, node, more), nodes=ct["nodes"])


def reference_weft(ct, ids):
    from oracle import causal_ref as R

    return R.weft(padded_map_weave, lambda: R.new_map_ct(site_id=ct["site_id"], uuid=ct["uuid"]), ct, ids)
