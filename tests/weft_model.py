"""CPU model of cw_weft_lists at array level (a helper, not a test).

Plain numpy, one document at a time, written from include/causeweave.h and
oracle/causal_ref.py (weft, shared.cljc:268-293); it shares no code with
k_weft_select.  tests/test_weft_model.py pins it to the restatement R.weft,
tests/test_gpu_weft.py compares the library with it array for array.

Also the input builders of both files: ragged batches of generator documents
and the cut recipes (consistent, random node, first / last node, an id that is
no node, site not named).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import oracle
from cause_amd import abi, gen, pack

NO_SRC = 0xFFFFFFFF  # kept_src of an [id] node


def weft_select(offsets, id_key, cause_key, kind, layout, cut):
    """-> (kept_offsets u64[D+1], kept_id u64[M], kept_cause u64[M], kept_kind
    u8[M], kept_src u32[M], weft u32[D]): per document every KIND_ROOT node and
    each named site's ids <= its cut (cut is a node) or whole yarn (it is not),
    in input order; then one [id] node per cut that is no node, by site rank."""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    idk, ck, kd = (np.asarray(id_key, np.uint64), np.asarray(cause_key, np.uint64),
                   np.asarray(kind, np.uint8))
    cut = np.asarray(cut, np.uint64)
    D, S = len(off) - 1, 1 << layout.site_bits
    assert len(cut) == D * S
    shift, mask = np.uint64(layout.site_shift), np.uint64(S - 1)
    ko = np.zeros(D + 1, np.uint64)
    kid, kca, kkd, ksrc = [], [], [], []
    weft = np.zeros(D, np.uint32)
    for d in range(D):
        lo, hi = off[d], off[d + 1]
        ids, dc = idk[lo:hi], cut[d * S:(d + 1) * S]
        named = np.nonzero(dc)[0]
        # the ABI's contract: the word at rank r is an id of the site of rank r
        if np.any(((dc[named] >> shift) & mask) != named.astype(np.uint64)):
            raise ValueError(f"document {d}: a cut word is not an id of its own site rank")
        is_node = np.zeros(S, bool)
        is_node[named] = np.isin(dc[named], ids)
        site = ((ids >> shift) & mask).astype(np.int64)
        c = dc[site]
        keep = ((kd[lo:hi] & pack.KIND_ROOT) != 0) | ((c != 0) & (~is_node[site] | (ids <= c)))
        k = np.nonzero(keep)[0]
        extra = named[~is_node[named]]  # ascending site rank
        kid += [ids[k], dc[extra]]
        kca += [ck[lo:hi][k], np.full(len(extra), pack.NIL, np.uint64)]
        kkd += [kd[lo:hi][k], np.zeros(len(extra), np.uint8)]
        ksrc += [k.astype(np.uint32), np.full(len(extra), NO_SRC, np.uint32)]
        ko[d + 1] = ko[d] + np.uint64(len(k) + len(extra))
        weft[d] = abi.STATUS_WEFT if len(extra) else 0
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return (ko, cat(kid, np.uint64), cat(kca, np.uint64), cat(kkd, np.uint8),
            cat(ksrc, np.uint32), weft)


@dataclasses.dataclass
class WeftExpected:
    offsets: np.ndarray        # uint64[D+1] kept offsets
    src: np.ndarray            # uint32[M]
    kept: tuple                # (id, cause, kind) of the kept nodes
    weave_perm: np.ndarray     # uint32[M] doc-local kept index per weave position
    visible: np.ndarray        # uint8[M] per global kept weave position
    visible_bits: np.ndarray   # uint32[(M+31)//32], laid out by the kept offsets
    visible_count: np.ndarray  # uint32[D]
    max_ts: np.ndarray         # uint64[D] (0 for an empty kept set)
    status: np.ndarray         # uint32[D]: oracle | WEFT (| ROOT on an empty kept set)
    yarn_perm: np.ndarray      # uint32[M]
    oracle_status: np.ndarray  # uint32[D]: the oracle's own word on the kept nodes


def weft_expected(offsets, id_key, cause_key, kind, layout, cut,
                  method=oracle.METHOD_LITERAL) -> WeftExpected:
    ko, kid, kca, kkd, ksrc, weft = weft_select(offsets, id_key, cause_key, kind, layout, cut)
    perm, vis, ost = oracle.batch_lists(ko, kid, kca, kkd, method=method)
    D, M = len(ko) - 1, len(kid)
    b = ko.astype(np.int64)
    vcount = np.array([int(vis[b[d]:b[d + 1]].sum()) for d in range(D)], np.uint32)
    max_ts = np.array([int(kid[b[d]:b[d + 1]].max()) >> layout.ts_shift if b[d + 1] > b[d] else 0
                       for d in range(D)], np.uint64)
    padded = np.zeros((M + 31) // 32 * 32, np.uint8)
    padded[:M] = vis
    bits = np.packbits(padded, bitorder="little").view(np.uint32)
    status = ost | weft
    status[np.diff(b) == 0] |= abi.STATUS_ROOT
    mask = (1 << layout.site_bits) - 1
    yarn = np.zeros(M, np.uint32)
    for d in range(D):
        yarn[b[d]:b[d + 1]] = oracle.list_yarns(kid[b[d]:b[d + 1]], layout.site_shift, mask)
    return WeftExpected(ko, ksrc, (kid, kca, kkd), perm, vis, bits, vcount, max_ts,
                        status.astype(np.uint32), yarn, ost)


# ------------------------------------------------------------------ inputs ----
def spec_for(n_sites, nodes_per_doc):
    return dataclasses.replace(gen.CONFIG2, nodes_per_doc=nodes_per_doc, n_sites=n_sites,
                               shuffle=False)


def ragged(spec, sizes, rng):
    """Documents of ``sizes`` nodes (root included; 0 = empty): id-order
    prefixes of generator documents -- causally closed, causes are older --
    each then permuted.  -> (offsets, id_key, cause_key, kind)."""
    assert max(sizes) <= spec.doc_size
    off, idk, ck, kd = gen.generate(spec, 0, len(sizes))
    parts = []
    for d, n in enumerate(sizes):
        lo, hi = int(off[d]), int(off[d + 1])
        order = lo + np.argsort(idk[lo:hi], kind="stable")[:n]
        parts.append(rng.permutation(order))
    cat = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    o = np.zeros(len(sizes) + 1, np.uint64)
    o[1:] = np.cumsum(sizes)
    return o, idk[cat], ck[cat], kd[cat]


def _absent_ts(ts, rng, top):
    """A ts >= 1 that no id of the yarn has: above every ts of the document,
    below the yarn's first, or in a gap."""
    have = set(int(t) for t in ts)
    pick = []
    if len(ts) and int(ts.min()) > 1:
        pick.append(int(rng.integers(1, int(ts.min()))))  # below the site's first
    pick.append(top + 1 + int(rng.integers(0, 3)))         # above the document's largest
    gaps = [t for t in range(int(ts.min()) + 1, int(ts.max())) if t not in have][:64] \
        if len(ts) else []
    if gaps:
        pick.append(gaps[int(rng.integers(len(gaps)))])
    return pick[int(rng.integers(len(pick)))]


CUT_KINDS = ("consistent", "node", "first", "last", "absent", "unnamed")


def make_cuts(off, idk, layout, rng, modes):
    """cut u64[D << site_bits].  modes[d]: "closed" = every site the consistent
    cut at one T (its last id with ts <= T); "whole" = every site cut at its
    last node; "none" = no site named; "nodes" = every site a random node of
    its own or not named (orphans, never an [id] node); "absent" = every rank
    an id that is no node; "random" = every rank draws one of CUT_KINDS (a rank
    with no node: absent or unnamed)."""
    off = np.asarray(off, np.uint64).astype(np.int64)
    D, S = len(off) - 1, 1 << layout.site_bits
    assert layout.tx_bits == 0
    shift, tss = np.uint64(layout.site_shift), np.uint64(layout.ts_shift)
    cut = np.zeros(D * S, np.uint64)
    for d in range(D):
        ids = np.sort(idk[off[d]:off[d + 1]])
        mode = modes[d]
        if mode == "none":
            continue
        site = ((ids >> shift) & np.uint64(S - 1)).astype(np.int64)
        ts = (ids >> tss).astype(np.int64)
        top = int(ts.max()) if len(ts) else 0
        T = int(rng.integers(1, top + 1)) if top else 1
        for r in range(S):
            y, yts = ids[site == r], ts[site == r]
            if mode == "closed":
                kind = "consistent"
            elif mode == "whole":
                kind = "last"
            elif mode == "absent":
                kind = "absent"
            elif mode == "nodes":
                kind = ("node", "unnamed", "first", "node")[int(rng.integers(4))]
            else:
                kind = CUT_KINDS[int(rng.integers(len(CUT_KINDS)))]
                if len(y) == 0 and kind != "unnamed":
                    kind = "absent" if rng.random() < 0.3 else "unnamed"
            if kind == "unnamed" or len(y) == 0 and kind != "absent":
                continue
            if kind == "absent":
                word = layout.pack(_absent_ts(yts, rng, top), r, 0)
            elif kind == "consistent":
                older = y[yts <= T]
                word = int(older[-1]) if len(older) else 0
            elif kind == "node":
                word = int(y[int(rng.integers(len(y)))])
            else:
                word = int(y[0] if kind == "first" else y[-1])
            cut[d * S + r] = word  # (the root's id is 0: naming it = not naming site "0")
    return cut


# ------------------------------------------------------------------- cases ----
# The inputs of tests/test_gpu_weft.py.  tests/test_weft_model.py checks on the
# CPU that the literal and the general fold agree on the kept documents of
# every one of them and that no oracle status carries CW_STATUS_DUP, so the GPU
# comparison skips no document.
TILE_SIZES = (0, 1, 2, 63, 0, 64, 65, 1023, 1024, 0, 1025, 2047, 2048, 2049, 5001)


def _case(n_sites, sizes, modes, seed):
    rng = np.random.default_rng(seed)
    spec = spec_for(n_sites, max(max(sizes) - 1, 1))
    off, idk, ck, kd = ragged(spec, list(sizes), rng)
    lay = spec.layout()
    return off, idk, ck, kd, lay, make_cuts(off, idk, lay, rng, modes)


def case_tiles():
    """Tile boundaries of k_weft_select (1,024 threads) in a ragged batch of 45
    documents, empty ones interleaved; site_bits = 4."""
    rng = np.random.default_rng(100)
    sizes = list(TILE_SIZES) + [int(x) for x in rng.integers(3, 3000, 26)] + [0, 3073, 0, 4096]
    pattern = ("random", "closed", "nodes", "random", "none", "closed", "whole")
    modes = [pattern[d % len(pattern)] for d in range(len(sizes))]
    modes[14] = "closed"  # the 5,001-node document, causally closed
    return _case(8, sizes, modes, 101)


def case_bits1():
    """site_bits = 1: one site besides the root's."""
    sizes = (1, 2, 3, 0, 300, 1500, 2049, 700, 64, 1025)
    modes = ("none", "whole", "random", "absent", "closed", "nodes", "random", "absent",
             "closed", "nodes")
    return _case(1, sizes, modes, 102)


def case_bits10():
    """site_bits = 10: 1,000 sites, four 5,001-node documents."""
    return _case(1000, (5001,) * 4, ("random", "closed", "nodes", "none"), 103)


def case_all_ranks_absent():
    """Every one of the 1,024 ranks named with an id that is no node: the kept
    size is n + 1,024 = N + (D << site_bits), the capacity of the kept arrays."""
    off, idk, ck, kd, lay, _ = _case(1000, (5001,), ("none",), 104)
    top = int(idk.max()) >> lay.ts_shift
    cut = np.array([lay.pack(top + 1 + r % 5, r, 0) for r in range(1 << lay.site_bits)], np.uint64)
    return off, idk, ck, kd, lay, cut


def case_upper_words():
    """Only ranks >= 32 named (found[] words 1..31), two documents."""
    off, idk, ck, kd, lay, cut = _case(1000, (5001, 1500), ("random", "whole"), 105)
    S = 1 << lay.site_bits
    cut.reshape(-1, S)[:, :32] = 0
    return off, idk, ck, kd, lay, cut


GIANT_N = 70_001


def _giant_doc():
    rng = np.random.default_rng(106)
    spec = spec_for(3, GIANT_N - 1)
    off, idk, ck, kd = ragged(spec, [GIANT_N], rng)
    return off, idk, ck, kd, spec.layout()


def _giant_cuts(idk, lay):
    """Cut rows of the three 70,001-node variants: every yarn whole; the
    consistent cut at the median ts (< 65,536 kept); two yarns whole and the
    third cut at 85% of its length (> 65,535 kept, not closed)."""
    S = 1 << lay.site_bits
    ids = np.sort(idk)
    site = ((ids >> np.uint64(lay.site_shift)) & np.uint64(S - 1)).astype(np.int64)
    ts = (ids >> np.uint64(lay.ts_shift)).astype(np.int64)
    T = int(np.median(ts))
    whole, closed, gib = (np.zeros(S, np.uint64) for _ in range(3))
    for r in range(1, S):
        y = ids[site == r]
        whole[r] = gib[r] = y[-1]
        closed[r] = y[ts[site == r] <= T][-1]
    y = ids[site == S - 1]
    gib[S - 1] = y[len(y) * 85 // 100]
    return whole, closed, gib


def case_giant(variant):
    """One 70,001-node document of 3 sites: variant 0 keeps every node (the
    giant path), 1 a consistent cut below 65,536 kept nodes, 2 a cut that is
    not causally closed with more than 65,535 kept (the exact path)."""
    off, idk, ck, kd, lay = _giant_doc()
    return off, idk, ck, kd, lay, _giant_cuts(idk, lay)[variant]


def case_giant_batch():
    """The three variants as one D = 3 batch."""
    off, idk, ck, kd, lay = _giant_doc()
    o = np.arange(4, dtype=np.uint64) * np.uint64(GIANT_N)
    return (o, np.tile(idk, 3), np.tile(ck, 3), np.tile(kd, 3), lay,
            np.concatenate(_giant_cuts(idk, lay)))


def case_one_5001():
    """A one-document batch of 5,001 nodes (for giant_min = 0)."""
    return _case(8, (5001,), ("random",), 107)


def case_small():
    """Batch B of the reuse sequence: much smaller than case_tiles."""
    return _case(8, (40, 0, 700, 1, 1100), ("random", "none", "closed", "whole", "nodes"), 108)


def case_empty_named():
    """An empty document with one cut named, between a root-only and an empty one."""
    off, idk, ck, kd, lay, cut = _case(8, (1, 0, 0), ("none",) * 3, 109)
    cut[(1 << lay.site_bits) + 3] = lay.pack(7, 3, 0)
    return off, idk, ck, kd, lay, cut


CASES = {
    "tiles": case_tiles, "bits1": case_bits1, "bits10": case_bits10,
    "all_ranks_absent": case_all_ranks_absent, "upper_words": case_upper_words,
    "giant_whole": lambda: case_giant(0), "giant_closed": lambda: case_giant(1),
    "giant_gibberish": lambda: case_giant(2), "giant_batch": case_giant_batch,
    "one_5001": case_one_5001, "small": case_small, "empty_named": case_empty_named,
}
GIANT_CASES = ("giant_whole", "giant_closed", "giant_gibberish", "giant_batch")


@functools.lru_cache(maxsize=None)
def expected(name) -> WeftExpected:
    """The model's answer for CASES[name] (literal fold), computed once a
    process; callers leave it unchanged."""
    return weft_expected(*CASES[name]())


def assert_status_classes(e: WeftExpected, args):
    """A batch with random cuts is nearly all ORPHAN: it must also hold a
    document with status 0, one with ORPHAN and no WEFT, one with WEFT, and a
    nonempty one whose kept set is the root alone because all its cuts are 0."""
    off, _, _, kd, lay, cut = args
    st = e.status
    assert (st == 0).any(), st
    assert (((st & abi.STATUS_ORPHAN) != 0) & ((st & abi.STATUS_WEFT) == 0)).any(), st
    assert ((st & abi.STATUS_WEFT) != 0).any(), st
    rows = cut.reshape(len(st), 1 << lay.site_bits)
    root_alone = [d for d in range(len(st))
                  if not rows[d].any() and e.offsets[d + 1] - e.offsets[d] == 1
                  and off[d + 1] - off[d] > 1
                  and kd[int(off[d]) + int(e.src[int(e.offsets[d])])] & pack.KIND_ROOT]
    assert root_alone, "no document is cut down to its root"


# ------------------------------------------------------------------ mirror ----
def mirror_items(seed=21):
    """The history and cut recipe of tests/test_gpu_merge.py::
    test_weft_matches_reference_restatement: -> [(reference ct, ids, R.weft of them)]."""
    import random

    from oracle import causal_ref as R
    from tests import refgen as G

    rng = random.Random(seed)
    items = []
    for steps in (5, 20, 60, 150):
        for _ in range(25):
            nodes, _ = G.random_history(rng, steps)
            ref = R.new_list_ct(rng=rng)
            ref["nodes"] = {n[0]: (n[1], n[2]) for n in [R.ROOT_NODE] + nodes}
            ref = R.refresh_caches(R.list_weave, ref)
            sites = sorted({n[0][1] for n in nodes})
            ids = []
            T = rng.randint(1, max(n[0][0] for n in nodes))
            for s in sites:
                r = rng.random()
                if r < 0.2:
                    ids.append(rng.choice(ref["yarns"][s])[0])  # arbitrary cut
                elif r < 0.3:
                    ids.append((rng.randint(1, T + 3), s, 7))     # no such node
                elif r < 0.9:  # consistent cut: the site's state at time T
                    older = [n for n in ref["yarns"][s] if n[0][0] <= T]
                    if older:
                        ids.append(older[-1][0])
            if rng.random() < 0.2:
                ids.append((T, R.new_site_id(rng), 0))            # a site with no node
            if not ids:
                continue
            nct = lambda ref=ref: R.new_list_ct(site_id=ref["site_id"], uuid=ref["uuid"])
            items.append((ref, ids, R.weft(R.list_weave, nct, ref, ids)))
    return items


def check_mirror(items, got):
    """got[k] (causal.weft_lists of the items) == R.weft per item; -> (checked,
    gibberish, with a bogus id)."""
    from cause_amd import causal
    from oracle import causal_ref as R

    assert len(got) == len(items)
    gibberish = bogus = 0
    for (ref, ids, want), g in zip(items, got):
        kept = set(want["nodes"])
        gibberish += any(len(b) > 1 and b[0] is not None and b[0] not in kept
                         for b in want["nodes"].values())
        bogus += any(len(b) == 0 for b in want["nodes"].values())
        assert g["weave"] == want["weave"]
        assert causal.causal_list_to_edn(g) == R.causal_list_to_edn(want)
        assert g["lamport_ts"] == want["lamport_ts"]
        assert g["nodes"] == want["nodes"]
        assert g["yarns"] == want["yarns"]
    return len(items), gibberish, bogus
