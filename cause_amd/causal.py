"""Host-side mirror of the reference's list interface, with the weave on the GPU.

Same names, argument meaning and errors as the reference (causal.collections.
shared / list); a causal tree is a dict with the reference's ct keys
(``nodes``, ``yarns``, ``weave``, ``lamport_ts``, ``site_id``, ``uuid``, ``type``).
Every ``weave`` arity is a full reweave on the MI355X through the C ABI
(cw_weave_lists) -- exact by SURVEY F7 (incremental insertion in any causal
order equals the full reweave).  There is no CPU weave in this module.

    shared.cljc:151-192   insert / append           -> insert, append, insert_bulk
    shared.cljc:300-314   merge-trees               -> merge_trees / merge_lists (cw_merge_lists)
    map.cljc:248-249      causal-merge              -> merge_trees / merge_maps (cw_merge_maps)
    shared.cljc:268-293   weft                      -> weft / weft_lists (cw_weft_lists)
    map.cljc:246-247      weft (maps)               -> map_weft / weft_maps (cw_weft_maps)
    shared.cljc:259-266   refresh-caches            -> refresh_caches
    list.cljc:20-34       weave (all arities)       -> list_weave / weave_lists
    list.cljc:29-34       weave 2/3-arity, incremental (s/weave-node)
                                                    -> list_weave_node / insert_lists (cw_insert_lists)
    map.cljc:29-45        weave 2/3-arity, incremental (s/weave-node on one key weave)
                                                    -> map_weave_node / insert_maps (cw_insert_maps)
    shared.cljc:96-108    (peek yarn) of every yarn -> versions (cw_version)
    shared.cljc:295-299   the diff merge-trees asks for
                                                    -> deltas / sync_lists / sync_maps (cw_delta)
    list.cljc:36-43       conj- / cons-             -> list_conj / list_cons
    list.cljc:48-72       hide? / ->edn / ->list    -> causal_list_to_edn / _to_list
"""
from __future__ import annotations

import random
import threading

import numpy as np

from . import abi, abi_insert, abi_map_insert, abi_sync, pack


class Keyword:
    """A Clojure keyword ``:ns/name``."""

    __slots__ = ("ns", "name")

    def __init__(self, ns, name):
        self.ns, self.name = ns, name

    def __eq__(self, other):
        return (getattr(other, "ns", None), getattr(other, "name", None)) == (self.ns, self.name) \
            and hasattr(other, "ns")

    def __hash__(self):
        return hash(("kw", self.ns, self.name))

    def __repr__(self):
        return f":{self.ns}/{self.name}" if self.ns else f":{self.name}"


HIDE = Keyword("causal", "hide")          # core.cljc:15
H_HIDE = Keyword("causal", "h.hide")
H_SHOW = Keyword("causal", "h.show")
ROOT_ID = (0, "0", 0)                      # shared.cljc:22
ROOT_NODE = (ROOT_ID, None, None)          # shared.cljc:23


class CauseError(Exception):
    """ex-info of the reference: ``causes`` is the :causes set."""

    def __init__(self, msg, causes):
        super().__init__(msg)
        self.causes = causes


_local = threading.local()


def weaver() -> abi.Weaver:
    """This thread's GPU context (device 0).  A cw_ctx is not thread-safe
    (include/causeweave.h), and swap! may run a weave-fn on several threads at
    once: each host thread gets its own context, so calls never share one."""
    w = getattr(_local, "weaver", None)
    if w is None:
        w = _local.weaver = abi.Weaver(0)
    return w


def causal_to_edn(v):
    """s/causal->edn (shared.cljc:320-328): a causal collection (a list or map
    ct held as a value) materialises recursively, anything else is itself."""
    if isinstance(v, dict) and v.get("type") in ("list", "map") and "weave" in v:
        return causal_list_to_edn(v) if v["type"] == "list" else causal_map_to_edn(v)
    return v


def new_node(ts, site, *rest):
    """shared.cljc:77-84"""
    if len(rest) == 2:
        return ((ts, site, 0), rest[0], rest[1])
    tx, cause, value = rest
    return ((ts, site, tx), cause, value)


def _uid(rng, n):
    first = "ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz"
    return rng.choice(first) + "".join(rng.choice("0123456789" + first) for _ in range(n - 1))


def new_site_id(rng=random):
    return _uid(rng, 13)


def new_list_ct(site_id=None, uuid=None, rng=random):
    """list.cljc:11-18"""
    return {"type": "list", "lamport_ts": 0, "uuid": uuid or _uid(rng, 21),
            "site_id": site_id or new_site_id(rng),
            "nodes": {ROOT_ID: (None, None)}, "yarns": {"0": [ROOT_NODE]},
            "weave": [ROOT_NODE], "_visible": [False]}


def weave_lists(cts):
    """Full reweave of many list cts in ONE GPU call (the batch entry point).
    Returns new cts with ::weave, ::yarns, ::lamport-ts and rendered flags."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct in cts]
    try:
        b = pack.pack_lists(docs)
        res = weaver().weave_lists(b.offsets, b.id_key, b.cause_key, b.kind, b.layout)
    except pack.KeyRangeError:  # ids over 63 bits: the K128 layout
        b = pack.pack_lists_k128(docs)
        res = weaver().weave_lists_k128(b.offsets, b.id_key, b.cause_key, b.kind)
    vis = res.visible()
    out = []
    for d, (ct, nodes) in enumerate(zip(cts, docs)):
        lo, hi = int(b.offsets[d]), int(b.offsets[d + 1])
        st = int(res.status[d])
        # c.list/weave's full reweave never throws: absent / non-Lamport / nil
        # causes and a missing root get the literal fold's weave (the library's
        # exact path); only a repeated id is impossible for a ::nodes map
        if st & (abi.STATUS_DUP | abi.STATUS_INTERNAL):
            raise CauseError(f"document outside the weave's domain (status {st})", {"weave-domain"})
        new = dict(ct)
        new["weave"] = [nodes[p] for p in res.weave_perm[lo:hi]]
        new["_visible"] = [bool(v) for v in vis[lo:hi]]
        yarns = {}
        if res.yarn_perm is not None:
            for p in res.yarn_perm[lo:hi]:
                nd = nodes[p]
                yarns.setdefault(nd[0][1], []).append(nd)
        new["yarns"] = yarns
        new["_max_ts"] = int(res.max_ts[d])
        out.append(new)
    return out


def list_weave(ct, node=None, more=None):
    """list.cljc:20-34 -- every arity is the full GPU reweave;
    like the reference, a node that is not in ::nodes leaves ct unchanged."""
    if node is not None and node[0] not in ct["nodes"]:
        return ct
    return weave_lists([ct])[0]


def refresh_caches(weave_fn, ct):
    """shared.cljc:259-266: yarns (spin), lamport-ts (refresh-ts) and the weave
    all come from the one GPU call."""
    out = weave_fn(ct)
    out = dict(out)
    out["lamport_ts"] = out.get("_max_ts", ct["lamport_ts"])
    return out


def insert(weave_fn, ct, node, more=None):
    """shared.cljc:151-184 (same validations, same ex-info causes)."""
    nodes = [node] + list(more or [])
    if len({(n[0][0], n[0][1]) for n in nodes}) > 1:
        raise CauseError("All nodes must belong to the same tx.", {"txs"})
    existing = ct["nodes"].get(node[0])
    if existing is not None:
        if (node[1], node[2]) == existing:
            return ct
        raise CauseError("This node is already in the tree and can't be changed.",
                         {"append-only", "edits-not-allowed"})
    is_key = isinstance(node[1], (str, Keyword))
    if not is_key and node[1] not in ct["nodes"]:
        raise CauseError("The cause of this node is not in the tree.", {"cause-must-exist"})
    out = dict(ct)
    if node[0][0] > ct["lamport_ts"]:
        out["lamport_ts"] = node[0][0]
    nm = dict(ct["nodes"])
    for n in nodes:
        nm[n[0]] = (n[1], n[2])
    out["nodes"] = nm
    woven = weave_fn(out, node, more)
    woven = dict(woven)
    woven["lamport_ts"] = out["lamport_ts"]
    return woven


class _Tokens:
    """Value identity for the merge's body check (equal values <=> equal token)."""

    def __init__(self):
        self.t = {}

    def __call__(self, v):
        try:
            key = ("h", type(v).__name__, v)
            hash(key)
        except TypeError:
            key = ("r", repr(v))
        return self.t.setdefault(key, len(self.t))


def insert_lists(items):
    """s/insert with the incremental weave (c.list/weave's 2/3-arity over
    s/weave-node, list.cljc:29-34, shared.cljc:225-241) for many ``(ct, node,
    more)`` in ONE GPU call (cw_insert_lists): each ct's current ``weave`` is
    packed as it stands and its tx spliced in, no reweave.  Same validations and
    ex-info causes as ``insert``; a node already in the tree with the same body
    returns its ct unchanged.  The yarns of a new ct come from the call's
    yarn_perm, its rendered flags from the call's visible_bits.  Ids that need
    the K128 layout (over 63 bits) raise a CauseError with cause "key-range":
    ``list_weave`` reweaves such a ct."""
    txs = []
    for ct, node, more in items:
        tx = [node] + list(more or [])
        if len({(n[0][0], n[0][1]) for n in tx}) > 1:
            raise CauseError("All nodes must belong to the same tx.", {"txs"})
        txs.append(tx)
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct, _, _ in items]
    try:
        pk = pack.pack_lists([d + tx for d, tx in zip(docs, txs)], min_site_bits=1)  # one site ranking
    except pack.KeyRangeError as e:  # ids over 63 bits: cw_insert_lists has no K128 form
        raise CauseError(f"insert_lists takes ids that pack into 63 bits ({e}); "
                         "list_weave reweaves such a ct", {"key-range"}) from e
    tok = _Tokens()
    vals = np.array([tok(n[2]) for d in pk.docs for n in d.nodes], np.uint64)
    sel, tsel, perm, vis, yarn = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [], [], []
    for d, ((ct, _, _), nodes, tx, pd) in enumerate(zip(items, docs, txs, pk.docs)):
        lo, n = int(pk.offsets[d]), len(nodes)
        sel.append(np.arange(lo, lo + n))
        tsel.append(np.arange(lo + n, lo + n + len(tx)))
        at = {nd[0]: s for s, nd in enumerate(nodes)}
        perm += [at[nd[0]] for nd in ct["weave"]]
        vis += [bool(v) for v in ct["_visible"]]
        ys = ct.get("yarns") or {}
        if sum(len(y) for y in ys.values()) != n:  # a ct without its ::yarns cache: spin (shared.cljc:121-132)
            ys = {}
            for nd in sorted(nodes, key=lambda nd: (nd[0][0], pack.java_str_key(nd[0][1]), nd[0][2])):
                ys.setdefault(nd[0][1], []).append(nd)
        for site in sorted(ys, key=lambda s: pd.site_rank[s]):
            yarn += [at[nd[0]] for nd in ys[site]]
    sel, tsel = np.concatenate(sel), np.concatenate(tsel)
    N = len(sel)
    if len(perm) != N or len(vis) != N:
        raise CauseError("a ct's weave does not hold its nodes", {"weave-domain"})
    bits = np.zeros((N + 31) // 32 * 32, np.uint8)
    bits[:N] = vis
    bits = np.packbits(bits, bitorder="little").view(np.uint32)
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    toff = np.zeros(len(items) + 1, np.uint64)
    toff[1:] = np.cumsum([len(t) for t in txs])
    res = abi_insert.insert_lists(
        weaver(), (off, pk.id_key[sel], pk.cause_key[sel], pk.kind[sel]), np.array(perm, np.uint32),
        bits, (toff, pk.id_key[tsel], pk.cause_key[tsel], pk.kind[tsel], vals[tsel]), pk.layout,
        yarn_perm=np.array(yarn, np.uint32), doc_value=vals[sel], columns=False)
    rendered = res.weave.visible()
    out = []
    for d, ((ct, _, _), nodes, tx) in enumerate(zip(items, docs, txs)):
        st = int(res.weave.status[d])
        if st & abi.STATUS_DUP:
            raise CauseError("This node is already in the tree and can't be changed.",
                             {"append-only", "edits-not-allowed"})
        if st & abi.STATUS_ORPHAN:
            raise CauseError("The cause of this node is not in the tree.", {"cause-must-exist"})
        if int(res.insert_pos[d]) == 0xFFFFFFFF:  # nothing inserted: the same node again
            out.append(ct)
            continue
        lo, hi = int(res.offsets[d]), int(res.offsets[d + 1])
        both = nodes + tx
        new = dict(ct)
        nm = dict(ct["nodes"])
        for n in tx:
            nm[n[0]] = (n[1], n[2])
        new["nodes"] = nm
        new["weave"] = [both[s] for s in res.weave.weave_perm[lo:hi]]
        new["_visible"] = [bool(v) for v in rendered[lo:hi]]
        yarns = {}
        for s in res.weave.yarn_perm[lo:hi]:
            yarns.setdefault(both[s][0][1], []).append(both[s])
        new["yarns"] = yarns
        new["_max_ts"] = int(res.weave.max_ts[d])
        if tx[0][0][0] > ct["lamport_ts"]:  # shared.cljc:179-181
            new["lamport_ts"] = tx[0][0][0]
        out.append(new)
    return out


def list_weave_node(ct, node=None, more=None):
    """A weave-fn for ``insert`` / ``append`` that weaves incrementally
    (list.cljc:29-34): ``ct`` holds the tx in ::nodes already, its ``weave``
    does not.  Without a node it is the full reweave (``list_weave``)."""
    if node is None:
        return list_weave(ct)
    if node[0] not in ct["nodes"]:
        return ct
    tx = [node] + list(more or [])
    base = dict(ct)
    base["nodes"] = {i: b for i, b in ct["nodes"].items() if all(i != n[0] for n in tx)}
    return insert_lists([(base, node, more)])[0]


def merge_lists(pairs):
    """s/merge-trees (shared.cljc:300-314) for many (ct1, ct2) list pairs in ONE
    GPU call (cw_merge_lists): the union of the two ::nodes maps, deduplicated,
    then the full reweave.  Same checks and ex-info causes as the
    reference; see include/causeweave.h for the one divergence (the reference
    can also throw :cause-must-exist because of its hash-map insertion order)."""
    for ct1, ct2 in pairs:
        if ct1["type"] != ct2["type"]:
            raise CauseError("Causal type missmatch. Merge not allowed.", {"type-missmatch"})
        if ct1["uuid"] != ct2["uuid"]:
            raise CauseError("Causal UUID missmatch. Merge not allowed.", {"uuid-missmatch"})
    da = [[(i, b[0], b[1]) for i, b in ct1["nodes"].items()] for ct1, _ in pairs]
    db = [[(i, b[0], b[1]) for i, b in ct2["nodes"].items()] for _, ct2 in pairs]
    pk = pack.pack_lists([a + b for a, b in zip(da, db)])  # one site ranking per pair
    tok = _Tokens()
    ia, ib = [], []
    for d, (a, b) in enumerate(zip(da, db)):
        lo = int(pk.offsets[d])
        ia.append(np.arange(lo, lo + len(a)))
        ib.append(np.arange(lo + len(a), lo + len(a) + len(b)))
    ia = np.concatenate(ia) if ia else np.zeros(0, np.int64)
    ib = np.concatenate(ib) if ib else np.zeros(0, np.int64)
    vals = np.array([tok(n[2]) for d in pk.docs for n in d.nodes], np.uint64)
    off_a = np.zeros(len(pairs) + 1, np.uint64)
    off_a[1:] = np.cumsum([len(a) for a in da])
    off_b = np.zeros(len(pairs) + 1, np.uint64)
    off_b[1:] = np.cumsum([len(b) for b in db])
    side = lambda idx, off: (off, pk.id_key[idx], pk.cause_key[idx], pk.kind[idx], vals[idx])
    res = weaver().merge_lists(side(ia, off_a), side(ib, off_b), pk.layout)
    return _merged_lists(res, [ct1 for ct1, _ in pairs], da, db)


def _merged_lists(res, firsts, da, db):
    """The merged cts of a cw_merge_lists result: document d is firsts[d] with
    the nodes da[d] (side a) and db[d] (side b)."""
    vis = res.weave.visible()
    out = []
    for d, (ct1, a, b) in enumerate(zip(firsts, da, db)):
        st = int(res.weave.status[d])
        if st & abi.STATUS_DUP:
            raise CauseError("This node is already in the tree and can't be changed.",
                             {"append-only", "edits-not-allowed"})
        if st & abi.STATUS_ORPHAN:
            raise CauseError("The cause of this node is not in the tree.", {"cause-must-exist"})
        if st:
            raise CauseError(f"document outside the weave's domain (status {st})", {"weave-domain"})
        lo, hi = int(res.offsets[d]), int(res.offsets[d + 1])
        src = res.src[lo:hi]
        node_of = lambda s: a[s] if s < len(a) else b[s - len(a)]
        merged = [node_of(int(s)) for s in src]
        new = dict(ct1)
        new["nodes"] = {n[0]: (n[1], n[2]) for n in merged}
        new["weave"] = [merged[p] for p in res.weave.weave_perm[lo:hi]]
        new["_visible"] = [bool(v) for v in vis[lo:hi]]
        yarns = {}
        for p in res.weave.yarn_perm[lo:hi]:
            nd = merged[p]
            yarns.setdefault(nd[0][1], []).append(nd)
        new["yarns"] = yarns
        # insert fast-forwards ::lamport-ts to every newly inserted node (shared.cljc:179-181)
        fresh = [merged[i][0][0] for i, s in enumerate(src) if s >= len(a)]
        new["lamport_ts"] = max([ct1["lamport_ts"]] + fresh)
        new["_max_ts"] = int(res.weave.max_ts[d])
        out.append(new)
    return out


def merge_trees(weave_fn, ct1, ct2):
    """shared.cljc:300-314; the weave-fn is the GPU weave of ct1's type (a list
    merges through cw_merge_lists, a map through cw_merge_maps)."""
    if ct1["type"] != ct2["type"]:
        raise CauseError("Causal type missmatch. Merge not allowed.", {"type-missmatch"})
    if ct1["type"] == "map":
        return merge_maps([(ct1, ct2)])[0]
    return merge_lists([(ct1, ct2)])[0]


def insert_bulk(ct, nodes):
    """Many s/insert calls (shared.cljc:151-184) in causal order, as one GPU
    merge of ``nodes`` into ``ct``."""
    ct2 = dict(ct)
    ct2["nodes"] = {n[0]: (n[1], n[2]) for n in nodes}
    return merge_trees(list_weave, ct, ct2)


def weft_lists(items):
    """s/weft (shared.cljc:268-293) for many (ct, ids-to-cut-yarns) list pairs in
    ONE GPU call (cw_weft_lists): time travel to the cut, then the full reweave.
    A cut id that is not a node keeps its site's whole yarn plus the
    one-element node ``(id,)`` (``(new-node [id nil])``), last in that yarn."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct, _ in items]
    cuts = []
    for ct, ids in items:
        last = {}
        for i in ids:  # (assoc-in [::yarns site] ..): the last id of a site wins
            if i != ROOT_ID:
                last[i[1]] = i
        cuts.append(last)
    pk = pack.pack_lists(docs, min_site_bits=1,  # cw_weft_lists indexes cuts by site rank
                         extra_ids=[list(c.values()) for c in cuts])
    lay = pk.layout
    S = 1 << lay.site_bits
    cut = np.zeros(len(items) << lay.site_bits, np.uint64)
    for d, (last, pd) in enumerate(zip(cuts, pk.docs)):
        for site, i in last.items():
            cut[d * S + pd.site_rank[site]] = lay.pack(i[0], pd.site_rank[site], i[2])
    res = weaver().weft_lists(pk.offsets, pk.id_key, pk.cause_key, pk.kind, lay, cut)
    vis = res.weave.visible()
    out = []
    for d, ((ct, ids), nodes, last, pd) in enumerate(zip(items, docs, cuts, pk.docs)):
        st = int(res.weave.status[d])
        if st & (abi.STATUS_DUP | abi.STATUS_INTERNAL):
            raise CauseError(f"weft outside the weave's domain (status {st})", {"weave-domain"})
        lo, hi = int(res.offsets[d]), int(res.offsets[d + 1])
        # the [id] nodes come after the kept nodes, in site-rank order
        bogus = iter(sorted((i for i in last.values() if i not in ct["nodes"]),
                            key=lambda i: pd.site_rank[i[1]]))
        kept = [nodes[s] if s != 0xFFFFFFFF else (next(bogus),) for s in res.src[lo:hi]]
        new = new_list_ct(site_id=ct["site_id"], uuid=ct["uuid"])
        new["nodes"] = {n[0]: tuple(n[1:]) for n in kept}
        new["weave"] = [kept[p] for p in res.weave.weave_perm[lo:hi]]
        new["_visible"] = [bool(v) for v in vis[lo:hi]]
        yarns = {}
        for p in res.weave.yarn_perm[lo:hi]:
            yarns.setdefault(kept[p][0][1], []).append(kept[p])
        for y in yarns.values():  # (conj yarn-prefix [id]): the [id] node is last
            y.sort(key=lambda n: len(n) == 1)
        new["yarns"] = yarns
        new["lamport_ts"] = max(i[0] for i in ids if i != ROOT_ID)
        out.append(new)
    return out


def weft(ct, ids):
    """(c/weft causal-list ids) -- list.cljc:165-166 over shared.cljc:268-293."""
    return weft_lists([(ct, ids)])[0]


def append(weave_fn, ct, cause, value):
    """shared.cljc:186-192"""
    ct2 = dict(ct)
    ct2["lamport_ts"] = ct["lamport_ts"] + 1
    return insert(weave_fn, ct2, new_node(ct2["lamport_ts"], ct2["site_id"], cause, value))


def list_conj(ct, v):
    """list.cljc:36-40"""
    return append(list_weave, ct, ct["weave"][-1][0], v)


def list_cons(v, ct):
    """list.cljc:42-43"""
    return append(list_weave, ct, ROOT_ID, v)


def causal_list_to_list(ct):
    """list.cljc:68-72 (rendered flags from the GPU, hide? list.cljc:48-55)."""
    return [n for n, v in zip(ct["weave"], ct["_visible"]) if v]


def causal_list_to_edn(ct):
    """list.cljc:57-66: (peek node) of every rendered node, nested causal
    values materialised (s/causal->edn, list.cljc:64-66)"""
    return [causal_to_edn(n[-1]) for n in causal_list_to_list(ct)]


def count(ct):
    """list.cljc:77"""
    return len(causal_list_to_list(ct))


def lists_to_edn(cts):
    """causal-list->edn (list.cljc:57-66) of many list cts, woven and rendered
    on the GPU (cw_weave_lists, then cw_render_lists): per ct the list
    causal_list_to_edn gives after a reweave, without the host filter.  When
    every value of the batch is a single character the values go along as a
    code-point column and the documents come back as rendered_value;
    otherwise rendered_src is mapped back to the nodes' values."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct in cts]
    w = weaver()
    try:
        b = pack.pack_lists(docs)
        res = w.weave_lists(b.offsets, b.id_key, b.cause_key, b.kind, b.layout, yarns=False)
    except pack.KeyRangeError:  # ids over 63 bits: the K128 layout
        b = pack.pack_lists_k128(docs)
        res = w.weave_lists_k128(b.offsets, b.id_key, b.cause_key, b.kind, yarns=False)
    for st in res.status.tolist():
        if st & (abi.STATUS_DUP | abi.STATUS_INTERNAL):
            raise CauseError(f"document outside the weave's domain (status {st})", {"weave-domain"})
    # root and special nodes never render (hide?, list.cljc:48-55): their word is 0
    plain = [n[2] for nodes in docs for n in nodes if n[0] != ROOT_ID and not _special(n[2])]
    chars = all(isinstance(v, str) and len(v) == 1 for v in plain)
    codes = None
    if chars:
        codes = np.array([ord(n[2]) if isinstance(n[2], str) and len(n[2]) == 1 else 0
                          for nodes in docs for n in nodes], np.uint32)
    r = w.render_lists(b.offsets, res.weave_perm, res.visible_bits, codes)
    out = []
    for d, nodes in enumerate(docs):
        lo, hi = int(r.offsets[d]), int(r.offsets[d + 1])
        if chars:
            out.append([chr(c) for c in r.value[lo:hi].tolist()])
        else:
            out.append([causal_to_edn(nodes[s][2]) for s in r.src[lo:hi].tolist()])
    return out


def _special(v):
    """shared.cljc:21 special-keywords"""
    return pack.kind_of(v) != pack.KIND_NORMAL


# ------------------------------------------------------------------------- maps
# map.cljc: the map interface over cw_weave_maps.  A map ct's ``weave`` is
# {key: key weave (root first)}; ``_active`` is {key: active node or BLANK}.
BLANK = Keyword("causal.collections.map", "blank")   # ::blank, map.cljc:52


def new_map_ct(site_id=None, uuid=None, rng=random):
    """map.cljc:12-19"""
    return {"type": "map", "lamport_ts": 0, "uuid": uuid or _uid(rng, 21),
            "site_id": site_id or new_site_id(rng), "nodes": {}, "yarns": {}, "weave": {},
            "_active": {}}


def _unpack_id(key, layout, rank):
    if key == 0:
        return ROOT_ID  # the virtual root packs to 0 (pack.pack_maps)
    inv = {r: s for s, r in rank.items()}
    ts = key >> layout.ts_shift
    site = (key >> layout.site_shift) & ((1 << layout.site_bits) - 1)
    tx = key & ((1 << layout.tx_bits) - 1)
    return (ts, inv[site], tx)


def weave_maps(cts):
    """Full reweave of many map cts in ONE GPU call (c.map/weave 1-arity,
    map.cljc:21-28, for each); also computes active-node per key."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct in cts]
    pm = pack.pack_maps(docs)
    res = weaver().weave_maps(pm.offsets, pm.id_key, pm.cause, pm.cause_is_id, pm.kind,
                              pm.token_bits, pm.layout.key_bits)
    out = []
    segs_of = _segs_by_coll(res)
    for d, (ct, nodes) in enumerate(zip(cts, docs)):
        st = int(res.status[d])
        # non-Lamport causes and causes that are not nodes are the literal
        # fold's (the library's fused map path); a repeated id, a key token
        # out of range or an internal check are not a ::nodes map it weaves
        if st & (abi.STATUS_DUP | abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL):
            raise CauseError(f"map outside the weave's domain (status {st})", {"weave-domain"})
        new = dict(ct)
        new["weave"], new["_active"] = _key_weaves(res, segs_of.get(d, []), nodes, pm, d)
        out.append(new)
    return out


def _segs_by_coll(res):
    segs_of = {}
    for s, d in enumerate(res.seg_coll.tolist()):
        segs_of.setdefault(d, []).append(s)
    return segs_of


def _seg_key(k, pm, d):
    """The map key a seg_key word of collection d stands for."""
    if k == pack.NIL:
        return None
    if k >> 63:
        return _unpack_id(k & ((1 << 63) - 1), pm.layout, pm.ranks[d])
    return pm.keys[k]


def _key_weaves(res, segs, nodes, pm, d):
    """{key: key weave} and {key: active node} of collection d from the key
    weaves `segs` of a cw_map_result, whose indices point into `nodes`."""
    weave, active = {}, {}
    for s in segs:
        key = _seg_key(int(res.seg_key[s]), pm, d)
        # nodes are woven as [id cause-in-weave v] (map.cljc:35-41)
        weave[key] = [ROOT_NODE] + [
            (nodes[p][0], nodes[p][1] if pack.valid_id(nodes[p][1]) else ROOT_ID, nodes[p][2])
            for p in res.key_weave(s)[1:]]
        a = int(res.seg_active[s])
        active[key] = BLANK if a < 0 else (nodes[a][0], key, nodes[a][2])
    return weave, active


def merge_maps(pairs):
    """CausalMap's causal-merge (map.cljc:248-249: s/merge-trees, shared.cljc:
    300-314, with the map weave) for many (ct1, ct2) map pairs in ONE GPU call
    (cw_merge_maps): the union of the two ::nodes maps, deduplicated, then the
    full map reweave.  Same checks and ex-info causes as the reference; see
    include/causeweave.h for where the reference's own result depends on its
    hash-map insertion order."""
    for ct1, ct2 in pairs:
        if ct1["type"] != ct2["type"]:
            raise CauseError("Causal type missmatch. Merge not allowed.", {"type-missmatch"})
        if ct1["uuid"] != ct2["uuid"]:
            raise CauseError("Causal UUID missmatch. Merge not allowed.", {"uuid-missmatch"})
    da = [[(i, b[0], b[1]) for i, b in ct1["nodes"].items()] for ct1, _ in pairs]
    db = [[(i, b[0], b[1]) for i, b in ct2["nodes"].items()] for _, ct2 in pairs]
    # one site ranking and one key-token table per pair
    pm = pack.pack_maps([a + b for a, b in zip(da, db)])
    tok = _Tokens()
    vals = np.array([tok(n[2]) for d in pm.docs for n in d], np.uint64)
    ia, ib = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for d, (a, b) in enumerate(zip(da, db)):
        lo = int(pm.offsets[d])
        ia.append(np.arange(lo, lo + len(a)))
        ib.append(np.arange(lo + len(a), lo + len(a) + len(b)))
    ia, ib = np.concatenate(ia), np.concatenate(ib)
    off_a = np.zeros(len(pairs) + 1, np.uint64)
    off_a[1:] = np.cumsum([len(a) for a in da])
    off_b = np.zeros(len(pairs) + 1, np.uint64)
    off_b[1:] = np.cumsum([len(b) for b in db])
    side = lambda idx, off: (off, pm.id_key[idx], pm.cause[idx], pm.cause_is_id[idx], pm.kind[idx],
                             vals[idx])
    res = weaver().merge_maps(side(ia, off_a), side(ib, off_b), pm.token_bits, pm.layout.key_bits)
    return _merged_maps(res, [ct1 for ct1, _ in pairs], da, db, pm, range(len(pairs)))


def _merged_maps(res, firsts, da, db, pm, packed_as):
    """The merged cts of a cw_merge_maps result: collection d is firsts[d] with
    the nodes da[d] (side a) and db[d] (side b), packed as pm's collection
    packed_as[d] (its site ranks)."""
    segs_of = _segs_by_coll(res.maps)
    out = []
    for d, (ct1, a, b) in enumerate(zip(firsts, da, db)):
        st = int(res.maps.status[d])
        if st & abi.STATUS_DUP:
            raise CauseError("This node is already in the tree and can't be changed.",
                             {"append-only", "edits-not-allowed"})
        if st & abi.STATUS_ORPHAN:
            raise CauseError("The cause of this node is not in the tree.", {"cause-must-exist"})
        if st & (abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL):
            raise CauseError(f"map outside the weave's domain (status {st})", {"weave-domain"})
        lo, hi = int(res.offsets[d]), int(res.offsets[d + 1])
        src = res.src[lo:hi]
        merged = [a[s] if s < len(a) else b[s - len(a)] for s in src.tolist()]
        new = dict(ct1)
        new["nodes"] = {n[0]: (n[1], n[2]) for n in merged}
        new["weave"], new["_active"] = _key_weaves(res.maps, segs_of.get(d, []), merged, pm, packed_as[d])
        # insert fast-forwards ::lamport-ts to every newly inserted node (shared.cljc:179-181)
        fresh = [merged[i][0][0] for i, s in enumerate(src.tolist()) if s >= len(a)]
        new["lamport_ts"] = max([ct1["lamport_ts"]] + fresh)
        out.append(new)
    return out


def weft_maps(items):
    """CausalMap's weft (map.cljc:246-247: s/weft, shared.cljc:268-293, with the
    map weave) for many (map ct, ids-to-cut-yarns) pairs in ONE GPU call
    (cw_weft_maps): time travel to the cut, then the full map reweave.  A cut id
    that is not a node keeps its site's whole yarn plus the one-element node
    ``(id,)`` (body ``()`` in ``nodes``), last in that yarn and woven as
    ``(id, ROOT_ID, None)`` under the nil key (map.cljc:30)."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct, _ in items]
    cuts = []
    for ct, ids in items:
        last = {}
        for i in ids:  # (assoc-in [::yarns site] ..): the last id of a site wins
            if i != ROOT_ID:
                last[i[1]] = i
        cuts.append(last)
    pm = pack.pack_maps(docs, extra_ids=[list(c.values()) for c in cuts],
                        min_site_bits=1)  # cw_weft_maps indexes cuts by site rank
    lay = pm.layout
    S = 1 << lay.site_bits
    cut = np.zeros(len(items) << lay.site_bits, np.uint64)
    for d, (last, rank) in enumerate(zip(cuts, pm.ranks)):
        for site, i in last.items():
            word = lay.pack(i[0], rank[site], i[2])
            if word == 0:  # (0 = site not named: only an id sorting at the root id packs so)
                raise pack.KeyRangeError(f"cut id {i} sorts at the root id")
            cut[d * S + rank[site]] = word
    res = weaver().weft_maps(pm.offsets, pm.id_key, pm.cause, pm.cause_is_id, pm.kind,
                             pm.token_bits, lay.site_shift, lay.site_bits, cut, lay.key_bits)
    segs_of = _segs_by_coll(res.maps)
    out = []
    for d, ((ct, ids), nodes, last) in enumerate(zip(items, docs, cuts)):
        st = int(res.maps.status[d])
        if st & (abi.STATUS_DUP | abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL):
            raise CauseError(f"weft outside the weave's domain (status {st})", {"weave-domain"})
        lo, hi = int(res.offsets[d]), int(res.offsets[d + 1])
        # the [id] nodes come after the kept nodes, in site-rank order; woven
        # they destructure to cause nil, value nil
        bogus = iter(sorted((i for i in last.values() if i not in ct["nodes"]),
                            key=lambda i: pm.ranks[d][i[1]]))
        kept = [nodes[s] if s != 0xFFFFFFFF else (next(bogus), None, None)
                for s in res.src[lo:hi].tolist()]
        is_bogus = [s == 0xFFFFFFFF for s in res.src[lo:hi].tolist()]
        new = new_map_ct(site_id=ct["site_id"], uuid=ct["uuid"])
        new["nodes"] = {n[0]: () if b else (n[1], n[2]) for n, b in zip(kept, is_bogus)}
        new["weave"], new["_active"] = _key_weaves(res.maps, segs_of.get(d, []), kept, pm, d)
        yarns = {}
        # yarns on the host: id order, (conj yarn-prefix [id]) puts the [id] node last
        for n, b in sorted(zip(kept, is_bogus), key=lambda t: (t[1], t[0][0][0], t[0][0][2])):
            yarns.setdefault(n[0][1], []).append((n[0],) if b else n)
        new["yarns"] = yarns
        new["lamport_ts"] = max(i[0] for i in ids if i != ROOT_ID)
        out.append(new)
    return out


def map_weft(ct, ids):
    """(c/weft causal-map ids) -- map.cljc:246-247 over shared.cljc:268-293."""
    return weft_maps([(ct, ids)])[0]


def map_insert_bulk(ct, nodes):
    """Many s/insert calls (shared.cljc:151-184) into a map ct, as one GPU merge
    of ``nodes`` into ``ct`` (the twin of insert_bulk)."""
    ct2 = dict(ct)
    ct2["nodes"] = {n[0]: (n[1], n[2]) for n in nodes}
    return merge_trees(map_weave, ct, ct2)


def map_weave(ct, node=None, more=None):
    """map.cljc:21-45 -- every arity is the full GPU reweave."""
    if node is not None and node[0] not in ct["nodes"]:
        return ct
    return weave_maps([ct])[0]


def insert_maps(items):
    """s/insert with the incremental map weave (c.map/weave's 2/3-arity over
    s/weave-node, map.cljc:29-45) for many ``(ct, node, more)`` in ONE GPU call
    (cw_insert_maps): each ct's key weaves are packed as they stand and its tx
    woven in node by node, no reweave.  Same validations and ex-info causes as
    ``insert``; a node already in the collection with the same body returns its
    ct unchanged.  Only the key weaves the tx went to are rebuilt."""
    txs = []
    for ct, node, more in items:
        tx = [node] + list(more or [])
        if len({(n[0][0], n[0][1]) for n in tx}) > 1:
            raise CauseError("All nodes must belong to the same tx.", {"txs"})
        txs.append(tx)
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct, _, _ in items]
    pm = pack.pack_maps([d + tx for d, tx in zip(docs, txs)])  # one site ranking, one key-token table
    tok = _Tokens()
    vals = np.array([tok(n[2]) for d in pm.docs for n in d], np.uint64)
    ktok = {k: t for t, k in enumerate(pm.keys)}
    sel, tsel = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    so, sc, sk, sa, sp = [0], [], [], [], []
    for d, ((ct, _, _), nodes, tx) in enumerate(zip(items, docs, txs)):
        lo, n = int(pm.offsets[d]), len(nodes)
        sel.append(np.arange(lo, lo + n))
        tsel.append(np.arange(lo + n, lo + n + len(tx)))
        at = {nd[0]: s for s, nd in enumerate(nodes)}
        words = {}
        for k in ct["weave"]:
            if k is None:
                words[pack.NIL] = k
            elif pack.valid_id(k):
                words[1 << 63 | (0 if k == ROOT_ID else pm.layout.pack(k[0], pm.ranks[d][k[1]], k[2]))] = k
            else:
                words[ktok[k]] = k
        for word in sorted(words):
            k = words[word]
            a = ct["_active"].get(k, BLANK)
            sc.append(d)
            sk.append(word)
            sa.append(-1 if a is BLANK else at[a[0]])
            sp += [0xFFFFFFFF] + [at[nd[0]] for nd in ct["weave"][k][1:]]
            so.append(len(sp))
    sel, tsel = np.concatenate(sel), np.concatenate(tsel)
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    toff = np.zeros(len(items) + 1, np.uint64)
    toff[1:] = np.cumsum([len(t) for t in txs])
    if len(sp) != len(sel) + len(sk):
        raise CauseError("a ct's weave does not hold its nodes", {"weave-domain"})
    res = abi_map_insert.insert_maps(
        weaver(), (off, pm.id_key[sel], pm.cause[sel], pm.cause_is_id[sel], pm.kind[sel]),
        (np.array(so, np.uint64), np.array(sc, np.uint32), np.array(sk, np.uint64), np.array(sa, np.int64),
         np.array(sp, np.uint32)),
        (toff, pm.id_key[tsel], pm.cause[tsel], pm.cause_is_id[tsel], pm.kind[tsel], vals[tsel]),
        coll_value=vals[sel], columns=False)
    out = []
    for d, ((ct, _, _), nodes, tx) in enumerate(zip(items, docs, txs)):
        st = int(res.maps.status[d])
        if st & abi.STATUS_DUP:
            raise CauseError("This node is already in the tree and can't be changed.",
                             {"append-only", "edits-not-allowed"})
        if st & abi.STATUS_ORPHAN:
            raise CauseError("The cause of this node is not in the tree.", {"cause-must-exist"})
        if st & abi.STATUS_MAP_KEY:
            raise CauseError(f"map outside the weave's domain (status {st})", {"weave-domain"})
        t0 = int(toff[d])
        if int(res.tx_seg[t0]) == 0xFFFFFFFF:  # nothing inserted: the same node again
            out.append(ct)
            continue
        both = nodes + tx
        new = dict(ct)
        nm = dict(ct["nodes"])
        for n in tx:
            nm[n[0]] = (n[1], n[2])
        new["nodes"] = nm
        touched = sorted({int(s) for s in res.tx_seg[t0:t0 + len(tx)]})
        w, a = _key_weaves(res.maps, touched, both, pm, d)
        new["weave"] = {**ct["weave"], **w}
        new["_active"] = {**ct["_active"], **a}
        if tx[0][0][0] > ct["lamport_ts"]:  # shared.cljc:179-181
            new["lamport_ts"] = tx[0][0][0]
        out.append(new)
    return out


def map_weave_node(ct, node=None, more=None):
    """A weave-fn for ``insert`` / ``append`` that weaves incrementally
    (map.cljc:29-45): ``ct`` holds the tx in ::nodes already, its ``weave``
    does not.  Without a node it is the full reweave (``map_weave``)."""
    if node is None:
        return map_weave(ct)
    if node[0] not in ct["nodes"]:
        return ct
    tx = [node] + list(more or [])
    base = dict(ct)
    base["nodes"] = {i: b for i, b in ct["nodes"].items() if all(i != n[0] for n in tx)}
    return insert_maps([(base, node, more)])[0]


def active_node(ct, k):
    """map.cljc:47-59 (computed on the GPU with the weave)."""
    return ct["_active"].get(k, BLANK)


def map_get(ct, k):
    """map.cljc:61-66"""
    n = active_node(ct, k)
    return None if n is BLANK else n[2]


def map_count(ct):
    """map.cljc:68-73"""
    return sum(1 for n in ct["_active"].values() if n is not BLANK)


def map_assoc(ct, k, v, weave_fn=None):
    """map.cljc:75-81.  weave_fn: the weave-fn ``append`` uses (default: the full
    reweave, ``map_weave``; ``map_weave_node`` weaves the one node in)."""
    if v != map_get(ct, k):
        return append(weave_fn or map_weave, ct, k, v)
    return ct


def map_dissoc(ct, k, weave_fn=None):
    """map.cljc:83-89.  weave_fn: as in ``map_assoc``."""
    v = map_get(ct, k)
    if v is not None and v is not False:
        return append(weave_fn or map_weave, ct, k, HIDE)
    return ct


def causal_map_to_edn(ct):
    """map.cljc:94-103: the active value of every key, nested causal values
    materialised (s/causal->edn, map.cljc:101)."""
    return {n[1]: causal_to_edn(n[2]) for n in ct["_active"].values() if n is not BLANK}


def maps_to_edn(cts):
    """causal-map->edn (map.cljc:94-103) of many map cts, woven and rendered on
    the GPU (cw_weave_maps, then cw_render_maps): per ct the dict
    causal_map_to_edn gives after a reweave, its keys in ascending key-token
    order (the reference's reduce-kv order over a hash map is unspecified)."""
    docs = [[(i, b[0], b[1]) for i, b in ct["nodes"].items()] for ct in cts]
    pm = pack.pack_maps(docs)
    w = weaver()
    res = w.weave_maps(pm.offsets, pm.id_key, pm.cause, pm.cause_is_id, pm.kind, pm.token_bits,
                       pm.layout.key_bits)
    for st in res.status.tolist():
        if st & (abi.STATUS_DUP | abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL):
            raise CauseError(f"map outside the weave's domain (status {st})", {"weave-domain"})
    r = w.render_maps(len(docs), res.seg_coll, res.seg_key, res.seg_active)
    out = []
    for d, nodes in enumerate(docs):
        lo, hi = int(r.offsets[d]), int(r.offsets[d + 1])
        out.append({_seg_key(k, pm, d): causal_to_edn(nodes[s][2])
                    for k, s in zip(r.key[lo:hi].tolist(), r.src[lo:hi].tolist())})
    return out


def causal_map_to_list(ct):
    """map.cljc:105-109"""
    return [n for n in ct["_active"].values() if n is not BLANK]


# ------------------------------------------------ versions, deltas and syncing ----
def _pack_ids(cts, extra_ids=None):
    """The ids of list and map cts alike under one layout (only ids decide what
    cw_version / cw_delta compute); every document gets its own site ranking."""
    docs = [[(i, None, None) for i in ct["nodes"]] for ct in cts]
    return pack.pack_lists(docs, min_site_bits=1, extra_ids=extra_ids)


def versions(cts):
    """The version vector of many cts (lists and maps may be mixed) in ONE GPU
    call (cw_version): per ct a dict {site_id: id}, the newest id of each site,
    ``(first (peek yarn))`` of every yarn of s/spin (shared.cljc:96-108).  The
    root's own yarn ("0") is left out: its only id is the root id, which no weft
    and no delta names."""
    pk = _pack_ids(cts)
    lay = pk.layout
    S = 1 << lay.site_bits
    res = abi_sync.version(weaver(), pk.offsets, pk.id_key, lay)
    out = []
    for d, pd in enumerate(pk.docs):
        row = res.ver[d * S:(d + 1) * S].tolist()
        ids = (_unpack_id(w, lay, pd.site_rank) for w in row if w)
        out.append({i[1]: i for i in ids if i != ROOT_ID})
    return out


def _have_table(pk, vers):
    """A version dict per document of pk as the have table of cw_delta."""
    lay = pk.layout
    S = 1 << lay.site_bits
    have = np.zeros(len(pk.docs) << lay.site_bits, np.uint64)
    for d, (pd, ver) in enumerate(zip(pk.docs, vers)):
        for site, i in ver.items():
            if i != ROOT_ID:
                have[d * S + pd.site_rank[site]] = lay.pack(i[0], pd.site_rank[site], i[2])
    return have


def deltas(items):
    """What a peer lacks, for many (ct, version) items in ONE GPU call
    (cw_delta): ``version`` is the peer's version vector as ``versions`` returns
    it ({site_id: id}; a site it does not name: the peer has nothing of it).
    Per item the nodes ``(id, cause, value)`` of ct whose id is above the peer's
    head of their site, in id order: the complement of what s/weft
    (shared.cljc:268-293) keeps at that version.  Lists and maps may be mixed."""
    cts = [ct for ct, _ in items]
    pk = _pack_ids(cts, extra_ids=[[i for i in v.values() if i != ROOT_ID] for _, v in items])
    have = _have_table(pk, [v for _, v in items])
    res = abi_sync.delta(weaver(), pk.offsets, pk.id_key, None, None, None, pk.layout, have)
    out = []
    for d, (ct, pd) in enumerate(zip(cts, pk.docs)):
        lo, hi = int(res.delta_offsets[d]), int(res.delta_offsets[d + 1])
        order = np.argsort(res.delta_id[lo:hi], kind="stable")
        ids = [pd.nodes[int(s)][0] for s in res.delta_src[lo:hi][order]]
        out.append([(i,) + tuple(ct["nodes"][i]) for i in ids])
    return out


def _sync_deltas(offsets, id_key, cause, kind, cause_is_id, layout):
    """Both replicas of every pair as one batch (documents 2d and 2d + 1): the
    versions of all, then per document the nodes above the OTHER replica's
    heads.  -> the cw_delta result (delta_src: indices into the document)."""
    w = weaver()
    ver = abi_sync.version(w, offsets, id_key, layout).ver
    have = ver.reshape((len(offsets) - 1) // 2, 2, 1 << layout.site_bits)[:, ::-1].reshape(-1)
    return abi_sync.delta(w, offsets, id_key, cause, kind, cause_is_id, layout, have)


def _sync_offsets(da, db):
    """The offsets of the batch in which document 2d is replica 1 of pair d and
    document 2d + 1 replica 2: the arrays of the pairs packed as a + b, split."""
    off2 = np.zeros(2 * len(da) + 1, np.uint64)
    off2[1:] = np.cumsum([n for a, b in zip(da, db) for n in (len(a), len(b))])
    return off2


def _other_side(res, off2):
    """cw_delta's documents with every two neighbours swapped: side b of the
    merge.  -> (offsets, where each side-b node stands in the delta columns,
    its index in the batch the delta was taken of)."""
    do = res.delta_offsets.astype(np.int64)
    D = len(do) - 1
    swap = [d ^ 1 for d in range(D)]
    off_b = np.zeros(D + 1, np.uint64)
    off_b[1:] = np.cumsum([do[k + 1] - do[k] for k in swap])
    at = np.concatenate([np.zeros(0, np.int64)] + [np.arange(do[k], do[k + 1]) for k in swap])
    first = np.repeat(off2[:-1].astype(np.int64), np.diff(do))  # of each delta node's document
    return off_b, at, (first + res.delta_src.astype(np.int64))[at]


def _sync(pairs, both, is_map):
    """sync_lists / sync_maps: the versions of both replicas of every pair, the
    deltas both ways, ONE merge call in which document 2d is replica 1 with
    replica 2's delta and document 2d + 1 the reverse."""
    for ct1, ct2 in pairs:
        if ct1["type"] != ct2["type"]:
            raise CauseError("Causal type missmatch. Merge not allowed.", {"type-missmatch"})
        if ct1["uuid"] != ct2["uuid"]:
            raise CauseError("Causal UUID missmatch. Merge not allowed.", {"uuid-missmatch"})
    da = [[(i, b[0], b[1]) for i, b in ct1["nodes"].items()] for ct1, _ in pairs]
    db = [[(i, b[0], b[1]) for i, b in ct2["nodes"].items()] for _, ct2 in pairs]
    both_sides = [a + b for a, b in zip(da, db)]  # one site ranking (and key-token table) per pair
    if is_map:
        pk = pack.pack_maps(both_sides, min_site_bits=1)
        nodes = [n for d in pk.docs for n in d]
        cols = (pk.id_key, pk.cause, pk.cause_is_id, pk.kind)
        res = _sync_deltas((off2 := _sync_offsets(da, db)), pk.id_key, pk.cause, pk.kind, pk.cause_is_id, pk.layout)
        gathered = (res.delta_id, res.delta_cause, res.delta_cause_is_id, res.delta_kind)
    else:
        pk = pack.pack_lists(both_sides, min_site_bits=1)
        nodes = [n for d in pk.docs for n in d.nodes]
        cols = (pk.id_key, pk.cause_key, pk.kind)
        res = _sync_deltas((off2 := _sync_offsets(da, db)), pk.id_key, pk.cause_key, pk.kind, None, pk.layout)
        gathered = (res.delta_id, res.delta_cause, res.delta_kind)
    off_b, at, ib = _other_side(res, off2)
    tok = _Tokens()
    vals = np.array([tok(n[2]) for n in nodes], np.uint64)
    side_a = (off2,) + cols + (vals,)
    side_b = (off_b,) + tuple(c[at] for c in gathered) + (vals[ib],)
    firsts = [ct for pair in pairs for ct in pair]
    la = [x for a, b in zip(da, db) for x in (a, b)]
    lb = [[nodes[int(g)] for g in ib[int(off_b[k]):int(off_b[k + 1])]] for k in range(2 * len(pairs))]
    if is_map:
        m = weaver().merge_maps(side_a, side_b, pk.token_bits, pk.layout.key_bits)
        out = _merged_maps(m, firsts, la, lb, pk, [k // 2 for k in range(2 * len(pairs))])
    else:
        m = weaver().merge_lists(side_a, side_b, pk.layout)
        out = _merged_lists(m, firsts, la, lb)
    return [(out[2 * d], out[2 * d + 1]) for d in range(len(pairs))] if both else out[::2]


def sync_lists(pairs, both=False):
    """s/merge-trees (shared.cljc:300-314) for many (ct1, ct2) list pairs by
    way of the diff its own comment asks for (shared.cljc:295-299): both
    replicas of every pair packed under one layout, the versions of both
    (cw_version), the deltas both ways (cw_delta), and each replica merged with
    only the other's delta (ONE cw_merge_lists call).  Per pair the merged ct,
    the value ``merge_lists(pairs)`` returns; both=True: (ct1 merged, ct2
    merged).

    Precondition: each replica holds a PREFIX of every yarn -- if it has a node
    of a site it has every older node of that site.  That is what s/insert's
    cause-must-exist check (shared.cljc:151-184) and a Lamport clock give
    replicas that only ever append and merge.  Then the nodes above the other
    side's heads are exactly the nodes it lacks.  For arbitrary node bags
    ``merge_lists`` is the call to use."""
    return _sync(pairs, both, False)


def sync_maps(pairs, both=False):
    """CausalMap's causal-merge (map.cljc:248-249) for many (ct1, ct2) map pairs
    by way of versions and deltas, as ``sync_lists``: ONE cw_version, ONE
    cw_delta and ONE cw_merge_maps call in which each replica meets only the
    other's delta.  Per pair the merged ct, the value ``merge_maps(pairs)``
    returns; both=True: (ct1 merged, ct2 merged).

    Precondition: as ``sync_lists``: each replica holds a prefix of every yarn
    (s/insert's cause-must-exist and a Lamport clock give that); for arbitrary
    node bags ``merge_maps`` is the call to use."""
    return _sync(pairs, both, True)
