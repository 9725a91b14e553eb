"""Host mirror of CausalBase materialisation, with the
weaves and the history sort on the MI355X.

A causal base (base/core.cljc) keeps nested collections flat: every nested
list or map is its own causal collection and the parent holds a ref keyword
``:causal.collection.ref/<uuid>``.  What touches node data here goes through the
C ABI in batches:

  * ``cb_to_edn`` (base/core.cljc:92-96, with the ref resolution of :83-90):
    every collection is rewoven in ONE cw_weave_lists call (all lists) and ONE
    cw_weave_maps call (all maps), then the refs are resolved on the host;
  * ``history`` (the ``::history`` sorted log, :107-115): the reverse paths
    ``[id uuid]`` of every insertion sorted by id with cw_sort_keys (the
    reference keeps the vector sorted by one binary-search insertion each);
  * ``invert_`` (:322-343), what ``undo_``, ``redo_`` and ``reset_`` end in:
    every collection of the base (of many bases: ``invert_bases``) is packed
    into ONE cw_invert call, which returns the inverting transaction; its nodes
    are inserted like any other tx.  ``subhis``, ``get_next_tx_id`` and the undo
    markers (:272-311, :354-409) are host logic;
  * ``bases_to_edn``: ``cb_to_edn`` for many bases at once, the refs resolved on
    the device too: every list of every base in ONE cw_weave_lists and ONE
    cw_render_lists call, every map in ONE cw_weave_maps and ONE cw_render_maps
    call, both rendered with the ref column as the value, and ONE
    cw_render_bases call that turns the entry table into a depth-first token
    stream per base.  The host rebuilds the nested values with one stack pass;
  * ``transact_bases``: ``transact-`` (:100-252) for many bases at once: the
    values of every transaction flattened into token streams on the host
    (``tokenize_tx``: one type test per tx-part, the three validation errors)
    and ONE cw_transact call that assigns the tx-index, allocates a collection
    per nested list or map, chains the lists and splices the strings.  The host
    draws the uuids and applies the nodes run by run through ``_insert``.

``transact_`` (with ``flatten_value``, ``map_to_nodes``, ``list_to_nodes``,
:117-268) is the same bookkeeping for one base as a host recursion, one node at
a time; it follows the reference clause by clause and is what ``transact_bases``
is tested against.  Both defer the weave: collections are woven when
materialised (insertion in any causal order equals the full
reweave), with the insert-time checks of s/insert kept.
"""
from __future__ import annotations

import bisect
import random

import numpy as np

from . import abi, abi_invert, abi_render_bases as RB, abi_transact, causal as C, pack

REF_NS = "causal.collection.ref"      # base/core.cljc:57


class Char(str):
    """A Clojure character (``\\a``): one element of a string woven as a list."""

    __slots__ = ()

    def __repr__(self):
        return "\\" + str.__str__(self)


def _no_weave(ct, node=None, more=None):
    return ct


def new_cb(rng=random):
    """base/core.cljc:39-53"""
    return {"lamport_ts": 1, "uuid": C._uid(rng, 21), "site_id": C.new_site_id(rng),
            "history": [], "root_uuid": None, "collections": {}, "_rng": rng,
            "first_undo_lamport_ts": None, "last_undo_lamport_ts": None, "last_redo_lamport_ts": None}


def uuid_to_ref(uuid):
    return C.Keyword(REF_NS, uuid)      # :59-60


def is_ref(v):
    return isinstance(v, C.Keyword) and v.ns == REF_NS     # :65-66


def ref_to_uuid(ref):
    return ref.name                     # :68-69


def _is_map(v):
    return isinstance(v, dict)


def _seqable(v):
    """clojure.core/seqable? for the values a transaction carries (nil is
    seqable; a character is not)."""
    if isinstance(v, Char):
        return False
    return v is None or isinstance(v, (str, list, tuple))


def new_node(cb, tx_index, cause, value):
    """:100-105 -> (tx_index + 1, node)"""
    return tx_index + 1, ((cb["lamport_ts"], cb["site_id"], tx_index or 0), cause, value)


def _insert(cb, uuid, nodes):
    """:107-115 -- proto/insert into the collection (s/insert's checks; the weave
    is deferred to materialisation) and the reverse paths into the history."""
    if not nodes:
        return cb
    cb = dict(cb)
    cols = dict(cb["collections"])
    cols[uuid] = C.insert(_no_weave, cols[uuid], nodes[0], nodes[1:])
    cols[uuid]["_dirty"] = True
    cb["collections"] = cols
    cb["history"] = cb["history"] + [(n[0], uuid) for n in nodes]
    return cb


def add_collection_for(cb, value, is_root=False):
    """:117-126 -> (cb, uuid or None)"""
    rng = cb.get("_rng", random)
    if _is_map(value):
        ct = C.new_map_ct(site_id=cb["site_id"], rng=rng)
    elif _seqable(value):
        ct = C.new_list_ct(site_id=cb["site_id"], rng=rng)
    else:
        return cb, None
    cb = dict(cb)
    cb["collections"] = dict(cb["collections"], **{ct["uuid"]: ct})
    if is_root:
        cb["root_uuid"] = ct["uuid"]
    return cb, ct["uuid"]


def map_to_nodes(cb, tx_index, m):
    """:130-138 -> (cb, tx_index, nodes)"""
    nodes = []
    for k, v in m.items():
        cb, tx_index, fv = flatten_value(cb, tx_index, v, preserve_strings=True)
        tx_index, node = new_node(cb, tx_index, k, fv)
        nodes.append(node)
    return cb, tx_index, nodes


def _elements(value, is_string):
    if value is None:
        return []
    if is_string:
        return [Char(ch) for ch in value]
    return list(value)


def list_to_nodes(cb, tx_index, value, cause=None):
    """:140-156 -> (cb, tx_index, nodes, last_node_id).  A string in a list of
    values is spliced into the same list, char by char."""
    is_string = isinstance(value, str) and not isinstance(value, Char)
    nodes = []
    cause = cause if cause is not None else C.ROOT_ID
    for v in _elements(value, is_string):
        if not is_string and isinstance(v, str) and not isinstance(v, Char):
            cb, tx_index, more, cause = list_to_nodes(cb, tx_index, v, cause)
            nodes += more
        else:
            cb, tx_index, fv = flatten_value(cb, tx_index, v, preserve_strings=is_string)
            tx_index, node = new_node(cb, tx_index, cause, fv)
            nodes.append(node)
            cause = node[0]
    return cb, tx_index, nodes, cause


def _flatten_collection(cb, tx_index, value, node_fn):
    """:158-164"""
    cb, uuid = add_collection_for(cb, value)
    cb, tx_index, nodes = node_fn(cb, tx_index, value)[:3]
    cb = _insert(cb, uuid, nodes)
    return cb, tx_index, uuid_to_ref(uuid)


def flatten_value(cb, tx_index, value, preserve_strings=False):
    """:166-172 -> (cb, tx_index, flat value)"""
    if preserve_strings and isinstance(value, str) and not isinstance(value, Char):
        return cb, tx_index, value
    if _is_map(value):
        return _flatten_collection(cb, tx_index, value, map_to_nodes)
    if _seqable(value):
        return _flatten_collection(cb, tx_index, value, list_to_nodes)
    return cb, tx_index, value


def _value_to_nodes(cb, tx_index, cause, value):
    """:174-183"""
    if _is_map(value):
        return map_to_nodes(cb, tx_index, value)
    if _seqable(value):
        return list_to_nodes(cb, tx_index, value, cause)[:3]
    tx_index, node = new_node(cb, tx_index, cause, value)
    return cb, tx_index, [node]


def _handle_value(cb, uuid, cause, value, tx_index):
    """:185-205"""
    ct = cb["collections"][uuid]
    merge = (cause is None and _is_map(value) and ct["type"] == "map") or \
        (not _is_map(value) and _seqable(value) and ct["type"] == "list")
    if merge:
        cb, tx_index, nodes = _value_to_nodes(cb, tx_index, cause, value)
        return _insert(cb, uuid, nodes), tx_index
    cb, tx_index, fv = flatten_value(cb, tx_index, value, preserve_strings=ct["type"] == "map")
    tx_index, node = new_node(cb, tx_index, cause, fv)
    return _insert(cb, uuid, [node]), tx_index


def transact_(cb, tx):
    """:238-268 -- tx = [(uuid, cause, value), ...]; uuid None makes a root."""
    tx_index = 0
    for uuid, cause, value in tx:
        if uuid is not None and cb["root_uuid"] is None:               # :219-221
            raise C.CauseError("Please transact a root collection first by setting uuid "
                               "and cause to nil", set())
        if uuid is not None and uuid not in cb["collections"]:          # :222-224
            raise C.CauseError("Collection with provided uuid not found", set())
        if uuid is None and not (_is_map(value) or isinstance(value, (list, tuple))):
            raise C.CauseError("Root node must satisfy the coll? predicate", set())
        if uuid is None:                                                # :207-212
            cb, uuid = add_collection_for(cb, value, is_root=True)
        cb, tx_index = _handle_value(cb, uuid, cause, value, tx_index)
    return _end_tx(cb)


def _end_tx(cb):
    """:249-252 -- the lamport-ts bumped, the undo markers cleared."""
    cb = dict(cb)
    cb["lamport_ts"] = cb["lamport_ts"] + 1
    cb["first_undo_lamport_ts"] = cb["last_undo_lamport_ts"] = cb["last_redo_lamport_ts"] = None
    return cb


# ------------------------------------------- transact- of many bases ----
def _gpu_transact(*args):
    return abi_transact.transact(C.weaver(), *args)


def _is_string(v):
    return isinstance(v, str) and not isinstance(v, Char)


def tokenize_tx(cb, tx):
    """The value walk of transact- (:185-252) as the token stream cw_transact
    takes: one type test per tx-part (merge-value-into-parent-collection?,
    :184-190), no tx-index, no collection, no chaining.  -> [(kind, uuid or
    length, cause, value, parent)]: the uuid of a PART's collection, the length
    of a STR; the cause as the tx gives it (a part's, or a map child's key), with
    ``C.ROOT_ID`` where list-to-nodes starts from the root; parent: the token that
    opens the enclosing group (a CLOSE's: its own opener), -1 for a part.  The
    three validate-tx-part errors are raised as ``transact_`` raises them."""
    T = abi_transact
    toks = []

    def child(v, key, parent):
        if _is_string(v):
            toks.append((T.TX_STR, len(v), key, v, parent))
        elif _is_map(v) or _seqable(v):
            me = len(toks)
            toks.append((T.TX_OPEN_MAP if _is_map(v) else T.TX_OPEN_LIST, 0, key, None, parent))
            contents(v, me)
            toks.append((T.TX_CLOSE, 0, None, None, me))
        else:
            toks.append((T.TX_LEAF, 0, key, v, parent))

    def contents(v, parent):
        if _is_map(v):
            for k, x in v.items():
                child(x, k, parent)
        else:
            for x in _elements(v, False):
                child(x, None, parent)

    has_root = cb["root_uuid"] is not None
    for uuid, cause, value in tx:
        if uuid is not None and not has_root:                          # :219-221
            raise C.CauseError("Please transact a root collection first by setting uuid "
                               "and cause to nil", set())
        if uuid is not None and uuid not in cb["collections"]:          # :222-224
            raise C.CauseError("Collection with provided uuid not found", set())
        if uuid is None and not (_is_map(value) or isinstance(value, (list, tuple))):
            raise C.CauseError("Root node must satisfy the coll? predicate", set())
        me = len(toks)
        if uuid is None:                                                # :207-212
            kind, to_map, has_root = (T.TX_ROOT_MAP if _is_map(value) else T.TX_ROOT_LIST), _is_map(value), True
        else:
            kind, to_map = T.TX_PART, cb["collections"][uuid]["type"] == "map"
        merge = (cause is None and _is_map(value) and to_map) or \
            (not _is_map(value) and _seqable(value) and not to_map)
        if merge and not to_map and cause is None:
            cause = C.ROOT_ID                                           # list-to-nodes (:142)
        toks.append((kind, uuid, cause, None, -1))
        if not merge:
            child(value, cause, me)
        elif _is_string(value):
            toks.append((T.TX_STR, len(value), None, value, me))
        else:
            contents(value, me)
        toks.append((T.TX_CLOSE, 0, None, None, me))
    return toks


def transact_bases(cbs, txs, transact_fn=None):
    """``[transact_(cb, tx) for cb, tx in zip(cbs, txs)]`` with the nodes of every
    base made by ONE cw_transact call: the token streams of ``tokenize_tx`` in,
    the node columns out; the uuids of the new collections are drawn from each
    base's rng in creation order, the nodes go through ``_insert`` run by run in
    the order of the reference's inserts (a group is inserted when it closes),
    and ``_end_tx`` ends the transaction.  transact_fn: the call (default: the
    GPU), taking abi_transact.transact's arguments after the Weaver."""
    T = abi_transact
    cbs = list(cbs)
    streams = [tokenize_tx(cb, tx) for cb, tx in zip(cbs, txs)]
    # one key layout and one site ranking for every id the call sees or makes
    ids = [C.ROOT_ID] + [(cb["lamport_ts"], cb["site_id"], 0) for cb in cbs]
    ids += [t[2] for s in streams for t in s if pack.valid_id(t[2])]
    sites = sorted({i[1] for i in ids}, key=pack.java_str_key)
    rank = {s: r for r, s in enumerate(sites)}
    most = max([sum(t[1] if t[0] == T.TX_STR else 1 for t in s) for s in streams] + [i[2] + 1 for i in ids])
    lay = pack.KeyLayout(max(1, max(i[0] for i in ids).bit_length()), max(1, (len(sites) - 1).bit_length()),
                         max(1, (most - 1).bit_length()))
    if lay.key_bits > 63:
        raise pack.KeyRangeError(f"ids need {lay.key_bits} bits (> 63)")
    pk = lambda i: 0 if i == C.ROOT_ID else lay.pack(i[0], rank[i[1]], i[2])
    keys = {}
    doff, toff, ism, ntx = [0], [0], [], []
    kind, arg, cause, cii, vkind = [], [], [], [], []
    for cb, s in zip(cbs, streams):
        index = {u: doff[-1] + k for k, u in enumerate(cb["collections"])}
        ism += [ct["type"] == "map" for ct in cb["collections"].values()]
        ntx.append(lay.pack(cb["lamport_ts"], rank[cb["site_id"]], 0))
        for k, a, c, v, _ in s:
            kind.append(k)
            arg.append(index[a] if k == T.TX_PART else a if k == T.TX_STR else 0)
            if pack.valid_id(c):
                cause.append(pk(c)), cii.append(1)
            elif c is None:      # the nil key of a map; nil as a list part's cause
                cause.append(pack.NIL), cii.append(2)
            elif pack.is_id(c):  # (an id that is not a valid one: no node has it)
                cause.append(pack.NON_ID_CAUSE), cii.append(1)
            else:
                cause.append(keys.setdefault(c, len(keys))), cii.append(0)
            vkind.append(pack.kind_of(v) if k == T.TX_LEAF else 0)
        doff.append(len(ism))
        toff.append(len(kind))
    res = (transact_fn or _gpu_transact)(np.array(doff, np.uint64), np.array(ism, np.uint8), lay,
                                         np.array(ntx, np.uint64), np.array(toff, np.uint64),
                                         np.array(kind, np.uint8), np.array(arg, np.uint32),
                                         np.array(cause, np.uint64), np.array(cii, np.uint8),
                                         np.array(vkind, np.uint8))
    if np.any(res.base_status & abi.STATUS_KEY_RANGE):
        raise C.CauseError("the transaction does not fit the key layout", {"key-range"})
    if np.any(res.base_status):
        raise C.CauseError("tokenize_tx made a stream that cw_transact refuses", {"internal"})
    D, no = len(ism), res.node_offsets.tolist()
    nid, nca, src, sub, ref, run, nkd = (x.tolist() for x in (res.node_id, res.node_cause, res.node_src, res.node_sub,
                                                               res.node_ref, res.node_run, res.node_kind))
    out = []
    for g, (cb, s) in enumerate(zip(cbs, streams)):
        t0, c0, c1 = toff[g], int(res.base_new_offsets[g]), int(res.base_new_offsets[g + 1])
        uuids = list(cb["collections"])
        for c in range(c0, c1):      # add-collection-of-this-values-type-to-cb (:117-126), in creation order
            k = s[int(res.new_open[c]) - t0][0]
            cb, u = add_collection_for(cb, {} if k in (T.TX_OPEN_MAP, T.TX_ROOT_MAP) else [],
                                       is_root=k in (T.TX_ROOT_MAP, T.TX_ROOT_LIST))
            uuids.append(u)
        doc_uuid = lambda d: uuids[d - doff[g]] if d < D else uuids[len(uuids) - (c1 - c0) + (d - D - c0)]
        runs = []                    # (the token that closes the run's group, uuid, nodes)
        for d in list(range(doff[g], doff[g + 1])) + list(range(D + c0, D + c1)):
            for j in range(no[d], no[d + 1]):
                if nkd[j] & pack.KIND_ROOT:
                    continue         # new-causal-list made the root
                tok = s[src[j] - t0]
                made_by = tok[4] if tok[0] == T.TX_CLOSE else src[j] - t0   # a ref: the OPEN_* that its CLOSE closes
                k, a, c, v, parent = s[made_by]
                grp = s[parent]
                if run[j]:
                    runs.append((parent, doc_uuid(d), []))
                in_map = grp[0] in (T.TX_OPEN_MAP, T.TX_ROOT_MAP) or \
                    (grp[0] == T.TX_PART and cb["collections"][grp[1]]["type"] == "map")
                if in_map:
                    node_cause = c
                elif run[j]:         # the group's initial cause
                    node_cause = grp[2] if grp[0] in (T.TX_PART, T.TX_ROOT_LIST) else C.ROOT_ID
                else:                # chained: a node of this transaction
                    node_cause = (cb["lamport_ts"], cb["site_id"], nca[j] - int(ntx[g]))
                value = uuid_to_ref(doc_uuid(ref[j])) if k in (T.TX_OPEN_LIST, T.TX_OPEN_MAP) else \
                    v if k == T.TX_LEAF or in_map else Char(v[sub[j]])
                runs[-1][2].append(((cb["lamport_ts"], cb["site_id"], nid[j] - int(ntx[g])), node_cause, value))
        close_of = {t[4]: i for i, t in enumerate(s) if t[0] == T.TX_CLOSE}
        for _, u, nodes in sorted(runs, key=lambda r: close_of[r[0]]):
            cb = _insert(cb, u, nodes)
        out.append(_end_tx(cb))
    return out


# ------------------------------------------------------------- history ----
def _id_key(i):
    return (i[0], pack.java_str_key(i[1]), i[2])       # util.cljc:4-10


def _sorted_history(cb):
    """::history is kept sorted by id (:107-115); local transactions append in
    that order already, merged ones may not."""
    return sorted(cb["history"], key=lambda rp: _id_key(rp[0]))


def tx_id_indexes(cb, tx_id):
    """:272-289 -> (tx_start_i, tx_end_i) of the reverse paths of one tx-id in
    the sorted history, (None, None) when it has none."""
    if tx_id is None:
        return None, None
    hist = _sorted_history(cb)
    keys = [_id_key(rp[0]) for rp in hist]
    start = bisect.bisect_left(keys, _id_key(tuple(tx_id) + (0,)))
    if start == len(hist) or hist[start][0] != tuple(tx_id) + (0,):
        return None, None
    end = start
    while end + 1 < len(hist) and hist[end + 1][0][:2] == tuple(tx_id):
        end += 1
    return start, end


_SAME = object()


def subhis(cb, start_tx_id, end_tx_id=_SAME):
    """:291-311 -- the history between two tx-ids, inclusive; None is the start
    or the end; one argument slices out one tx-id."""
    if end_tx_id is _SAME:
        end_tx_id = start_tx_id
    hist = _sorted_history(cb)
    start_i, end_i = tx_id_indexes(cb, start_tx_id)
    if start_tx_id != end_tx_id:
        _, end_i = tx_id_indexes(cb, end_tx_id)
    if (start_tx_id is not None and start_i is None) or (end_tx_id is not None and end_i is None):
        return []
    return hist[start_i or 0:end_i + 1] if end_i is not None else hist[start_i or 0:]


def get_next_tx_id(cb, last_undo_or_redo_ts):
    """:354-369 -- the tx-id next in line to be undone or redone."""
    remaining = subhis(cb, None, (last_undo_or_redo_ts - 1, cb["site_id"])) if last_undo_or_redo_ts \
        else _sorted_history(cb)
    for (ts, site, _), _ in reversed(remaining):
        if site == cb["site_id"]:
            return (ts, site)
    return None


def invert_path(path):
    """:313-320 -- path = {"uuid": ..., "node": (id, cause, value)} -> tx-part."""
    uuid, (nid, cause, value) = path["uuid"], path["node"]
    if value == C.HIDE or value == C.H_HIDE:
        return (uuid, cause, C.H_SHOW)
    if value == C.H_SHOW:
        return (uuid, cause, C.H_HIDE)
    return (uuid, nid, C.H_HIDE)


def _gpu_invert(*args):
    return abi_invert.invert(C.weaver(), *args)


def _selection(cb, history_slice):
    """A slice as cw_invert takes it: (lo id, hi id, sites).  subhis filtered by
    site is every reverse path of an id range with those sites; any other
    subset of the history is refused."""
    ids = [i for i, _ in history_slice]
    lo, hi = min(ids, key=_id_key), max(ids, key=_id_key)
    sites = {i[1] for i in ids}
    inside = sum(1 for i, _ in cb["history"]
                 if _id_key(lo) <= _id_key(i) <= _id_key(hi) and i[1] in sites)
    if inside != len(set(ids)):
        raise ValueError("history_slice is not a site-filtered range of the history")
    return lo, hi, sites


def _pack_bases(cbs, sels):
    """Every collection of every base as one cw_invert batch: lists and maps
    together, one key layout and one site ranking, ref_doc from the ref values."""
    ids = [C.ROOT_ID]
    for cb in cbs:
        ids.append((cb["lamport_ts"], cb["site_id"], 0))
        for ct in cb["collections"].values():
            for nid, (cause, _) in ct["nodes"].items():
                ids.append(nid)
                if pack.valid_id(cause):
                    ids.append(cause)
    sites = sorted({i[1] for i in ids}, key=pack.java_str_key)
    rank = {s: r for r, s in enumerate(sites)}
    most = max([len(cb["history"]) for cb in cbs] + [i[2] + 1 for i in ids])
    lay = pack.KeyLayout(max(1, max(i[0] for i in ids).bit_length()), max(1, (len(sites) - 1).bit_length()),
                         max(1, (most - 1).bit_length()))
    if lay.key_bits > 63:
        raise pack.KeyRangeError(f"ids need {lay.key_bits} bits (> 63)")
    pk = lambda i: 0 if i == C.ROOT_ID else lay.pack(i[0], rank[i[1]], i[2])
    tok = {}
    off, boff, docs = [0], [0], []
    idk, ca, ci, kd, rf = [], [], [], [], []
    for cb in cbs:
        uuids = list(cb["collections"])
        index = {u: len(docs) + k for k, u in enumerate(uuids)}
        for u in uuids:
            ct = cb["collections"][u]
            nodes = [(nid, cause, value) for nid, (cause, value) in ct["nodes"].items()]
            docs.append((u, nodes))
            for nid, cause, value in nodes:
                idk.append(pk(nid))
                k = pack.kind_of(value)
                if ct["type"] == "list":
                    if nid == C.ROOT_ID and cause is None and value is None:
                        k |= pack.KIND_ROOT
                    ca.append(pack.NIL if cause is None else pk(cause) if pack.is_id(cause) else pack.NON_ID_CAUSE)
                    ci.append(1)
                elif pack.valid_id(cause):
                    ca.append(pk(cause))
                    ci.append(1)
                elif cause is None:
                    ca.append(0)
                    ci.append(2)
                else:
                    ca.append(tok.setdefault(cause, len(tok)))
                    ci.append(0)
                kd.append(k)
                rf.append(index.get(ref_to_uuid(value), abi_invert.U32_MAX) if is_ref(value) else abi_invert.U32_MAX)
            off.append(len(idk))
        boff.append(len(docs))
    W, G = abi_invert.mask_words(lay.site_bits), len(cbs)
    lo_a, hi_a = np.ones(G, np.uint64), np.zeros(G, np.uint64)
    masks, ntx = np.zeros(G * W, np.uint64), np.zeros(G, np.uint64)
    for g, (cb, sel) in enumerate(zip(cbs, sels)):
        ntx[g] = lay.pack(cb["lamport_ts"], rank[cb["site_id"]], 0)
        if sel is None:          # an empty slice: lo > hi selects nothing
            continue
        lo_a[g], hi_a[g] = pk(sel[0]), pk(sel[1])
        for s in sel[2]:
            masks[g * W + rank[s] // 64] |= np.uint64(1 << (rank[s] % 64))
    args = (np.array(off, np.uint64), np.array(idk, np.uint64), np.array(ca, np.uint64), np.array(kd, np.uint8),
            np.array(ci, np.uint8), np.array(rf, np.uint32), lay, np.array(boff, np.uint64), lo_a, hi_a, masks,
            ntx)
    return args, docs


def invert_bases(cbs, slices, invert_fn=None):
    """invert- (:322-343) for many bases in ONE cw_invert call: every node of
    each slice becomes an inverting tx-part, one part per [uuid cause], nested
    collections that are about to be hidden dropped, the rest transacted at the
    base's lamport-ts.  invert_fn: the call (default: the GPU), taking
    abi_invert.invert's arguments after the Weaver."""
    sels = [_selection(cb, sl) if sl else None for cb, sl in zip(cbs, slices)]
    args, docs = _pack_bases(cbs, sels)
    res = (invert_fn or _gpu_invert)(*args)
    if np.any(res.status):
        raise C.CauseError("the inverting tx does not fit the key layout", {"key-range"})
    boff, po, ntx = args[7], res.part_offsets, args[11]
    out = []
    for g, cb in enumerate(cbs):
        parts = []
        for d in range(int(boff[g]), int(boff[g + 1])):
            uuid, nodes = docs[d]
            for j in range(int(po[d]), int(po[d + 1])):
                nid, cause, value = nodes[int(res.inv_src[j])]
                special = pack.kind_of(value) != pack.KIND_NORMAL
                kw = C.H_HIDE if int(res.inv_kind[j]) == pack.KIND_HHIDE else C.H_SHOW
                parts.append((int(res.inv_id[j]) - int(ntx[g]), uuid, cause if special else nid, kw))
        for tx_index, uuid, cause, kw in sorted(parts, key=lambda p: p[0]):   # transact- (:232-252)
            cb = _insert(cb, uuid, [new_node(cb, tx_index, cause, kw)[1]])
        out.append(_end_tx(cb))
    return out


def invert_(cb, history_slice, invert_fn=None):
    """:322-343"""
    return invert_bases([cb], [history_slice], invert_fn)[0]


def reset_(cb, tx_id, site_ids, invert_fn=None):
    """:345-352 -- every transaction of ``site_ids`` back to ``tx_id`` undone."""
    sites = set(site_ids)
    return invert_(cb, [rp for rp in subhis(cb, tx_id, None) if rp[0][1] in sites], invert_fn)


def _local(cb, tx_id):
    return [rp for rp in subhis(cb, tx_id) if rp[0][1] == cb["site_id"]]


def undo_(cb, invert_fn=None):
    """:375-390 -- the next transaction of the undo stack undone."""
    next_id = get_next_tx_id(cb, cb.get("last_undo_lamport_ts"))
    if next_id is None:
        return cb
    first = cb.get("first_undo_lamport_ts") or next_id[0]
    cb = invert_(cb, _local(cb, next_id), invert_fn)
    cb.update(first_undo_lamport_ts=first, last_undo_lamport_ts=next_id[0], last_redo_lamport_ts=None)
    return cb


def redo_(cb, invert_fn=None):
    """:392-409 -- the last undone transaction done again, never past the first undo."""
    next_id = get_next_tx_id(cb, cb.get("last_redo_lamport_ts"))
    first, last = cb.get("first_undo_lamport_ts"), cb.get("last_undo_lamport_ts")
    if first is None or next_id is None or next_id[0] <= first:
        return cb
    cb = invert_(cb, _local(cb, next_id), invert_fn)
    cb.update(first_undo_lamport_ts=first, last_undo_lamport_ts=last, last_redo_lamport_ts=next_id[0])
    return cb


# ------------------------------------------------------------ on the GPU ----
def weave_all(cb):
    """Reweave every collection changed since the last call: all lists in one
    cw_weave_lists call, all maps in one cw_weave_maps call."""
    cols = cb["collections"]
    lists = [u for u, ct in cols.items() if ct["type"] == "list" and ct.get("_dirty")]
    maps = [u for u, ct in cols.items() if ct["type"] == "map" and ct.get("_dirty")]
    if not lists and not maps:
        return cb
    new = dict(cols)
    if lists:
        for u, ct in zip(lists, C.weave_lists([cols[u] for u in lists])):
            new[u] = dict(ct, _dirty=False)
    if maps:
        for u, ct in zip(maps, C.weave_maps([cols[u] for u in maps])):
            new[u] = dict(ct, _dirty=False)
    out = dict(cb)
    out["collections"] = new
    return out


def get_collection(cb, uuid_or_ref=None):
    """:72-79"""
    key = uuid_or_ref if uuid_or_ref is not None else cb["root_uuid"]
    if key is None:
        return None
    return cb["collections"].get(ref_to_uuid(key) if is_ref(key) else key)


def _edn(cb, v, seen):
    """s/causal->edn (shared.cljc:320-328) with the ref resolution of
    Keyword's causal->edn (base/core.cljc:83-90); a ref met twice on one path
    raises instead of recursing forever (the reference's TODO at :88)."""
    if is_ref(v):
        u = ref_to_uuid(v)
        if u in seen:
            raise C.CauseError("collections reference each other", {"ref-cycle"})
        ct = cb["collections"].get(u)
        return None if ct is None else _ct_edn(cb, ct, seen | {u})
    return v


def _ct_edn(cb, ct, seen):
    if ct["type"] == "list":             # list.cljc:57-66
        return [_edn(cb, n[2], seen) for n in C.causal_list_to_list(ct)]
    return {n[1]: _edn(cb, n[2], seen) for n in C.causal_map_to_list(ct)}   # map.cljc:94-103


def cb_to_edn(cb):
    """base/core.cljc:92-96 -> (edn, cb with every collection woven)."""
    cb = weave_all(cb)
    root = get_collection(cb)
    if root is None:
        return None, cb
    return _ct_edn(cb, root, {root["uuid"]}), cb


# ---------------------------------------------------- cb->edn of many bases ----
def _gpu_render_bases(*args):
    return RB.render_bases(C.weaver(), *args)


def _collect_docs(cbs):
    """The documents of a batch of bases, lists first, then maps: [(base, uuid,
    nodes)], the number of lists, and each base's root document (D: none)."""
    picked = {"list": [], "map": []}
    for g, cb in enumerate(cbs):
        for u, ct in cb["collections"].items():
            picked[ct["type"]].append((g, u, [(i, b[0], b[1]) for i, b in ct["nodes"].items()]))
    docs = picked["list"] + picked["map"]
    index = {(g, u): d for d, (g, u, _) in enumerate(docs)}
    roots = np.array([index.get((g, cb["root_uuid"]), len(docs)) for g, cb in enumerate(cbs)], np.uint32)
    return docs, len(picked["list"]), index, roots


def _ref_column(docs, index):
    """ref_doc per node, in document order: U32_MAX for a plain value, the
    batch-wide document of a ref's collection, n_docs for a ref to a collection
    the base does not hold (the reference's get-in gives nil)."""
    D = len(docs)
    return np.array([index.get((g, ref_to_uuid(n[2])), D) if is_ref(n[2]) else RB.U32_MAX
                     for g, _, nodes in docs for n in nodes], np.uint32)


def _gpu_entries(docs, n_lists, refs):
    """The entry table of the documents, woven and rendered on the GPU with the
    ref column as the value: (ent_offsets, ent_ref, ent_src, ent_key), ent_key a
    list with the map key of every map entry (None for a list entry)."""
    w = C.weaver()
    lists, maps = [nodes for _, _, nodes in docs[:n_lists]], [nodes for _, _, nodes in docs[n_lists:]]
    n_list_nodes = sum(len(x) for x in lists)
    off, ref, src, key = [np.zeros(1, np.uint64)], [], [], []
    if lists:
        try:
            b = pack.pack_lists(lists)
            res = w.weave_lists(b.offsets, b.id_key, b.cause_key, b.kind, b.layout, yarns=False)
        except pack.KeyRangeError:  # ids over 63 bits: the K128 layout
            b = pack.pack_lists_k128(lists)
            res = w.weave_lists_k128(b.offsets, b.id_key, b.cause_key, b.kind, yarns=False)
        if np.any(res.status & (abi.STATUS_DUP | abi.STATUS_INTERNAL)):
            raise C.CauseError("document outside the weave's domain", {"weave-domain"})
        r = w.render_lists(b.offsets, res.weave_perm, res.visible_bits, refs[:n_list_nodes])
        off.append(r.offsets[1:])
        ref.append(r.value), src.append(r.src)
        key += [None] * len(r.src)
    if maps:
        pm = pack.pack_maps(maps)
        res = w.weave_maps(pm.offsets, pm.id_key, pm.cause, pm.cause_is_id, pm.kind, pm.token_bits,
                           pm.layout.key_bits)
        if np.any(res.status & (abi.STATUS_DUP | abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL)):
            raise C.CauseError("map outside the weave's domain", {"weave-domain"})
        r = w.render_maps(len(maps), res.seg_coll, res.seg_key, res.seg_active, pm.offsets, refs[n_list_nodes:])
        off.append(r.offsets[1:] + off[-1][-1])
        ref.append(r.value), src.append(r.src)
        for d in range(len(maps)):
            key += [C._seg_key(k, pm, d) for k in r.key[int(r.offsets[d]):int(r.offsets[d + 1])].tolist()]
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return cat(off, np.uint64), cat(ref, np.uint32), cat(src, np.uint32), key


def bases_to_edn(cbs, render_fn=None, entries_fn=None):
    """cb->edn (base/core.cljc:92-96) of many bases -> [edn].  Every collection
    of every base goes through one weave and one render call per kind, the refs
    are resolved by ONE cw_render_bases call, and each base's nested value is
    rebuilt from its token stream with one stack pass.  A base the call flags
    (a collection referred to twice, a reference cycle) goes through cb_to_edn.
    render_fn: the call (default: the GPU), taking abi_render_bases.render_bases'
    arguments after the Weaver.  entries_fn: what makes the entry table
    (default: the GPU weaves and renders), taking _gpu_entries' arguments."""
    cbs = list(cbs)
    docs, n_lists, index, roots = _collect_docs(cbs)
    ent_off, ent_ref, ent_src, ent_key = (entries_fn or _gpu_entries)(docs, n_lists, _ref_column(docs, index))
    res = (render_fn or _gpu_render_bases)(ent_off, ent_ref, roots)
    kinds, tdoc, tent = res.tok_kind.tolist(), res.tok_doc.tolist(), res.tok_entry.tolist()
    src, bo = ent_src.tolist(), res.base_tok_offsets.tolist()
    map0 = int(ent_off[n_lists])          # the first entry of a map
    out = []
    for g, cb in enumerate(cbs):
        if int(res.base_status[g]) & RB.STATUS_REF_SHARED:
            out.append(cb_to_edn(cb)[0])
            continue
        value, stack = None, []           # stack: the open collections, innermost last

        def put(e, v):                    # entry e of the innermost collection gets the value v
            if e >= map0:
                stack[-1][ent_key[e]] = v
            else:
                stack[-1].append(v)

        for t in range(bo[g], bo[g + 1]):
            k, d, e = kinds[t], tdoc[t], tent[t]
            if k == RB.TOK_OPEN:
                stack.append([] if d < n_lists else {})
            elif k == RB.TOK_CLOSE:
                value = stack.pop()
                if stack:
                    put(e, value)
            elif k == RB.TOK_LEAF:
                put(e, docs[d][2][src[e]][2])
            else:
                put(e, None)
        out.append(value)
    return out


def history(cb):
    """The ::history log: [(id, uuid)] sorted by id (vector compare of
    util.cljc:4-10), sorted on the GPU (cw_sort_keys)."""
    hist = cb["history"]
    if not hist:
        return []
    sites = sorted({i[1] for i, _ in hist}, key=pack.java_str_key)
    rank = {s: r for r, s in enumerate(sites)}
    ts_bits = max(1, max(i[0] for i, _ in hist).bit_length())
    tx_bits = max(1, max(i[2] for i, _ in hist).bit_length())
    site_bits = max(1, (len(sites) - 1).bit_length())
    if ts_bits + site_bits + tx_bits > 63:
        raise ValueError("history ids do not pack into 63 bits")
    keys = np.array([(i[0] << (site_bits + tx_bits)) | (rank[i[1]] << tx_bits) | i[2]
                     for i, _ in hist], np.uint64)
    _, order = C.weaver().sort_keys(keys, ts_bits + site_bits + tx_bits)
    return [hist[j] for j in order]
