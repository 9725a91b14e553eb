"""Bases for the cw_render_bases tests, and the CPU side of bases_to_edn: the
collections woven by the CPU reference (oracle/causal_ref.py) instead of the
GPU, so that base.py's cb_to_edn and bases_to_edn run without one.
"""
import random

import numpy as np

from cause_amd import base as B, causal as C
from oracle import causal_ref as R
from tests import invert_model

K = lambda name: C.Keyword(None, name)
R_KW = {C.HIDE: R.HIDE, C.H_HIDE: R.H_HIDE, C.H_SHOW: R.H_SHOW}
U32, U64 = np.uint32, np.uint64


def _rct(kind, nodes):
    """A collection for the CPU reference: its special keywords are the reference's."""
    return {"type": kind, "lamport_ts": 0, "uuid": "u", "site_id": "s", "weave": None,
            "nodes": {i: (c, R_KW.get(v, v) if isinstance(v, C.Keyword) else v) for i, c, v in nodes}}


def cpu_weave_all(cb):
    """base.weave_all by the CPU reference's full reweave: every collection gets
    what cb_to_edn reads (weave and _visible, or _active) and is clean."""
    new = {}
    for u, ct in cb["collections"].items():
        nodes = [(i, b[0], b[1]) for i, b in ct["nodes"].items()]
        own = {i: (i, c, v) for i, c, v in nodes}
        out = dict(ct, _dirty=False)
        if ct["type"] == "list":
            w = R.list_weave(_rct("list", nodes))["weave"]
            out["weave"] = [C.ROOT_NODE if n[0] == C.ROOT_ID else own[n[0]] for n in w]
            out["_visible"] = [not R.hide_q(n, w[k + 1] if k + 1 < len(w) else None) for k, n in enumerate(w)]
        else:
            w = R.map_weave(_rct("map", nodes))["weave"]
            out["weave"] = w
            out["_active"] = {}
            for k, wk in w.items():
                n = R.active_node(k, wk)
                out["_active"][k] = C.BLANK if n is R.BLANK else (n[0], k, own[n[0]][2])
        new[u] = out
    return dict(cb, collections=new)


def cpu_entries(docs, n_lists, refs):
    """base._gpu_entries on the CPU: the rendered entries of every document."""
    off, ref, src, key = [0], [], [], []
    at = 0
    for d, (_, _, nodes) in enumerate(docs):
        pos = {i: k for k, (i, _, _) in enumerate(nodes)}
        if d < n_lists:
            shown = [(n[0], None) for n in R.causal_list_to_list(R.list_weave(_rct("list", nodes)))]
        else:
            shown = [(n[0], n[1]) for n in R.causal_map_to_list(R.map_weave(_rct("map", nodes)))]
        for i, k in shown:
            src.append(pos[i])
            ref.append(int(refs[at + pos[i]]))
            key.append(k)
        at += len(nodes)
        off.append(len(src))
    return np.array(off, U64), np.array(ref, U32), np.array(src, U32), key


# ------------------------------------------------------------------- bases ----
def cb0(seed=0):
    return B.new_cb(random.Random(seed))


def known_answers():
    """[(base, edn)]: the reference's own tests, as tests/test_base.py restates
    them (base/core_test.cljc:8-15, :60-83)."""
    out = [(cb0(), None)]
    cb = B.transact_(cb0(), [[None, None, [K("div"), {K("foo"): "bar"}, "wat", [K("p"), "baz"]]]])
    out.append((cb, [K("div"), {K("foo"): "bar"}, "w", "a", "t", [K("p"), "b", "a", "z"]]))
    cb = B.transact_(cb0(), [[None, None, {K("a"): 1}]])
    r = cb["root_uuid"]
    out += [(cb, {K("a"): 1}),
            (B.transact_(cb, [[r, K("a"), "hi"]]), {K("a"): "hi"}),
            (B.transact_(cb, [[r, None, {K("a"): 2, K("b"): 3}]]), {K("a"): 2, K("b"): 3}),
            (B.transact_(cb, [[r, K("b"), {K("c"): 2}]]), {K("a"): 1, K("b"): {K("c"): 2}}),
            (B.transact_(cb, [[r, K("a"), C.HIDE], [r, None, {K("b"): 2, K("c"): "hi"}],
                              [r, None, {K("b"): C.HIDE}]]), {K("c"): "hi"})]
    cb = B.transact_(cb0(), [[None, None, [1, 2]]])
    r = cb["root_uuid"]
    out += [(cb, [1, 2]),
            (B.transact_(cb, [[r, C.ROOT_ID, 0]]), [0, 1, 2]),
            (B.transact_(cb, [[r, C.ROOT_ID, [0]]]), [0, 1, 2]),
            (B.transact_(cb, [[r, C.ROOT_ID, [-2, -1, 0]]]), [-2, -1, 0, 1, 2]),
            (B.transact_(cb, [[r, C.ROOT_ID, "hi"]]), ["h", "i", 1, 2]),
            (B.transact_(cb, [[r, C.ROOT_ID, ["hi"]]]), ["h", "i", 1, 2]),
            (B.transact_(cb, [[r, C.ROOT_ID, [["hi"]]]]), [["h", "i"], 1, 2])]
    return out


def random_value(rng, depth=0):
    x = rng.random()
    if depth >= 4 or x < 0.35:
        return rng.choice([rng.randint(-9, 99), "txt", K("kw"), 2.5, True])
    if x < 0.7:
        return [random_value(rng, depth + 1) for _ in range(rng.randint(0, 4))]
    return {rng.choice("abcdef"): random_value(rng, depth + 1) for _ in range(rng.randint(0, 4))}


def random_base(rng, seed, steps=5, history=True):
    """A base of nested plain values: a root, then transactions that add, replace
    and hide nested values, then (history) some undo_ / redo_ steps."""
    cb = B.new_cb(random.Random(seed))
    root = random_value(rng, 0)
    while not isinstance(root, (list, dict)) or not root:
        root = random_value(rng, 0)
    cb = B.transact_(cb, [[None, None, root]])
    r = cb["root_uuid"]
    for _ in range(rng.randint(0, steps)):
        uuid = rng.choice(list(cb["collections"]))
        ct = cb["collections"][uuid]
        v = rng.choice([random_value(rng, 1), C.HIDE])
        if ct["type"] == "map":
            keys = [c for c, _ in ct["nodes"].values() if isinstance(c, str)] + list("abg")
            cb = B.transact_(cb, [[uuid, rng.choice(keys), v]])
        else:
            cause = rng.choice(list(ct["nodes"]))
            if v is C.HIDE and cause == C.ROOT_ID:
                v = 7
            cb = B.transact_(cb, [[uuid, cause, v]])
    if history:
        for op in rng.choice([(), ("undo",), ("undo", "undo"), ("undo", "redo"), ("undo", "undo", "redo")]):
            cb = (B.undo_ if op == "undo" else B.redo_)(cb, invert_fn=invert_model.invert_columns)
    assert r == cb["root_uuid"]
    return cb


def random_bases(seed, n, **kw):
    rng = random.Random(seed)
    return [random_base(rng, seed * 1000 + g, **kw) for g in range(n)]
