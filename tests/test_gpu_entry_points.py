"""Every host-memory entry point on ONE context.

cw_weave_lists, cw_weave_lists_k32, cw_weave_lists_k128, cw_merge_lists and
cw_weft_lists stage the caller's cw_list_result under one set of scratch names
(stage_list_result), and every entry point uploads its inputs through one
helper.  What that sharing can break is a call that finds a buffer an earlier,
different call left behind: too small, or holding that call's words.  So one
Weaver runs all seven entry points in turn, then again in reverse order on a
larger batch (every staged buffer regrows), then the all-empty batches, then
the first batch once more.  Every result must equal, array for array, the
same call on a fresh context, and that reference passed the oracle checks of
the feature's own test module.

Two parts of a list result are unspecified and compared as those modules
compare them: max_ts of an empty document (not written) and the bits of the
last visible_bits word past the last node."""
import numpy as np
import pytest

import oracle
from cause_amd import abi, gen, pack
from tests import weft_model as M
from tests.test_gpu_list_merge import check as check_list_merge
from tests.test_gpu_map_merge import check as check_map_merge
from tests.test_gpu_map_merge import split as split_maps
from tests.test_gpu_maps import check as check_maps
from tests.test_gpu_merge import split_batch
from tests.test_gpu_weft import check_weft, last_error, raw_weft

pytestmark = pytest.mark.gpu

# empty documents in front and inside (the ROOT fix-up), one node, one document
# above a 2,048-rank tile; then more documents and more nodes in every array
SIZES_A = (0, 1, 37, 300, 0, 2049)
SIZES_B = (5, 0, 4100, 1, 700, 0, 2500, 64)
SIZES_EMPTY = (0, 0, 0)
# tests/test_gpu_maps.py::test_ragged_and_empty_collections, and a larger one
COLLS_A = (0, 1, 2, 0, 5, 100, 4097, 1, 0, 9000, 33)
COLLS_B = (700, 0, 9500, 3, 0, 4097, 4097, 1, 12, 0, 0, 260, 2)
OPTIONS = {"map_fused": 0}  # cw_weave_maps (and the weave inside cw_merge_maps): the general path
LIST_FIELDS = ("weave_perm", "visible_count", "status", "yarn_perm")
MAP_FIELDS = ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm", "status")


# ------------------------------------------------------------------ inputs ----
def list_batch(sizes, seed):
    """(offsets, id_key, cause_key, kind, layout, cut) with documents of exactly
    these sizes; every rank of a document draws a cut of its own kind (none in
    an empty document, whose kept set then is empty too: an absent cut id would
    keep an [id] node)."""
    rng = np.random.default_rng(seed)
    spec = M.spec_for(8, max(max(sizes) - 1, 1))
    off, idk, ck, kd = M.ragged(spec, list(sizes), rng)
    lay = spec.layout()
    modes = ["random" if n else "none" for n in sizes]
    return off, idk, ck, kd, lay, M.make_cuts(off, idk, lay, rng, modes)


def map_batch(sizes, seed):
    """(offsets, id_key, cause, cause_is_id, kind) with collections of these sizes."""
    rng = np.random.default_rng(seed)
    parts = []
    for d, n in enumerate(sizes):
        if n == 0:
            parts.append((np.zeros(0, np.uint64),) * 2 + (np.zeros(0, np.uint8),) * 2)
            continue
        spec = gen.MapSpec(nodes_per_coll=n, n_keys=int(rng.integers(1, 300)), seed=100 + d)
        parts.append(gen.generate_maps(spec, d, d + 1, nthreads=1)[1:])
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    return (off,) + tuple(np.concatenate([p[j] for p in parts]) for j in range(4))


def to128(k, lay):
    """K64 packed keys as K128 (hi = ts, lo = site << 32 | tx): the same order."""
    k = k.astype(np.uint64)
    nil = k == np.uint64(pack.NIL)
    hi = k >> np.uint64(lay.ts_shift)
    site = (k >> np.uint64(lay.site_shift)) & np.uint64((1 << lay.site_bits) - 1)
    lo = (site << np.uint64(32)) | (k & np.uint64((1 << lay.tx_bits) - 1))
    out = np.stack([hi, lo], axis=1)
    out[nil] = np.uint64(pack.NIL)
    return out


# ------------------------------------------------- results as named arrays ----
def list_arrays(r, off):
    """A ListResult's specified words: max_ts of the nonempty documents, the
    visible flag of every weave position."""
    full = np.diff(np.asarray(off).astype(np.int64)) > 0
    out = {f: getattr(r, f) for f in LIST_FIELDS}
    out["visible"] = r.visible()
    out["max_ts"] = r.max_ts[full]
    return out


def merge_arrays(r):
    return dict(list_arrays(r.weave, r.offsets), offsets=r.offsets, src=r.src)


def weft_arrays(o, D):
    """A raw cw_weft_lists call's arrays (tests.test_gpu_weft.Out), guard words
    included where every word is specified."""
    ko = o.kept_offsets[:D + 1]
    Mk = int(ko[D])
    full = np.diff(ko.astype(np.int64)) > 0
    out = {f: getattr(o, f) for f in ("kept_offsets", "src", "weave_perm", "visible_count", "status",
                                      "yarn_perm")}
    out["visible"] = np.unpackbits(o.visible_bits[:(Mk + 31) // 32].view(np.uint8), bitorder="little")[:Mk]
    out["max_ts"] = o.max_ts[:D][full]
    out["max_ts_guard"] = o.max_ts[D:]
    return out


def map_arrays(r):
    return {f: getattr(r, f) for f in MAP_FIELDS}


def check_lists(res, off, idk, ck, kd, lay):
    """A list weave against the oracle: order, visibility, counts, status,
    ::lamport-ts and the yarns of every document."""
    perm, vis, st = oracle.batch_lists(off, idk, ck, kd, method=oracle.METHOD_LITERAL)
    assert not (st & abi.STATUS_DUP).any()
    b = off.astype(np.int64)
    np.testing.assert_array_equal(res.status, st)
    np.testing.assert_array_equal(res.weave_perm, perm)
    np.testing.assert_array_equal(res.visible(), vis)
    for d in range(len(b) - 1):
        lo, hi = b[d], b[d + 1]
        assert res.visible_count[d] == int(vis[lo:hi].sum()), d
        if hi > lo:
            assert res.max_ts[d] == int(idk[lo:hi].max()) >> lay.ts_shift, d
            np.testing.assert_array_equal(
                res.yarn_perm[lo:hi], oracle.list_yarns(idk[lo:hi], lay.site_shift, (1 << lay.site_bits) - 1))
    return res


# ------------------------------------------------------------ entry points ----
# name -> (call(weaver, inputs) -> named arrays, reference(weaver, inputs) ->
# named arrays of a call that passed the feature's oracle checks)
def _lists(w, b):
    off, idk, ck, kd, lay, _ = b["list"]
    return w.weave_lists(off, idk, ck, kd, lay)


def _k32(w, b):
    off, idk, ck, kd, lay, _ = b["list"]
    return w.weave_lists_k32(off, *abi.narrow_k32(idk, ck), kd, lay)


def _k128(w, b):
    off, idk, ck, kd, lay, _ = b["list"]
    return w.weave_lists_k128(off, to128(idk, lay), to128(ck, lay), kd)


def _weft(w, b, checked):
    off, idk, ck, kd, lay, cut = b["list"]
    if checked:
        o = check_weft(w, off, idk, ck, kd, lay, cut, exp=b["weft_exp"])
    else:
        rc, o = raw_weft(w, off, idk, ck, kd, lay, cut)
        assert rc == 0, last_error(w)
    return weft_arrays(o, len(off) - 1)


def _list_call(call):
    plain = lambda w, b: list_arrays(call(w, b), b["list"][0])
    checked = lambda w, b: list_arrays(check_lists(call(w, b), *b["list"][:5]), b["list"][0])
    return plain, checked


ENTRY_POINTS = {
    "weave_lists": _list_call(_lists),
    "weave_lists_k32": _list_call(_k32),
    "weave_lists_k128": _list_call(_k128),
    "merge_lists": (lambda w, b: merge_arrays(w.merge_lists(*b["list_sides"], b["list"][4])),
                    lambda w, b: merge_arrays(check_list_merge(w, *b["list_sides"], b["list"][4]))),
    "weft_lists": (lambda w, b: _weft(w, b, False), lambda w, b: _weft(w, b, True)),
    "weave_maps": (lambda w, b: map_arrays(w.weave_maps(*b["map"], b["token_bits"])),
                   lambda w, b: map_arrays(check_maps(w, *b["map"], b["token_bits"]))),
    "merge_maps": (lambda w, b: (lambda r: dict(map_arrays(r.maps), offsets=r.offsets, src=r.src))(
                       w.merge_maps(*b["map_sides"], b["token_bits"])),
                   lambda w, b: (lambda r: dict(map_arrays(r.maps), offsets=r.offsets, src=r.src))(
                       check_map_merge(w, *b["map_sides"], b["token_bits"])[0])),
}
LIST_ENTRY_POINTS = ("weave_lists", "weave_lists_k32", "weave_lists_k128", "merge_lists", "weft_lists")


def inputs(name, sizes, colls, seed):
    b = {"name": name, "list": list_batch(sizes, seed), "token_bits": 9}
    off, idk, ck, kd, lay, cut = b["list"]
    (a, _), (bb, _) = split_batch(off, idk, ck, kd, np.random.default_rng(seed), overlap=0.2)
    b["list_sides"] = (a, bb)
    b["weft_exp"] = M.weft_expected(off, idk, ck, kd, lay, cut)
    if colls:
        b["map"] = map_batch(colls, seed)
        b["map_sides"] = split_maps(b["map"][0], b["map"][1:], 0.3, np.random.default_rng(seed + 1))[:2]
    return b


def test_every_host_entry_point_on_one_context():
    A = inputs("A", SIZES_A, COLLS_A, 5)
    B = inputs("B", SIZES_B, COLLS_B, 6)
    E = inputs("empty", SIZES_EMPTY, None, 7)
    assert int(A["list"][0][-1]) < int(B["list"][0][-1]) and len(SIZES_A) < len(SIZES_B)
    assert int(A["map"][0][-1]) < int(B["map"][0][-1]) and len(COLLS_A) < len(COLLS_B)
    assert int(E["list"][0][-1]) == 0 and len(SIZES_EMPTY) == 3
    names = list(ENTRY_POINTS)
    sequence = ([(n, A) for n in names] + [(n, B) for n in reversed(names)] +
                [(n, E) for n in LIST_ENTRY_POINTS] + [(n, A) for n in names])

    reference = {}

    def want(n, b):
        """The call on a context of its own, through the feature's oracle checks."""
        if (n, b["name"]) not in reference:
            with abi.Weaver(0, options=OPTIONS) as fresh:
                reference[n, b["name"]] = ENTRY_POINTS[n][1](fresh, b)
        return reference[n, b["name"]]

    with abi.Weaver(0, options=OPTIONS) as w:
        for step, (n, b) in enumerate(sequence):
            got, ref = ENTRY_POINTS[n][0](w, b), want(n, b)
            assert got.keys() == ref.keys()
            for f in got:
                np.testing.assert_array_equal(got[f], ref[f],
                                              err_msg=f"step {step}: {n} on batch {b['name']}, {f}")
