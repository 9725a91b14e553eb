"""cw_weft_lists / k_weft_select vs the CPU model of weft, array for array (-m gpu).

Every call goes through the C ABI with result arrays built here by ctypes, so
that the optional outputs can be NULL and every array carries guard words past
the room the header asks for (N + (n_docs << site_bits) kept nodes).  The
model (tests/weft_model.py, pinned to R.weft by tests/test_weft_model.py) is
the literal fold of the oracle on the kept nodes; every comparison is equality,
for every document -- test_weft_model.py shows that no input has a repeated id,
the one case whose output is unspecified.

Covered: the tile loop of k_weft_select (1,024 threads) and its carry, koff in
ragged batches, site_bits 1 / 4 / 10 with every found[] word and the exact
capacity of the kept arrays, kept documents beyond the fused kernel (giant and
exact path), the context options, NULL outputs, empty shapes, the error
returns, and weft alternating with cw_weave_lists on one context.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from cause_amd import abi, causal, pack
from tests import weft_model as M

pytestmark = pytest.mark.gpu

GUARD = 64                 # words past the end of every result array
FILL = 0xA5                # ... and what they and the unwritten tail must still hold


@pytest.fixture(scope="module")
def weaver():
    with abi.Weaver(0) as w:
        yield w


class Out:
    """The result arrays of one raw call, filled with FILL bytes beforehand."""

    def __init__(self, D, cap, yarns, bits, max_ts):
        new = lambda n, dt: np.full(n + GUARD, np.iinfo(dt).max // 255 * FILL, dt)
        self.cap = cap
        self.kept_offsets = new(D + 1, np.uint64)
        self.src = new(cap, np.uint32)
        self.weave_perm = new(cap, np.uint32)
        self.visible_bits = new((cap + 31) // 32, np.uint32) if bits else None
        self.visible_count = new(D, np.uint32)
        self.max_ts = new(D, np.uint64) if max_ts else None
        self.status = new(D, np.uint32)
        self.yarn_perm = new(cap, np.uint32) if yarns else None

    def untouched(self, name, start):
        a = getattr(self, name)
        return bool(np.all(a[start:] == np.iinfo(a.dtype).max // 255 * FILL))


def raw_weft(weaver, off, idk, ck, kd, layout, cut, yarns=True, bits=True, max_ts=True,
             site_bits=None, memspace=abi.CW_MEM_HOST, null_cut=False):
    """cw_weft_lists with result arrays of exactly the header's capacity (+ the
    guard).  -> (return code, Out)."""
    off = np.ascontiguousarray(off, np.uint64)
    i, c, k = (np.ascontiguousarray(idk, np.uint64), np.ascontiguousarray(ck, np.uint64),
               np.ascontiguousarray(kd, np.uint8))
    cut = np.ascontiguousarray(cut, np.uint64)
    D, N = len(off) - 1, len(i)
    b, off = abi.Weaver._batch(off, abi._ptr(i), abi._ptr(c), abi._ptr(k), layout)
    if site_bits is not None:
        b.site_bits = site_bits
    wb = abi.CwWeftBatch(b, None if null_cut else cut.ctypes.data_as(C.POINTER(C.c_uint64)))
    o = Out(D, N + (D << layout.site_bits), yarns, bits, max_ts)
    r = abi.CwWeftResult(o.kept_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), abi._ptr(o.src),
                         abi.CwListResult(abi._ptr(o.weave_perm), abi._ptr(o.visible_bits),
                                          abi._ptr(o.visible_count), abi._ptr(o.max_ts),
                                          abi._ptr(o.status), abi._ptr(o.yarn_perm)))
    rc = weaver._L.cw_weft_lists(weaver._h, C.byref(wb), C.byref(r), memspace)
    return rc, o


def last_error(weaver):
    return weaver._L.cw_last_error(weaver._h).decode()


def check_weft(weaver, off, idk, ck, kd, layout, cut, exp=None, yarns=True, bits=True,
               max_ts=True):
    """One call == the model, for every document and every array: kept offsets
    and src, weave_perm, the visible flag of every global kept position,
    visible_count, max_ts (nonempty kept sets), status, yarn_perm -- and nothing
    written past the kept nodes.  -> the call's Out."""
    if exp is None:
        exp = M.weft_expected(off, idk, ck, kd, layout, cut)
    rc, o = raw_weft(weaver, off, idk, ck, kd, layout, cut, yarns=yarns, bits=bits, max_ts=max_ts)
    assert rc == 0, last_error(weaver)
    D, Mk = len(exp.offsets) - 1, len(exp.src)
    assert Mk <= o.cap
    assert np.array_equal(o.kept_offsets[:D + 1], exp.offsets), "kept_offsets"
    ko = exp.offsets.astype(np.int64)
    for name, want in (("src", exp.src), ("weave_perm", exp.weave_perm),
                       ("yarn_perm", exp.yarn_perm if yarns else None)):
        if want is None:
            continue
        got = getattr(o, name)
        if not np.array_equal(got[:Mk], want):
            bad = int(np.nonzero(got[:Mk] != want)[0][0])
            d = int(np.searchsorted(ko, bad, side="right")) - 1
            raise AssertionError(f"{name}: document {d} (kept {ko[d + 1] - ko[d]} nodes, status "
                                 f"{exp.status[d]}) differs at kept position {bad - ko[d]}")
        assert o.untouched(name, Mk), f"{name} written past the {Mk} kept nodes"
    if bits:
        words = (Mk + 31) // 32
        flags = np.unpackbits(o.visible_bits[:words].view(np.uint8), bitorder="little")[:Mk]
        if not np.array_equal(flags, exp.visible):
            bad = int(np.nonzero(flags != exp.visible)[0][0])
            d = int(np.searchsorted(ko, bad, side="right")) - 1
            raise AssertionError(f"visible_bits: document {d} differs at weave position {bad - ko[d]}")
        assert o.untouched("visible_bits", words), "visible_bits written past the kept nodes"
    assert np.array_equal(o.visible_count[:D], exp.visible_count), "visible_count"
    if max_ts:
        ne = np.diff(ko) > 0
        assert np.array_equal(o.max_ts[:D][ne], exp.max_ts[ne]), "max_ts"
        assert o.untouched("max_ts", D)
    assert np.array_equal(o.status[:D], exp.status), (o.status[:D], exp.status)
    for name, n in (("kept_offsets", D + 1), ("visible_count", D), ("status", D)):
        assert o.untouched(name, n), f"{name} written past its {n} entries"
    return o


def check_case(weaver, name, **kw):
    return check_weft(weaver, *M.CASES[name](), exp=M.expected(name), **kw)


ARRAYS = ("kept_offsets", "src", "weave_perm", "visible_bits", "visible_count", "max_ts",
          "status", "yarn_perm")


def assert_same_arrays(a, b, skip=()):
    """Two calls' result arrays, guard and unwritten tail included.  (max_ts of
    an empty kept set and the bits past the last kept node are unspecified, so
    those two are compared through the model only.)"""
    for f in ARRAYS:
        if f in skip or f in ("max_ts", "visible_bits"):
            continue
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


# ------------------------------------------------ 1. tiles, a ragged batch ----
@pytest.mark.parametrize("yarns", [True, False])
def test_tile_boundaries_in_a_ragged_batch(weaver, yarns):
    M.assert_status_classes(M.expected("tiles"), M.case_tiles())
    check_case(weaver, "tiles", yarns=yarns)


# ----------------------------------------------------------- 2. site widths ----
@pytest.mark.parametrize("name", ["bits1", "bits10", "all_ranks_absent", "upper_words"])
def test_site_widths(weaver, name):
    """site_bits = 1 and 10 (4 is the ragged batch): every found[] word, the
    scan of the missing cuts over 1,024 ranks, rows of ranks with no node, and a
    kept size of exactly N + (D << site_bits)."""
    exp = M.expected(name)
    if name == "bits10":
        M.assert_status_classes(exp, M.case_bits10())
    if name == "all_ranks_absent":
        off, idk, _, _, lay, _ = M.case_all_ranks_absent()
        assert int(exp.offsets[-1]) == len(idk) + (1 << lay.site_bits)
    if name == "bits1":  # (one site: no cut can orphan a node of it)
        st = exp.status
        assert (st == 0).any() and (st & abi.STATUS_WEFT).any()
    check_case(weaver, name)


# ----------------------------------------------- 3. beyond the fused kernel ----
@pytest.mark.parametrize("name", M.GIANT_CASES)
def test_kept_documents_beyond_the_fused_kernel(weaver, name):
    """70,001 nodes, 3 sites: all kept (giant path), a consistent cut below
    65,536, a cut with orphans above 65,535 (exact path); then the three as one
    batch (the per-document tree)."""
    exp = M.expected(name)
    kept = np.diff(exp.offsets.astype(np.int64))
    if name == "giant_whole":
        assert kept[0] == M.GIANT_N > 65535 and exp.status[0] == 0
    elif name == "giant_closed":
        assert kept[0] < 65536 and exp.status[0] == 0
    elif name == "giant_gibberish":
        assert kept[0] > 65535 and exp.status[0] == abi.STATUS_ORPHAN
    else:
        assert len(kept) == 3 and kept[0] > 65535 > kept[1] and kept[2] > 65535
    check_case(weaver, name)


def test_kept_size_chooses_the_path():
    """The three 70,001-node cuts reach the paths they are for (per-kernel
    profile of the call): the giant tree (geff) from 65,536 kept nodes in a
    one-document call, the fused kernel (weave) below, the exact path (xjoin)
    for the cut with orphans, alone and in the batch."""
    with abi.Weaver(0) as w:
        w.set_profiling(True)
        ran = {}
        for name in M.GIANT_CASES:
            w.reset_kernel_stats()
            check_case(w, name)
            ran[name] = set(w.kernel_stats())
    show = "\n".join(f"{k}: {sorted(v)}" for k, v in ran.items())
    assert {"gdir", "geff"} <= ran["giant_whole"] and "xjoin" not in ran["giant_whole"], show
    assert "weave" in ran["giant_closed"] and not {"gdir", "geff", "xjoin"} & ran["giant_closed"], show
    assert {"gdir", "geff", "xjoin"} <= ran["giant_gibberish"], show
    # the batch: the per-document directories, no giant front end; its third
    # document rewoven by the exact path (whose synthetic list may be a giant one)
    assert {"fdir", "xjoin"} <= ran["giant_batch"] and "gdir" not in ran["giant_batch"], show


# -------------------------------------------------------- 4. context options ----
PATHS = {"fused0": {"fused": 0}, "tour0": {"tour": 0}, "front0": {"front": 0},
         "tree_l0": {"tree_l": 0}}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_path_gives_the_same_arrays(path):
    with abi.Weaver(0, options=PATHS[path]) as w:
        check_case(w, "tiles")
        check_case(w, "giant_whole")


def test_giant_path_on_a_small_document():
    """giant_min = 0: a one-document batch of 5,001 nodes (337 kept) takes the
    giant path; the batches are untouched by it."""
    with abi.Weaver(0, options={"giant_min": 0}) as w:
        check_case(w, "one_5001")
        check_case(w, "tiles")
        check_case(w, "giant_whole")


# -------------------------------------------------------- 5. optional outputs ----
@pytest.mark.parametrize("null", [("bits",), ("max_ts",), ("yarns",), ("bits", "max_ts", "yarns")],
                         ids=lambda t: "+".join(t))
def test_optional_outputs_null(weaver, null):
    full = check_case(weaver, "tiles")
    o = check_case(weaver, "tiles", **{k: False for k in null})
    gone = {"bits": "visible_bits", "max_ts": "max_ts", "yarns": "yarn_perm"}
    assert_same_arrays(full, o, skip=[gone[k] for k in null])


# ------------------------------------------------------------ 6. empty shapes ----
def test_no_documents(weaver):
    lay = pack.KeyLayout(8, 4, 0)
    z64 = np.zeros(0, np.uint64)
    rc, o = raw_weft(weaver, np.zeros(1, np.uint64), z64, z64, np.zeros(0, np.uint8), lay, z64)
    assert rc == 0, last_error(weaver)
    assert o.kept_offsets[0] == 0 and o.untouched("kept_offsets", 1)
    for f in ("src", "weave_perm", "visible_bits", "visible_count", "max_ts", "status", "yarn_perm"):
        assert o.untouched(f, 0), f


def test_every_document_empty(weaver):
    lay = pack.KeyLayout(8, 4, 0)
    D = 5
    z64 = np.zeros(0, np.uint64)
    args = (np.zeros(D + 1, np.uint64), z64, z64, np.zeros(0, np.uint8), lay,
            np.zeros(D << lay.site_bits, np.uint64))
    exp = M.weft_expected(*args)
    assert list(exp.status) == [abi.STATUS_ROOT] * D
    o = check_weft(weaver, *args, exp=exp)
    assert list(o.status[:D]) == [abi.STATUS_ROOT] * D and not o.kept_offsets[:D + 1].any()


def test_empty_document_with_a_cut_named(weaver):
    exp = M.expected("empty_named")
    assert list(np.diff(exp.offsets.astype(np.int64))) == [1, 1, 0]
    assert exp.src[1] == M.NO_SRC and exp.status[1] & abi.STATUS_WEFT
    check_case(weaver, "empty_named")


# ------------------------------------------------------------------ 7. errors ----
def _bad_calls():
    off, idk, ck, kd, lay, cut = M.case_small()
    D, N = len(off) - 1, len(idk)
    shifted = off.copy()
    shifted[0] = 1
    falling = off.copy()
    falling[2] = falling[3] + np.uint64(5)  # offsets[2] > offsets[3]
    assert falling[2] <= N
    return {
        "site_bits 0": dict(site_bits=0),
        "site_bits 11": dict(site_bits=11),
        "device memory": dict(memspace=abi.CW_MEM_DEVICE),
        "null cut": dict(null_cut=True),
        "offsets[0] != 0": dict(off=shifted),
        "offsets decrease": dict(off=falling),
    }


@pytest.mark.parametrize("bad", sorted(_bad_calls()))
def test_error_returns_and_the_context_lives_on(weaver, bad):
    off, idk, ck, kd, lay, cut = M.case_small()
    kw = dict(_bad_calls()[bad])
    rc, o = raw_weft(weaver, kw.pop("off", off), idk, ck, kd, lay, cut, **kw)
    assert rc < 0 and last_error(weaver), (bad, rc)
    for f in ("src", "weave_perm", "status"):
        assert o.untouched(f, 0), f"{f} written by a refused call"
    check_case(weaver, "small")


def test_wrapper_raises_weave_error(weaver):
    off, idk, ck, kd, lay, cut = M.case_small()
    D = len(off) - 1
    for sb in (0, 11):
        with pytest.raises(abi.WeaveError, match="site_bits"):
            weaver.weft_lists(off, idk, ck, kd, pack.KeyLayout(lay.ts_bits, sb, 0),
                              np.zeros(D << sb, np.uint64))
    shifted = off.copy()
    shifted[0] = 1
    with pytest.raises(abi.WeaveError, match="doc_offsets"):
        weaver.weft_lists(shifted, idk, ck, kd, lay, cut)
    # ... and the wrapper's arrays equal the model's
    exp = M.expected("small")
    res = weaver.weft_lists(off, idk, ck, kd, lay, cut)
    assert np.array_equal(res.offsets, exp.offsets) and np.array_equal(res.src, exp.src)
    assert np.array_equal(res.weave.weave_perm, exp.weave_perm)
    assert np.array_equal(res.weave.visible(), exp.visible)
    assert np.array_equal(res.weave.visible_count, exp.visible_count)
    assert np.array_equal(res.weave.status, exp.status)
    assert np.array_equal(res.weave.yarn_perm, exp.yarn_perm)


# -------------------------------------- 8. cached tables and scratch reuse ----
def test_weft_alternating_with_weave_on_one_context():
    """ensure_tables caches by offset content and the scratch buffers are
    reused: weft A, weave_lists of A's input (same D, other offsets), weft A,
    weft of the much smaller B, weft A -- every weft of A the same arrays."""
    off, idk, ck, kd, lay, cut = M.case_tiles()
    perm, vis, st = oracle.batch_lists(off, idk, ck, kd, method=oracle.METHOD_LITERAL)
    assert not st[np.diff(off.astype(np.int64)) > 0].any()
    with abi.Weaver(0) as w:
        first = check_case(w, "tiles")
        res = w.weave_lists(off, idk, ck, kd, lay)
        assert np.array_equal(res.status, st)
        assert np.array_equal(res.weave_perm, perm) and np.array_equal(res.visible(), vis)
        assert_same_arrays(first, check_case(w, "tiles"))
        check_case(w, "small")
        assert_same_arrays(first, check_case(w, "tiles"))
        res = w.weave_lists(off, idk, ck, kd, lay)
        assert np.array_equal(res.weave_perm, perm) and np.array_equal(res.visible(), vis)


# ------------------------------------------------- 9. the mirror in one call ----
def test_mirror_one_call_many_documents():
    """causal.weft_lists of ~100 (ct, ids) items in ONE cw_weft_lists call (site
    ranks differ per document) == R.weft per item."""
    items = M.mirror_items(seed=21)
    cts = []
    for ref, ids, _ in items:
        ct = causal.new_list_ct(site_id=ref["site_id"], uuid=ref["uuid"])
        ct["nodes"] = dict(ref["nodes"])
        cts.append((ct, ids))
    got = causal.weft_lists(cts)
    checked, gibberish, bogus = M.check_mirror(items, got)
    assert checked > 60 and gibberish > 5 and bogus > 5, (checked, gibberish, bogus)
