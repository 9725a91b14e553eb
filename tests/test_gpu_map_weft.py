"""cw_weft_maps (CausalMap's weft, map.cljc:246-247) on the GPU, through the C ABI
and the Python mirror.

Every case compares every array with the CPU model (tests/mapweft_model.py):
kept_offsets, kept_src and the status with its WEFT bit; the key weaves are
identical to cw_weave_maps of the model's kept arrays (array for array: the
indices are collection-local into kept_src) and equal to the C oracle's literal
map fold.  No collection is skipped: tests/test_mapweft_model.py checks on the
CPU that no kept collection of any case repeats an id.  The weaver is
parametrised over the fused select kernel (k_map_weft) and the general route.
"""
import numpy as np
import pytest

from cause_amd import abi
from cause_amd import causal as C
from tests import mapweft_model as M
from tests.test_gpu_maps import gpu_maps
from tests.test_mapweft_model import check_mirror, mirror_ct

pytestmark = pytest.mark.gpu

MAP_FIELDS = ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm", "status")


@pytest.fixture(scope="module", params=[1, 0], ids=["fused", "general"])
def weaver(request):
    w = abi.Weaver(0, options={"map_weft_fused": request.param})
    w.fused = bool(request.param)
    yield w
    w.close()


# ------------------------------------------------------------------ helpers
def call(weaver, args):
    off, idk, ck, ci, kd, sh, sb, cut, tb = args
    return weaver.weft_maps(off, idk, ck, ci, kd, tb, sh, sb, cut)


def check(weaver, name, args=None, e=None):
    """The weft of CASES[name] against the model, cw_weave_maps of the model's
    kept arrays and the oracle's fold.  Returns the result."""
    args = M.case(name) if args is None else args
    e = M.expected(name) if e is None else e
    res = call(weaver, args)
    D = len(args[0]) - 1
    np.testing.assert_array_equal(res.offsets, e.offsets)
    np.testing.assert_array_equal(res.src, e.src)
    ref = weaver.weave_maps(e.offsets, *e.kept, args[8])
    assert not (ref.status & (abi.STATUS_DUP | abi.STATUS_MAP_KEY | abi.STATUS_INTERNAL)).any()
    for f in MAP_FIELDS[:-1]:
        np.testing.assert_array_equal(getattr(res.maps, f), getattr(ref, f), err_msg=f)
    np.testing.assert_array_equal(res.maps.status, ref.status | e.weft)
    got = gpu_maps(res.maps, D)
    for d in range(D):
        assert got[d] == e.folds[d], f"collection {d}"
    return res


def same(x, y):
    np.testing.assert_array_equal(x.offsets, y.offsets)
    np.testing.assert_array_equal(x.src, y.src)
    for f in MAP_FIELDS:
        np.testing.assert_array_equal(getattr(x.maps, f), getattr(y.maps, f), err_msg=f)


def routes(weaver, fn):
    """Kernel stat names of one call."""
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        fn()
        return set(weaver.kernel_stats())
    finally:
        weaver.set_profiling(False)
        weaver.reset_kernel_stats()


# ------------------------------------------------------------------ 1. packs
def test_pack_boundaries_and_status_classes(weaver):
    res = check(weaver, "boundaries")
    args, e = M.case("boundaries"), M.expected("boundaries")
    cls = M.status_classes(e, args)
    assert all(v > 0 for v in cls.values()), cls
    st, kept = res.maps.status, np.diff(res.offsets.astype(np.int64))
    assert ((st == 0) & (kept > 0)).any() and (st & abi.STATUS_WEFT).any()
    emptied = (kept == 0) & (np.diff(args[0].astype(np.int64)) > 0)
    assert emptied.any() and not st[emptied].any()
    assert not set(np.flatnonzero(kept == 0)) & set(res.maps.seg_coll.tolist())
    names = routes(weaver, lambda: call(weaver, args))
    assert ("map_weft" in names) == weaver.fused
    assert ({"mw_count", "mw_write"} <= names) == (not weaver.fused)


@pytest.mark.parametrize("limit", [512, 1024, 2048])
def test_pack_sizes(weaver, limit):
    check(weaver, f"pack{limit}")


def test_look_back_past_one_window(weaver):
    check(weaver, "lookback")


# ------------------------------------------------------------------ 2. site_bits
def test_site_bits_1(weaver):
    check(weaver, "bits1")


def test_site_bits_10(weaver):
    check(weaver, "bits10")


def test_every_rank_named_with_an_absent_id_fills_the_capacity(weaver):
    res = check(weaver, "all_ranks_absent")
    a = M.case("all_ranks_absent")
    assert int(res.offsets[-1]) == len(a[1]) + (1 << a[6])
    assert res.maps.status[0] & abi.STATUS_WEFT


def test_only_upper_ranks_named(weaver):
    check(weaver, "upper_words")


# ------------------------------------------------------------------ 3. past the pack limit
def test_kept_collection_over_the_pack_limit(weaver):
    """2,048 nodes and 16 [id] nodes: the select is still the fused kernel, the
    weave of the kept batch is cw_weave_maps' general path."""
    check(weaver, "kept_over_2048")
    names = routes(weaver, lambda: call(weaver, M.case("kept_over_2048")))
    assert ("map_weft" in names) == weaver.fused and "m_pack" not in names


def test_one_oversize_collection_takes_the_general_route(weaver):
    check(weaver, "oversize")
    names = routes(weaver, lambda: call(weaver, M.case("oversize")))
    assert {"mw_count", "mw_write"} <= names and "map_weft" not in names


# ------------------------------------------------------------------ 4. empty and degenerate
def test_empty_and_degenerate_batches(weaver):
    res = check(weaver, "d0")
    assert res.offsets.tolist() == [0] and len(res.maps.status) == 0
    res = check(weaver, "all_empty")
    assert res.offsets.tolist() == [0, 0, 0, 0] and res.maps.status.tolist() == [0, 0, 0]
    assert len(res.maps.seg_key) == 0
    res = check(weaver, "empty_named")
    assert res.offsets.tolist() == [0, 0, 1, 1] and res.src.tolist() == [M.NO_SRC]
    assert res.maps.status.tolist() == [0, abi.STATUS_WEFT, 0]
    assert res.maps.seg_coll.tolist() == [1] and res.maps.seg_key.tolist() == [(1 << 64) - 1]


# ------------------------------------------------------------------ 5. both routes
@pytest.mark.parametrize("name", ["boundaries", "bits10", "kept_over_2048"])
def test_both_routes_give_identical_arrays(name):
    with abi.Weaver(0, options={"map_weft_fused": 1}) as wf, \
            abi.Weaver(0, options={"map_weft_fused": 0}) as wg:
        same(call(wf, M.case(name)), call(wg, M.case(name)))


# ------------------------------------------------------------------ 6. device memory
GUARD = 0x5A


def _device_call(weaver, args, host):
    """weft_maps_device with every input and the cut table in device memory;
    each output array is followed by guard bytes."""
    import torch

    off, idk, ck, ci, kd, sh, sb, cut, tb = args
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    ins = [up(x) for x in (idk, ck, ci, kd)]
    gcut = up(cut)
    D, N = len(off) - 1, len(idk)
    cap = N + (D << sb)
    sizes = {"seg_offsets": (cap + 1) * 8, "seg_coll": cap * 4, "seg_key": cap * 8,
             "seg_active": cap * 8, "seg_perm": 2 * cap * 4, "status": D * 4, "src": cap * 4}
    bufs = {k: torch.full((n + 64,), GUARD, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    torch.cuda.synchronize()
    ko, S = weaver.weft_maps_device(off, [x.data_ptr() for x in ins], tb, 0, sh, sb, gcut.data_ptr(),
                                    bufs["src"].data_ptr(),
                                    {k: v.data_ptr() for k, v in bufs.items() if k != "src"}, cap)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ko, host.offsets)
    assert S == len(host.maps.seg_key)
    Mk = int(ko[-1])
    h = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, n in sizes.items():
        assert (h[k][n:] == GUARD).all(), f"guard bytes after {k}"
    view = lambda k, dt, n: h[k][:n * np.dtype(dt).itemsize].view(dt)
    np.testing.assert_array_equal(view("src", np.uint32, Mk), host.src)
    np.testing.assert_array_equal(view("seg_offsets", np.uint64, S + 1), host.maps.seg_offsets)
    np.testing.assert_array_equal(view("seg_coll", np.uint32, S), host.maps.seg_coll)
    np.testing.assert_array_equal(view("seg_key", np.uint64, S), host.maps.seg_key)
    np.testing.assert_array_equal(view("seg_active", np.int64, S), host.maps.seg_active)
    np.testing.assert_array_equal(view("seg_perm", np.uint32, Mk + S), host.maps.seg_perm)
    np.testing.assert_array_equal(view("status", np.uint32, D), host.maps.status)


@pytest.mark.parametrize("name", ["boundaries", "all_ranks_absent"])
def test_device_memory_call_matches_host(weaver, name):
    args = M.case(name)
    host = call(weaver, args)
    _device_call(weaver, args, host)
    weaver.set_async(True)
    try:
        _device_call(weaver, args, host)  # (it synchronises the device before it reads)
    finally:
        weaver.set_async(False)


# ------------------------------------------------------------------ 7. reuse
def test_reuse_of_one_context(weaver):
    """The pack table is cached by layout and site_bits and the look-back words
    carry an epoch: a large batch, a small one, the large one again; then the
    same layout with other cuts."""
    first = check(weaver, "lookback")
    check(weaver, "small")
    same(check(weaver, "lookback"), first)
    check(weaver, "bits10")  # another site_bits
    same(call(weaver, M.case("lookback")), first)
    a = list(M.case("small"))
    a[7] = M.W.make_cuts(a[0], a[1], M.KeyLayout(20, a[6], 0), np.random.default_rng(77),
                         ["whole", "absent", "random", "none", "closed"])
    assert not np.array_equal(a[7], M.case("small")[7])
    check(weaver, "small2", a, M.weft_maps_expected(*a[:8]))
    check(weaver, "small")


# ------------------------------------------------------------------ 8. errors
def test_bad_inputs_fail_with_a_text(weaver):
    off, idk, ck, ci, kd, sh, sb, cut, tb = M.case("small")
    for bad in (0, 11):
        with pytest.raises(abi.WeaveError, match="site_bits in 1..10"):
            weaver.weft_maps(off, idk, ck, ci, kd, tb, sh, bad, cut)
    back = off.copy()
    back[2], back[3] = back[3], back[2]  # offsets that run backwards inside
    assert back[3] < back[2] and back[-1] == off[-1]
    with pytest.raises(abi.WeaveError, match="not monotone"):
        weaver.weft_maps(back, idk, ck, ci, kd, tb, sh, sb, cut)
    with pytest.raises(abi.WeaveError, match="token_bits"):
        weaver.weft_maps(off, idk, ck, ci, kd, 0, sh, sb, cut)

    def raw(null_cut=False, null_src=False):
        oc = np.ascontiguousarray(off, np.uint64)
        p = lambda x: x.ctypes.data_as(abi.C.c_void_p)
        wb = abi.CwMapWeftBatch(weaver._map_batch(oc, [p(x) for x in (idk, ck, ci, kd)], 0, tb), sh, sb,
                                None if null_cut else p(cut))
        cap = len(idk) + ((len(oc) - 1) << sb)
        ko = np.zeros(len(oc), np.uint64)
        outs = [np.zeros(2 * cap + 1, np.uint64) for _ in range(7)]
        r = abi.CwMapWeftResult(ko.ctypes.data_as(abi.C.POINTER(abi.C.c_uint64)),
                                None if null_src else p(outs[0]),
                                abi.CwMapResult(cap, 0, *[p(x) for x in outs[1:]]))
        rc = weaver._L.cw_weft_maps(weaver._h, abi.C.byref(wb), abi.C.byref(r), abi.CW_MEM_HOST)
        assert rc in (0, -1)
        weaver._check(rc, "cw_weft_maps")

    raw()
    with pytest.raises(abi.WeaveError, match="cut is required"):
        raw(null_cut=True)
    with pytest.raises(abi.WeaveError, match="kept_src"):
        raw(null_src=True)
    check(weaver, "small")  # the context is still good


# ------------------------------------------------------------------ 9. the mirror
def test_mirror_weft_maps_equals_the_reference():
    items = M.mirror_items()
    pairs = [(mirror_ct(ref), ids) for ref, ids in items]
    got = C.weft_maps(pairs)
    got[0] = C.map_weft(*pairs[0])  # the one-item entry point
    checked, gibberish, bogus = check_mirror(items, got)
    assert checked > 30 and gibberish > 3 and bogus > 3, (checked, gibberish, bogus)
