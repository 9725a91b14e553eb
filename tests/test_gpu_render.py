"""cw_render_lists / cw_render_maps vs tests/render_model.py, array for array (-m gpu).

The inputs are the device arrays of the existing calls -- cw_weave_lists,
cw_merge_lists, cw_weft_lists_dev, cw_weave_maps in device memory -- handed to
the render call as they lie, so every test also shows that the calls compose
without a host round trip.  The output tensors have the header's capacity (N,
or n_segs) plus guard words and are filled beforehand: everything past the
rendered count must come back untouched.  Every comparison is equality.

The shapes are the smallest at which the kernel can go wrong, with TILE = 8,192
positions a workgroup: document boundaries inside a bitmap word, empty
documents first / last / adjacent, N no multiple of 32 with the bits past N
set, a document across four tiles, thousands of documents in one tile, more
than 130 tiles (the look-back crosses two 64-word windows) with and without a
stretch of more than 64 tiles that render nothing, repeated calls and changing
layouts on one context, perm16, every value size, the count-only call,
out-of-range indices, host memory, the error returns.
"""
import ctypes as C
import dataclasses
import functools
import random

import numpy as np
import pytest

from cause_amd import abi, causal, gen, pack
from tests import mapweft_model as MM
from tests import render_model as M
from tests import weft_model as W
from tests.test_gpu_list_merge import split_at

pytestmark = pytest.mark.gpu

TILE = 8192
GUARD = 9
FILL = {1: 0xA5, 2: 0xA5A5, 4: 0xDEADBEEF, 8: 0xDEADBEEFDEADBEEF}
UNS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SGN = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
U64 = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def weaver():
    with abi.Weaver(0) as w:
        yield w


def up(x):
    import torch

    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(SGN[x.dtype.itemsize])).to(torch.device("cuda", 0))


def down(t, dtype):
    return t.cpu().numpy().view(dtype)


def filled(n, size):
    """A device tensor of n + GUARD words of `size` bytes holding the fill pattern."""
    return up(np.full(n + GUARD, FILL[size], UNS[size]))


def dp(t):
    return t.data_ptr() if t is not None and t.numel() else 0


def last_error(w):
    return w._L.cw_last_error(w._h).decode()


# ------------------------------------------------------------------ inputs ----
@dataclasses.dataclass
class Woven:
    """A batch woven in device memory: the layout and the two result arrays the
    render reads, on the device (perm, bits) and as numpy (perm_h, bits_h)."""
    off: np.ndarray
    perm: object
    bits: object
    perm_h: np.ndarray
    bits_h: np.ndarray

    @property
    def n(self):
        return int(self.off[-1])


def weave_dev(weaver, off, idk, ck, kd, lay, ones_above=True):
    """cw_weave_lists in device memory; the bits past N of the last bitmap word
    are then set to 1 (the render must ignore them)."""
    import torch

    dev = torch.device("cuda", 0)
    N, D = len(idk), len(off) - 1
    g = [up(idk), up(ck), up(kd)]
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    o = {"weave_perm": z(N, torch.int32), "visible_bits": z((N + 31) // 32, torch.int32),
         "visible_count": z(D, torch.int32), "status": z(D, torch.int32)}
    torch.cuda.synchronize()
    weaver.weave_lists_device(off, *[dp(t) for t in g], lay, {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    st = down(o["status"], np.uint32)[:D]
    assert not (st & (abi.STATUS_DUP | abi.STATUS_INTERNAL)).any()
    return finish(off, o["weave_perm"], o["visible_bits"], ones_above)


def finish(off, perm, bits, ones_above=True):
    import torch

    off = np.ascontiguousarray(off, np.uint64)
    N = int(off[-1])
    perm, bits = perm[:max(N, 1)], bits[:max((N + 31) // 32, 1)]
    if ones_above and N % 32:
        bits[(N - 1) // 32] |= ((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF) - (1 << 32)  # (as int32)
    torch.cuda.synchronize()
    return Woven(off, perm, bits, down(perm, np.uint32)[:N], down(bits, np.uint32)[:(N + 31) // 32])


def ragged(sizes, seed, n_sites=8, spec=None):
    spec = spec or W.spec_for(n_sites, max(max(sizes) - 1, 1))
    return W.ragged(spec, list(sizes), np.random.default_rng(seed)) + (spec.layout(),)


def all_hide(off, idk, ck, kd, lay, docs):
    """Documents `docs` rewritten as the root and hides of the root: nothing of
    them renders (hide?, list.cljc:48-55)."""
    for d in docs:
        lo, n = int(off[d]), int(off[d + 1]) - int(off[d])
        idk[lo:lo + n] = [0] + [lay.pack(k, 1, 0) for k in range(1, n)]
        ck[lo:lo + n] = [pack.NIL] + [0] * (n - 1)
        kd[lo:lo + n] = [pack.KIND_ROOT] + [1] * (n - 1)


MIXED = (0, 0, 1, 31, 32, 33, 65, 0, 0, 1, 65, 33, 0)          # 262 nodes: N % 32 = 6
SPAN = (0, 33, 3 * TILE + 5, 1, 0)                             # one document across four tiles
MANY = tuple([1, 2, 0, 3, 1, 4, 0, 0, 5, 1] * 260) + (7000,)   # 2,600 documents in the first tile
BIG = (5000,) * 222                                            # 1.11e6 positions: 136 tiles


@functools.lru_cache(maxsize=None)
def batch(name):
    w = batch.weaver
    if name == "mixed":
        return weave_dev(w, *ragged(MIXED, 1))
    if name == "span":
        return weave_dev(w, *ragged(SPAN, 2))
    if name == "many":
        return weave_dev(w, *ragged(MANY, 3))
    if name == "big_hidden":  # documents 60 .. 179 render nothing: 600,000 positions, 73 tiles
        off, idk, ck, kd, lay = ragged(BIG, 4)
        all_hide(off, idk, ck, kd, lay, range(60, 180))
        return weave_dev(w, off, idk, ck, kd, lay)
    if name == "big_plain":   # no specials: everything but the roots renders
        spec = dataclasses.replace(gen.CONFIG1, nodes_per_doc=4999, shuffle=False)
        return weave_dev(w, *ragged(BIG, 5, spec=spec))
    raise KeyError(name)


@pytest.fixture(autouse=True)
def _batch_weaver(weaver):
    batch.weaver = weaver


@functools.lru_cache(maxsize=None)
def values(n, size, seed=7):
    return np.random.default_rng(seed + size).integers(1, 1 << (8 * size - 1), n, dtype=np.uint64).astype(UNS[size])


# --------------------------------------------------------------- the call ----
def render(weaver, b, value_size=0, src=True, perm16=False, memspace=abi.CW_MEM_DEVICE, value=None):
    """cw_render_lists on a Woven batch -> (offsets, src array or None, value
    array or None), the arrays whole (capacity + guard) as they came back."""
    import torch

    N = b.n
    val = value if value is not None else (values(N, value_size) if value_size else None)
    ro = np.full(len(b.off) + 1, FILL[8], np.uint64)
    if memspace == abi.CW_MEM_DEVICE:
        perm = b.perm.to(torch.int16) if perm16 else b.perm
        gv = up(val) if val is not None and len(val) else None
        osrc = filled(N, 4) if src else None
        oval = filled(N, value_size) if value_size else None
        torch.cuda.synchronize()
        bt = abi.CwRenderBatch(len(b.off) - 1, b.off.ctypes.data_as(U64), dp(perm) or None, dp(b.bits) or None,
                               int(perm16), value_size, dp(gv) or None)
        r = abi.CwRenderResult(ro.ctypes.data_as(U64), dp(osrc) or None, dp(oval) or None)
        rc = weaver._L.cw_render_lists(weaver._h, C.byref(bt), C.byref(r), memspace)
        torch.cuda.synchronize()
        hs = down(osrc, np.uint32) if src else None
        hv = down(oval, UNS[value_size]) if value_size else None
    else:
        perm = b.perm_h.astype(np.uint16) if perm16 else b.perm_h
        hs = np.full(N + GUARD, FILL[4], np.uint32) if src else None
        hv = np.full(N + GUARD, FILL[value_size], UNS[value_size]) if value_size else None
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None
        bt = abi.CwRenderBatch(len(b.off) - 1, b.off.ctypes.data_as(U64), p(perm), p(b.bits_h), int(perm16),
                               value_size, p(val))
        r = abi.CwRenderResult(ro.ctypes.data_as(U64), p(hs), p(hv))
        rc = weaver._L.cw_render_lists(weaver._h, C.byref(bt), C.byref(r), memspace)
    assert rc == 0, last_error(weaver)
    assert ro[-1] == FILL[8], "rendered_offsets written past n_docs + 1 words"
    return ro[:-1], hs, hv


def check(weaver, b, value_size=0, src=True, **kw):
    """One call == the model, and nothing written past the rendered nodes."""
    val = kw.get("value")
    if val is None and value_size:
        val = values(b.n, value_size)
    exp = M.render_lists(b.off, b.perm_h, b.bits_h, val)
    ro, hs, hv = render(weaver, b, value_size, src, **kw)
    R = int(exp.offsets[-1])
    np.testing.assert_array_equal(ro, exp.offsets)
    if src:
        np.testing.assert_array_equal(hs[:R], exp.src)
        assert (hs[R:] == FILL[4]).all(), "rendered_src written past the rendered nodes"
    if value_size:
        np.testing.assert_array_equal(hv[:R], exp.value)
        assert (hv[R:] == FILL[value_size]).all(), "rendered_value written past the rendered nodes"
    return exp


# ------------------------------------------------------------ 1. the shapes ----
@pytest.mark.parametrize("value_size", [0, 1, 2, 4, 8])
def test_boundaries_inside_a_bitmap_word(weaver, value_size):
    b = batch("mixed")
    assert b.n % 32 and b.bits_h[-1] >> (b.n % 32) == (1 << (32 - b.n % 32)) - 1  # ones past N
    exp = check(weaver, b, value_size)
    sizes = np.diff(b.off.astype(np.int64))
    counts = np.diff(exp.offsets.astype(np.int64))
    assert (counts[sizes <= 1] == 0).all() and counts.sum() > 0  # empty and root-only documents
    check(weaver, b, value_size, src=False)  # the value alone; value_size 0: the count-only call


def test_a_document_across_four_tiles(weaver):
    b = batch("span")
    assert int(b.off[2]) % TILE and int(b.off[3]) // TILE - int(b.off[2]) // TILE == 3
    check(weaver, b, 4)


def test_thousands_of_documents_in_one_tile(weaver):
    b = batch("many")
    assert np.searchsorted(b.off, TILE) > 2000 and (np.diff(b.off.astype(np.int64)) == 1).sum() > 500
    check(weaver, b, 2)
    check(weaver, b, 8)


@pytest.mark.parametrize("name", ["big_hidden", "big_plain"])
def test_look_back_over_two_windows(weaver, name):
    b = batch(name)
    assert b.n > 130 * TILE
    vis = M.flags(b.bits_h, b.n)
    if name == "big_hidden":
        lo, hi = int(b.off[60]), int(b.off[180])
        assert vis[lo:hi].sum() == 0 and hi // TILE - (lo + TILE - 1) // TILE > 64
    else:
        assert vis.sum() == b.n - (len(b.off) - 1)
    check(weaver, b, 1)


def test_repeated_calls_and_changing_layouts_on_one_context():
    """The look-back epochs, the ticket and the layout cache: the same three
    batches again and again on one context, another layout in between."""
    with abi.Weaver(0) as w:
        for name in ("big_hidden", "mixed", "big_plain", "mixed", "big_hidden", "many", "big_plain"):
            check(w, batch(name), 4)
        check(w, batch("big_plain"), 0)
        check(w, batch("big_plain"), 4)


def test_perm16_equals_u32(weaver):
    for name in ("mixed", "span", "many"):
        b = batch(name)
        a = render(weaver, b, 4)
        c = render(weaver, b, 4, perm16=True)
        for x, y in zip(a, c):
            np.testing.assert_array_equal(x, y)
        check(weaver, b, 4, perm16=True)


@pytest.mark.parametrize("name", ["mixed", "span", "many"])
def test_host_memory_equals_device_memory(weaver, name):
    b = batch(name)
    for vs in (0, 2, 8):
        check(weaver, b, vs, memspace=abi.CW_MEM_HOST)
    check(weaver, b, 4, memspace=abi.CW_MEM_HOST, perm16=True)
    check(weaver, b, 0, src=False, memspace=abi.CW_MEM_HOST)


def test_wrappers(weaver):
    b = batch("span")
    val = values(b.n, 4)
    exp = M.render_lists(b.off, b.perm_h, b.bits_h, val)
    r = weaver.render_lists(b.off, b.perm_h, b.bits_h, val)
    np.testing.assert_array_equal(r.offsets, exp.offsets)
    np.testing.assert_array_equal(r.src, exp.src)
    np.testing.assert_array_equal(r.value, exp.value)
    osrc = filled(b.n, 4)
    ro = weaver.render_lists_device(b.off, dp(b.perm), dp(b.bits), src_ptr=dp(osrc))
    np.testing.assert_array_equal(ro, exp.offsets)
    np.testing.assert_array_equal(down(osrc, np.uint32)[:len(exp.src)], exp.src)


def test_empty_batches(weaver):
    for off in ([0], [0, 0, 0]):
        b = Woven(np.array(off, np.uint64), None, None, np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        for mem in (abi.CW_MEM_HOST, abi.CW_MEM_DEVICE):
            ro, _, _ = render(weaver, b, 0, src=False, memspace=mem)
            assert not ro.any()
            ro, hs, hv = render(weaver, b, 4, memspace=mem, value=np.zeros(1, np.uint32))  # nothing is written
            assert not ro.any() and (hs == FILL[4]).all() and (hv == FILL[4]).all()
    r = weaver.render_lists([0, 0], np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert list(r.offsets) == [0, 0] and len(r.src) == 0 and len(r.value) == 0


def test_stat_names_and_bytes(weaver):
    b = batch("span")
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        exp = check(weaver, b, 2)
        st = weaver.kernel_stats()
    finally:
        weaver.set_profiling(False)
        weaver.reset_kernel_stats()
    assert {"render_lists", "render_offsets"} <= set(st)
    R = int(exp.offsets[-1])
    # perm 4 B and 1/8 B of bitmap a position; 4 + 2 B written and 2 B gathered a rendered node
    assert st["render_lists"][0] == 1 and st["render_lists"][2] == b.n * 0.125 + R * (4 + 4 + 2 + 2)


# ------------------------------------------------ 2. merge and weft outputs ----
def test_renders_a_merge_by_its_merged_offsets(weaver):
    import torch

    sizes = (40, 0, 1, 700, 65, 33)
    off, idk, ck, kd, lay = ragged(sizes, 11)
    rng = np.random.default_rng(12)
    a, bb = split_at(off, idk, ck, kd, rng, [n // 2 for n in sizes])
    dev = torch.device("cuda", 0)
    ga, gb = [up(x) for x in a[1:]], [up(x) for x in bb[1:]]
    NC, D = len(idk), len(sizes)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    o = {"weave_perm": z(NC, torch.int32), "visible_bits": z((NC + 31) // 32 + 1, torch.int32),
         "visible_count": z(D, torch.int32), "status": z(D, torch.int32)}
    src = z(NC, torch.int32)
    torch.cuda.synchronize()
    mo = weaver.merge_lists_device(a[0], [dp(t) for t in ga], bb[0], [dp(t) for t in gb], lay, src.data_ptr(),
                                   {k: v.data_ptr() for k, v in o.items()})
    assert list(np.diff(mo.astype(np.int64))) == list(sizes)
    b = finish(mo, o["weave_perm"], o["visible_bits"])
    exp = check(weaver, b, 4)
    assert list(np.diff(exp.offsets.astype(np.int64))) == list(down(o["visible_count"], np.uint32)[:D])


def test_renders_a_weft_by_its_kept_offsets(weaver):
    import torch

    off, idk, ck, kd, lay, cut = W.case_small()
    dev = torch.device("cuda", 0)
    g = [up(np.asarray(x)) for x in (idk, ck, kd)]
    gcut = up(np.asarray(cut, np.uint64))
    D, cap = len(off) - 1, len(idk) + ((len(off) - 1) << lay.site_bits)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    o = {"weave_perm": z(cap, torch.int32), "visible_bits": z((cap + 31) // 32 + 1, torch.int32),
         "visible_count": z(D, torch.int32), "status": z(D, torch.int32)}
    src = z(cap, torch.int32)
    torch.cuda.synchronize()
    ko = weaver.weft_lists_device(off, [dp(t) for t in g], lay, gcut.data_ptr(), src.data_ptr(),
                                  {k: v.data_ptr() for k, v in o.items()})
    assert 0 < int(ko[-1]) <= cap
    b = finish(ko, o["weave_perm"], o["visible_bits"])
    exp = check(weaver, b, 8)
    assert list(np.diff(exp.offsets.astype(np.int64))) == list(down(o["visible_count"], np.uint32)[:D])


# -------------------------------------------------- 3. bounds and errors ----
def test_out_of_range_weave_perm_gets_value_zero(weaver):
    """weave_perm of a DUP / INTERNAL document is unspecified: an entry at or past
    the document's size reads nothing and gets value 0."""
    b0 = batch("mixed")
    perm = b0.perm_h.copy()
    vis = M.flags(b0.bits_h, b0.n)
    hit = np.flatnonzero(vis)[[0, 5, -1]]
    doc = np.searchsorted(b0.off, hit, side="right") - 1
    size = np.diff(b0.off.astype(np.int64))[doc]
    perm[hit] = [size[0], 0xFFFFFFFF, size[2] + 40000]  # the size itself, the largest word, past N
    b = Woven(b0.off, up(perm), b0.bits, perm, b0.bits_h)
    for vs in (1, 8):
        exp = check(weaver, b, vs)
        assert (exp.value == 0).sum() == 3


def _buffers(host, arrays):
    """name -> (pointer, read-back function) of real buffers holding `arrays`, in
    device memory or (host) as numpy arrays."""
    out = {}
    for name, arr in arrays.items():
        if host:
            x = np.ascontiguousarray(arr).copy()
            out[name] = (x.ctypes.data, lambda x=x: x)
        else:
            t = up(arr)
            out[name] = (t.data_ptr(), lambda t=t, dt=arr.dtype: down(t, dt))
    return out


def raw(weaver, off, null=(), perm16=0, vs=0, memspace=abi.CW_MEM_DEVICE):
    """cw_render_lists on a real four-node batch with one thing wrong.  Every
    pointer handed over is memory of `memspace` (or NULL where `null` names
    it); the outputs hold the fill pattern.  -> (return code, the outputs as
    they came back: name -> (array, fill))."""
    import torch

    size = vs if vs in UNS else 4
    off = np.array(off, np.uint64)
    ro = np.full(max(len(off), 1) + 1, FILL[8], np.uint64)
    buf = _buffers(memspace == abi.CW_MEM_HOST, {
        "weave_perm": np.array([0, 2, 1, 0], np.uint32), "visible_bits": np.array([0xE], np.uint32),
        "value": np.arange(1, 5).astype(UNS[size]),
        "rendered_src": np.full(4 + GUARD, FILL[4], np.uint32),
        "rendered_value": np.full(4 + GUARD, FILL[size], UNS[size])})
    p = lambda name: None if name in null else C.c_void_p(buf[name][0])
    torch.cuda.synchronize()
    bt = abi.CwRenderBatch(len(off) - 1, None if "doc_offsets" in null else off.ctypes.data_as(U64),
                           p("weave_perm"), p("visible_bits"), perm16, vs, p("value"))
    r = abi.CwRenderResult(None if "rendered_offsets" in null else ro.ctypes.data_as(U64), p("rendered_src"),
                           p("rendered_value"))
    rc = weaver._L.cw_render_lists(weaver._h, None if "batch" in null else C.byref(bt),
                                   None if "result" in null else C.byref(r), memspace)
    torch.cuda.synchronize()
    return rc, {"rendered_offsets": (ro, FILL[8]), "rendered_src": (buf["rendered_src"][1](), FILL[4]),
                "rendered_value": (buf["rendered_value"][1](), FILL[size])}


def test_the_error_batch_is_valid_when_nothing_is_wrong(weaver):
    for mem in (abi.CW_MEM_DEVICE, abi.CW_MEM_HOST):
        rc, out = raw(weaver, [0, 1, 4], vs=4, memspace=mem)
        assert rc == 0, last_error(weaver)
        assert list(out["rendered_offsets"][0][:3]) == [0, 0, 3]
        assert list(out["rendered_src"][0][:3]) == [2, 1, 0] and list(out["rendered_value"][0][:3]) == [4, 3, 2]
        assert (out["rendered_src"][0][3:] == FILL[4]).all() and (out["rendered_value"][0][3:] == FILL[4]).all()


BAD = {
    "null batch": dict(off=[0, 4], null=("batch",)),
    "null result": dict(off=[0, 4], null=("result",)),
    "null rendered_offsets": dict(off=[0, 4], null=("rendered_offsets",)),
    "null doc_offsets": dict(off=[0, 4], null=("doc_offsets",)),
    "offsets start past 0": dict(off=[1, 4]),
    "offsets decrease": dict(off=[0, 9, 4]),
    "N = 2^32 - 1": dict(off=[0, 0xFFFFFFFF]),
    "value_size 3": dict(off=[0, 4], vs=3),
    "value_size 16": dict(off=[0, 4], vs=16),
    "value without rendered_value": dict(off=[0, 4], vs=4, null=("rendered_value",)),
    "rendered_value without value": dict(off=[0, 4], vs=4, null=("value",)),
    "perm16 with 65,536 nodes": dict(off=[0, 3, 65539], perm16=1),
    "null visible_bits": dict(off=[0, 4], null=("visible_bits",)),
    "null weave_perm": dict(off=[0, 4], null=("weave_perm",)),
    "null weave_perm, value asked": dict(off=[0, 4], vs=4, null=("weave_perm", "rendered_src")),
    "bad memspace": dict(off=[0, 4], memspace=2),
}


@pytest.mark.parametrize("mem", [abi.CW_MEM_DEVICE, abi.CW_MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_error_returns_write_nothing_and_the_context_lives_on(weaver, bad, mem):
    kw = dict(BAD[bad])
    kw.setdefault("memspace", mem)
    if bad == "bad memspace" and mem == abi.CW_MEM_HOST:
        kw["memspace"] = -1
    rc, out = raw(weaver, **kw)
    assert rc < 0 and last_error(weaver), bad
    for name, (arr, fill) in out.items():
        assert (arr == fill).all(), f"{name} written by a failing call ({bad})"
    check(weaver, batch("mixed"), 2)


# -------------------------------------------------------------- 4. maps ----
@dataclasses.dataclass
class WovenMaps:
    off: np.ndarray
    S: int
    coll: object
    key: object
    act: object
    coll_h: np.ndarray
    key_h: np.ndarray
    act_h: np.ndarray

    @property
    def D(self):
        return len(self.off) - 1


def weave_maps_dev(weaver, off, idk, ck, ci, kd, tb, key_bits):
    import torch

    dev = torch.device("cuda", 0)
    g = [up(x) for x in (idk, ck, ci, kd)]
    N, D = len(idk), len(off) - 1
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    o = {"seg_offsets": z(N + 1, torch.int64), "seg_coll": z(N, torch.int32), "seg_key": z(N, torch.int64),
         "seg_active": z(N, torch.int64), "seg_perm": z(2 * N, torch.int32), "status": z(D, torch.int32)}
    torch.cuda.synchronize()
    S = weaver.weave_maps_device(off, [t.data_ptr() for t in g], tb, key_bits,
                                 {k: v.data_ptr() for k, v in o.items()}, max(N, 1))
    torch.cuda.synchronize()
    return WovenMaps(np.ascontiguousarray(off, np.uint64), S, o["seg_coll"], o["seg_key"], o["seg_active"],
                     down(o["seg_coll"], np.uint32)[:S], down(o["seg_key"], np.uint64)[:S],
                     down(o["seg_active"], np.int64)[:S])


MAP_SIZES = tuple([0, 0] + [7, 0, 0, 0, 12, 1, 30, 0, 64, 3] * 30 + [0])  # 303 collections


@functools.lru_cache(maxsize=None)
def map_batch(name):
    w = batch.weaver
    if name == "ragged":  # collections 12, 22, ... hold only specials: every key of theirs is blank
        off, idk, ck, ci, kd, lay, tb = MM.ragged_maps(5, list(MAP_SIZES), 21, p_bad=0.0)
        for d in range(12, len(MAP_SIZES), 10):
            kd[int(off[d]):int(off[d + 1])] = 1
        return weave_maps_dev(w, off, idk, ck, ci, kd, tb, lay.key_bits)
    if name == "big":  # more than 130 tiles of key weaves
        spec = gen.MapSpec(nodes_per_coll=5, n_keys=256, zipf_s=0.01, p_hhide=0.0, p_hshow=0.0, p_hide=0.3,
                           seed=31)
        lay, tb = spec.layout()
        return weave_maps_dev(w, *gen.generate_maps(spec, 0, 250_000, nthreads=8), tb, lay.key_bits)
    raise KeyError(name)


def render_maps(weaver, m, value_size=0, key=True, src=True, memspace=abi.CW_MEM_DEVICE, coll=None, act=None):
    import torch

    S, D = m.S, m.D
    val = values(int(m.off[-1]), value_size, 9) if value_size else None
    eo = np.full(D + 2, FILL[8], np.uint64)
    coll_h = m.coll_h if coll is None else coll
    act_h = m.act_h if act is None else act
    if memspace == abi.CW_MEM_DEVICE:
        gc = m.coll if coll is None else up(coll)
        ga = m.act if act is None else up(act)
        gv = up(val) if value_size else None
        okey, osrc = (filled(S, 8) if key else None), (filled(S, 4) if src else None)
        oval = filled(S, value_size) if value_size else None
        ptr = lambda t: dp(t) or None
        torch.cuda.synchronize()
    else:
        gc, ga, gk, gv = coll_h, act_h, m.key_h, val
        okey = np.full(S + GUARD, FILL[8], np.uint64) if key else None
        osrc = np.full(S + GUARD, FILL[4], np.uint32) if src else None
        oval = np.full(S + GUARD, FILL[value_size], UNS[value_size]) if value_size else None
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None
    gk = m.key if memspace == abi.CW_MEM_DEVICE else m.key_h
    bt = abi.CwMapRenderBatch(D, S, ptr(gc), ptr(gk), ptr(ga), m.off.ctypes.data_as(U64) if value_size else None,
                              value_size, ptr(gv))
    r = abi.CwMapRenderResult(eo.ctypes.data_as(U64), ptr(okey), ptr(osrc), ptr(oval))
    rc = weaver._L.cw_render_maps(weaver._h, C.byref(bt), C.byref(r), memspace)
    if memspace == abi.CW_MEM_DEVICE:
        torch.cuda.synchronize()
        okey = down(okey, np.uint64) if key else None
        osrc = down(osrc, np.uint32) if src else None
        oval = down(oval, UNS[value_size]) if value_size else None
    assert eo[-1] == FILL[8]
    return rc, eo[:-1], okey, osrc, oval, val


def check_maps(weaver, m, value_size=0, key=True, src=True, **kw):
    rc, eo, okey, osrc, oval, val = render_maps(weaver, m, value_size, key, src, **kw)
    assert rc == 0, last_error(weaver)
    exp = M.render_maps(m.D, m.coll_h, m.key_h, kw.get("act", m.act_h) if kw.get("act") is not None else m.act_h,
                        m.off, val)
    R = int(exp.offsets[-1])
    np.testing.assert_array_equal(eo, exp.offsets)
    for got, want, size in ((okey, exp.key, 8), (osrc, exp.src, 4), (oval, exp.value, value_size)):
        if got is not None:
            np.testing.assert_array_equal(got[:R], want)
            assert (got[R:] == FILL[size]).all(), "an entry array written past the entries"
    return exp


@pytest.mark.parametrize("value_size", [0, 1, 2, 4, 8])
def test_map_entries_equal_the_model(weaver, value_size):
    m = map_batch("ragged")
    exp = check_maps(weaver, m, value_size)
    counts = np.diff(exp.offsets.astype(np.int64))
    segs = np.bincount(m.coll_h, minlength=m.D)
    blank = np.arange(12, m.D - 1, 10)  # (the last collection is empty)
    assert (segs[blank] > 0).all() and (counts[blank] == 0).all()  # every key blank
    assert (segs[np.array(MAP_SIZES) == 0] == 0).all() and 0 < counts.sum() < m.S
    check_maps(weaver, m, value_size, key=False, src=False)  # value_size 0: the count-only call
    check_maps(weaver, m, value_size, memspace=abi.CW_MEM_HOST)


def test_map_entries_over_130_tiles(weaver):
    m = map_batch("big")
    assert m.S > 130 * TILE
    check_maps(weaver, m, 4)
    check_maps(weaver, map_batch("ragged"), 4)
    check_maps(weaver, m, 0)


def test_entry_counts_equal_map_count(weaver):
    rng = random.Random(5)
    foo, fizz = causal.Keyword(None, "foo"), causal.Keyword(None, "fizz")
    cts = [causal.new_map_ct(rng=rng)]
    ct = causal.map_assoc(causal.map_assoc(causal.new_map_ct(rng=rng), foo, "bar"), fizz, "buzz")
    for v in (None, causal.HIDE, causal.H_SHOW, causal.HIDE):
        ct = ct if v is None else causal.append(causal.map_weave, ct, foo, v)
        cts.append(ct)
    cts.append(causal.map_dissoc(causal.map_dissoc(ct, fizz), foo))
    docs = [[(i, b[0], b[1]) for i, b in c["nodes"].items()] for c in cts]
    pm = pack.pack_maps(docs)
    res = weaver.weave_maps(pm.offsets, pm.id_key, pm.cause, pm.cause_is_id, pm.kind, pm.token_bits,
                            pm.layout.key_bits)
    r = weaver.render_maps(len(cts), res.seg_coll, res.seg_key, res.seg_active)
    woven = causal.weave_maps(cts)
    assert list(np.diff(r.offsets.astype(np.int64))) == [causal.map_count(c) for c in woven]
    assert causal.maps_to_edn(cts) == [causal.causal_map_to_edn(c) for c in woven]


def test_out_of_range_seg_active_gets_value_zero(weaver):
    m = map_batch("ragged")
    act = m.act_h.copy()
    hit = np.flatnonzero(act >= 0)[[0, 3, -1]]
    size = np.diff(m.off.astype(np.int64))[m.coll_h[hit]]
    act[hit] = [size[0], 1 << 40, 0xFFFFFFFF]
    exp = check_maps(weaver, m, 8, act=act)
    assert (exp.value == 0).sum() == 3


def test_seg_coll_out_of_order_is_an_error(weaver):
    m = map_batch("ragged")
    down_ = m.coll_h[::-1].copy()
    assert render_maps(weaver, m, 0, coll=down_)[0] < 0 and "seg_coll" in last_error(weaver)
    past = m.coll_h.copy()
    past[-1] = m.D
    assert render_maps(weaver, m, 4, coll=past)[0] < 0
    assert render_maps(weaver, m, 4, coll=past, memspace=abi.CW_MEM_HOST)[0] < 0
    check_maps(weaver, m, 4)  # the context lives on


def raw_maps(weaver, null=(), n_segs=3, vs=0, memspace=abi.CW_MEM_DEVICE):
    """cw_render_maps on a real batch of two collections and three key weaves
    with one thing wrong: every pointer is memory of `memspace` or NULL, the
    outputs hold the fill pattern.  -> (return code, name -> (array, fill))."""
    import torch

    size = vs if vs in UNS else 4
    off = np.array([0, 2, 5], np.uint64)
    eo = np.full(4, FILL[8], np.uint64)
    buf = _buffers(memspace == abi.CW_MEM_HOST, {
        "seg_coll": np.array([0, 0, 1], np.uint32), "seg_key": np.array([5, 6, 5], np.uint64),
        "seg_active": np.array([1, -1, 2], np.int64), "value": np.arange(1, 6).astype(UNS[size]),
        "entry_key": np.full(3 + GUARD, FILL[8], np.uint64), "entry_src": np.full(3 + GUARD, FILL[4], np.uint32),
        "entry_value": np.full(3 + GUARD, FILL[size], UNS[size])})
    p = lambda name: None if name in null else C.c_void_p(buf[name][0])
    torch.cuda.synchronize()
    bt = abi.CwMapRenderBatch(2, n_segs, p("seg_coll"), p("seg_key"), p("seg_active"),
                              None if "coll_offsets" in null else off.ctypes.data_as(U64), vs, p("value"))
    r = abi.CwMapRenderResult(None if "entry_offsets" in null else eo.ctypes.data_as(U64), p("entry_key"),
                              p("entry_src"), p("entry_value"))
    rc = weaver._L.cw_render_maps(weaver._h, None if "batch" in null else C.byref(bt),
                                  None if "result" in null else C.byref(r), memspace)
    torch.cuda.synchronize()
    return rc, {"entry_offsets": (eo, FILL[8]), "entry_key": (buf["entry_key"][1](), FILL[8]),
                "entry_src": (buf["entry_src"][1](), FILL[4]), "entry_value": (buf["entry_value"][1](), FILL[size])}


MAP_BAD = {
    "null batch": dict(null=("batch",)),
    "null result": dict(null=("result",)),
    "null entry_offsets": dict(null=("entry_offsets",)),
    "value_size 5": dict(vs=5),
    "value without entry_value": dict(vs=4, null=("entry_value",)),
    "entry_value without value": dict(vs=4, null=("value",)),
    "null seg_coll": dict(null=("seg_coll",)),
    "null seg_active": dict(null=("seg_active",)),
    "null seg_key, entry_key asked": dict(null=("seg_key",)),
    "n_segs = 2^32 - 1": dict(n_segs=0xFFFFFFFF),
    "null coll_offsets with a value column": dict(vs=2, null=("coll_offsets",)),
    "bad memspace": dict(memspace=7),
}


@pytest.mark.parametrize("mem", [abi.CW_MEM_DEVICE, abi.CW_MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("bad", sorted(MAP_BAD))
def test_map_error_returns_write_nothing(weaver, bad, mem):
    kw = dict(MAP_BAD[bad])
    kw.setdefault("memspace", mem)
    rc, out = raw_maps(weaver, **kw)
    assert rc < 0 and last_error(weaver), bad
    for name, (arr, fill) in out.items():
        assert (arr == fill).all(), f"{name} written by a failing call ({bad})"


@pytest.mark.parametrize("mem", [abi.CW_MEM_DEVICE, abi.CW_MEM_HOST], ids=["device", "host"])
def test_the_map_error_batch_is_valid_when_nothing_is_wrong(weaver, mem):
    rc, out = raw_maps(weaver, vs=4, memspace=mem)
    assert rc == 0, last_error(weaver)
    assert list(out["entry_offsets"][0][:3]) == [0, 1, 2] and out["entry_offsets"][0][3] == FILL[8]
    assert list(out["entry_key"][0][:2]) == [5, 5] and list(out["entry_src"][0][:2]) == [1, 2]
    assert list(out["entry_value"][0][:2]) == [2, 5]
    for name in ("entry_key", "entry_src", "entry_value"):
        assert (out[name][0][2:] == out[name][1]).all()
    rc, out = raw_maps(weaver, null=("seg_key", "entry_key", "entry_src"), memspace=mem)  # the count-only call
    assert rc == 0 and list(out["entry_offsets"][0][:3]) == [0, 1, 2]


# ------------------------------------------------------ 5. the mirror ----
def test_lists_to_edn_equals_the_existing_path():
    from tests.test_golden import EDGE, case_nodes

    cts = []
    for ci, c in enumerate(EDGE["cases"]):
        nodes = case_nodes(c)
        random.Random(ci).shuffle(nodes)
        ct = causal.new_list_ct(rng=random.Random(ci))
        ct["nodes"] = {n[0]: (n[1], n[2]) for n in nodes}
        cts.append(ct)
    cts.insert(2, causal.new_list_ct(rng=random.Random(99)))
    want = [causal.causal_list_to_edn(c) for c in causal.weave_lists(cts)]
    assert causal.lists_to_edn(cts) == want  # every value a character: the code-point column
    assert want[0] == EDGE["cases"][0]["edn"]
    ct = causal.new_list_ct(rng=random.Random(3))
    for v in ("a", 17, ("x", "y"), "bc"):
        ct = causal.list_conj(ct, v)
    hidden = causal.append(causal.list_weave, ct, ct["weave"][1][0], causal.HIDE)
    mixed = [ct, hidden] + cts[:3]
    assert causal.lists_to_edn(mixed) == [causal.causal_list_to_edn(c) for c in causal.weave_lists(mixed)]
    assert causal.lists_to_edn(mixed)[1] == [17, ("x", "y"), "bc"]


def test_lists_to_edn_with_ids_past_63_bits():
    """lists_to_edn packs ids over 63 bits as K128 by itself, as weave_lists does."""
    from oracle import causal_ref as R
    from tests import refgen as G
    from tests.test_gpu_k128 import widen

    rng = random.Random(133)
    nodes, _ = G.random_history(rng, 40)
    wide = widen([R.ROOT_NODE] + nodes, rng, (1 << 62) + 7)
    with pytest.raises(pack.KeyRangeError):
        pack.pack_lists([wide])
    ct = causal.new_list_ct()
    ct["nodes"] = {n[0]: (n[1], n[2]) for n in wide}
    ref = R.new_list_ct()
    ref["nodes"] = dict(ct["nodes"])
    want = R.causal_list_to_edn(R.list_weave(ref))
    assert want and causal.lists_to_edn([ct, causal.new_list_ct()]) == [want, []]
