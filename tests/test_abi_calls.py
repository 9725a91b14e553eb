"""The Weaver wrappers against a stub in place of libcauseweave.so (no GPU).

Every call method is run with a stub `_L` that records the C function, the
structs behind its byref arguments and the memspace, and plays the library's
part in host memory: it writes the offsets a call returns, n_segs, and a known
pattern into every output buffer.  Pinned per call: the function and memspace,
every scalar field, NULL or not for every pointer field, the pointer values
the device forms pass through, the capacity of every buffer the host forms
allocate, and dtype, length and contents of every returned array.
(Weaver.sort_keys, the host form, makes torch device tensors: it stays with the
GPU suite; sort_keys_device is here.)
"""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest

from cause_amd import abi

U8, U16, U32, U64, I64 = np.uint8, np.uint16, np.uint32, np.uint64, np.int64
LAY2 = NS(key_bits=40, ts_shift=20, site_shift=18, site_bits=2)
LAY0 = NS(key_bits=33, ts_shift=12, site_shift=9, site_bits=0)
LIST_FIELDS = ("weave_perm", "visible_bits", "visible_count", "max_ts", "status", "yarn_perm")
MAP_FIELDS = ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm", "status")
# what the stub writes: field -> (dtype, first value)
LIST_PAT = {"weave_perm": (U32, 100), "visible_bits": (U32, 0xB0), "visible_count": (U32, 10),
            "max_ts": (U64, 1000), "status": (U32, 3), "yarn_perm": (U32, 200)}
MAP_PAT = {"seg_offsets": (U64, 2), "seg_coll": (U32, 5), "seg_key": (U64, 70),
           "seg_active": (I64, -1), "seg_perm": (U32, 300), "status": (U32, 40)}


def pat(table, field, n):
    dt, first = table[field]
    return (np.arange(n, dtype=np.int64) + first).astype(dt)


def rd(addr, dtype, n):
    """Copy n elements out of host memory at addr."""
    nbytes = n * np.dtype(dtype).itemsize
    if not nbytes:
        return np.zeros(0, dtype)
    return np.frombuffer((C.c_char * nbytes).from_address(addr), dtype).copy()


def wr(addr, values):
    """Write an array into host memory at addr."""
    v = np.ascontiguousarray(values)
    if v.nbytes:
        np.frombuffer((C.c_char * v.nbytes).from_address(addr), v.dtype)[:] = v


def snap(s):
    """A struct as {field: int, None for NULL, or a dict for a nested struct}."""
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out[name] = snap(v)
        elif v is None or isinstance(v, int):
            out[name] = v
        else:  # a typed pointer
            out[name] = C.cast(v, C.c_void_p).value
    return out


class Call:
    def __init__(self, name, args):
        self.name, self.h = name, args[0]
        self.structs = [a._obj for a in args[1:] if hasattr(a, "_obj")]
        self.types = [type(s) for s in self.structs]
        self.snaps = [snap(s) if isinstance(s, C.Structure) else s for s in self.structs]
        self.plain = [a for a in args[1:] if not hasattr(a, "_obj")]
        self.seen = {}  # what the play function read from the inputs


class Stub:
    """Stands in for the loaded library: records calls, then lets `play` write
    the outputs.  play(call) may return the C function's return value."""

    def __init__(self, play=None):
        self.calls, self.play = [], play

    def __getattr__(self, name):
        if not name.startswith("cw_"):
            raise AttributeError(name)

        def fn(*args):
            call = Call(name, args)
            self.calls.append(call)
            rc = self.play(call) if self.play else None
            return 0 if rc is None else rc
        return fn


H = C.c_void_p(0xC0DE)


@pytest.fixture
def weaver():
    w = object.__new__(abi.Weaver)
    w._L, w._h, w.device = Stub(), H, 0
    yield w
    w._h = None  # close() then calls nothing


def one_call(w, name, memspace="none"):
    assert [c.name for c in w._L.calls] == [name]
    call = w._L.calls[0]
    assert call.h is H
    if memspace == "none":
        assert call.plain == []
    elif memspace is not ...:
        assert call.plain == [memspace]
    return call


def fill_list(r, M, W, D):
    """The library's writes into a host cw_list_result: M nodes, W bitmap words, D documents."""
    sizes = {"weave_perm": M, "visible_bits": W, "visible_count": D, "max_ts": D, "status": D,
             "yarn_perm": M}
    for f in LIST_FIELDS:
        if r[f] is not None:
            wr(r[f], pat(LIST_PAT, f, sizes[f]))


def fill_map(r, S, P, D):
    sizes = {"seg_offsets": S + 1, "seg_coll": S, "seg_key": S, "seg_active": S, "seg_perm": P,
             "status": D}
    for f in MAP_FIELDS:
        wr(r[f], pat(MAP_PAT, f, sizes[f]))


def cap(a):
    """Elements of the buffer a returned array lies in."""
    return len(a) if a.base is None else len(a.base)


def same(a, want):
    assert a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want), (a, want)


def check_list(res, M, W, D, yarns, caps):
    """A returned ListResult: patterns trimmed to (M, W, D), buffers of caps =
    (per node, bitmap words, per document)."""
    sizes = {"weave_perm": M, "visible_bits": W, "visible_count": D, "max_ts": D, "status": D,
             "yarn_perm": M}
    kinds = {"weave_perm": 0, "visible_bits": 1, "visible_count": 2, "max_ts": 2, "status": 2,
             "yarn_perm": 0}
    for f in LIST_FIELDS:
        a = getattr(res, f)
        if f == "yarn_perm" and not yarns:
            assert a is None
            continue
        same(a, pat(LIST_PAT, f, sizes[f]))
        assert cap(a) == caps[kinds[f]], f


def check_map(res, S, P, D, caps):
    """A returned MapResult; caps = (cap_segs, seg_perm elements, status elements)."""
    sizes = {"seg_offsets": S + 1, "seg_coll": S, "seg_key": S, "seg_active": S, "seg_perm": P,
             "status": D}
    want = {"seg_offsets": caps[0] + 1, "seg_coll": caps[0], "seg_key": caps[0],
            "seg_active": caps[0], "seg_perm": caps[1], "status": caps[2]}
    for f in MAP_FIELDS:
        a = getattr(res, f)
        same(a, pat(MAP_PAT, f, sizes[f]))
        assert cap(a) == want[f], f


def nulls(s):
    return {k for k, v in s.items() if v is None}


OFF = [0, 20, 20, 32]  # three documents, the middle one empty; N a multiple of 32
N, D = 32, 3


def nodes(n, dt=U64):
    return (np.arange(n, dtype=dt) + dt(7), np.arange(n, dtype=dt) * dt(3), (np.arange(n) % 5).astype(U8))


def read_list_batch(call, dt=U64, width=1):
    """The play side of a host list batch: copy what the pointers hold."""
    b = call.snaps[0]
    b = b.get("nodes", b)
    off = rd(b["doc_offsets"], U64, b["n_docs"] + 1)
    n = int(off[-1])
    call.seen = {"off": off, "id": rd(b["id_key"], dt, n * width),
                 "cause": rd(b["cause_key"], dt, n * width), "kind": rd(b["kind"], U8, n)}


# ------------------------------------------------------------------ list weaves
@pytest.mark.parametrize("form", ["k64", "k32"])
@pytest.mark.parametrize("lay,yarns,key_bits", [(LAY2, True, None), (LAY2, False, 7),
                                                (LAY0, True, None)])
def test_weave_lists_host(weaver, form, lay, yarns, key_bits):
    dt = U64 if form == "k64" else U32
    i, c, k = nodes(N, dt)

    def play(call):
        read_list_batch(call, dt)
        fill_list(call.snaps[1], N, 1, D)
    weaver._L.play = play
    fn = weaver.weave_lists if form == "k64" else weaver.weave_lists_k32
    res = fn(OFF, i, c, k, lay, yarns, key_bits)
    call = one_call(weaver, "cw_weave_lists" if form == "k64" else "cw_weave_lists_k32",
                    abi.CW_MEM_HOST)
    assert call.types == [abi.CwListBatch if form == "k64" else abi.CwListBatchK32,
                          abi.CwListResult]
    b, r = call.snaps
    want = {"n_docs": D, "key_bits": lay.key_bits if key_bits is None else key_bits,
            "ts_shift": lay.ts_shift, "site_shift": lay.site_shift, "site_bits": lay.site_bits}
    if form == "k32":
        want["perm16"] = 0
    assert {f: b[f] for f in want} == want and len(b) == len(want) + 4
    assert nulls(b) == set()
    assert (b["id_key"], b["cause_key"], b["kind"]) == (i.ctypes.data, c.ctypes.data,
                                                        k.ctypes.data)
    same(call.seen["off"], np.array(OFF, U64))
    has_yarn = bool(yarns and lay.site_bits)
    assert nulls(r) == (set() if has_yarn else {"yarn_perm"})
    assert isinstance(res, abi.ListResult)
    check_list(res, N, 1, D, has_yarn, (N, 1, D))


def test_weave_lists_host_converts_and_checks(weaver):
    weaver._L.play = lambda call: read_list_batch(call)
    i, c, k = nodes(5)
    weaver.weave_lists([0, 3, 3, 5], list(map(int, i)), c.astype(np.int64), list(map(int, k)), LAY2)
    seen = weaver._L.calls[0].seen
    same(seen["id"], i), same(seen["cause"], c), same(seen["kind"], k)
    with pytest.raises(ValueError):
        weaver.weave_lists([0, 3, 3, 6], i, c, k, LAY2)
    for bad in ((i[:4], c, k), (i, c[:4], k), (i, c, k[:4])):
        with pytest.raises(ValueError):
            weaver.weave_lists_k32([0, 3, 3, 5], *bad, LAY2)
    assert len(weaver._L.calls) == 1


@pytest.mark.parametrize("yarns", [True, False])
def test_weave_lists_k128_host(weaver, yarns):
    i = np.arange(2 * N, dtype=U64).reshape(N, 2) + U64(9)
    c = i * U64(2)
    k = nodes(N)[2]

    def play(call):
        read_list_batch(call, U64, 2)
        fill_list(call.snaps[1], N, 1, D)
    weaver._L.play = play
    res = weaver.weave_lists_k128(OFF, i.ravel(), c, k, yarns)
    call = one_call(weaver, "cw_weave_lists_k128", abi.CW_MEM_HOST)
    assert call.types == [abi.CwListBatchK128, abi.CwListResult]
    b, r = call.snaps
    assert b["n_docs"] == D and nulls(b) == set() and len(b) == 5
    same(call.seen["id"], i.ravel()), same(call.seen["cause"], c.ravel())
    same(call.seen["kind"], k)
    assert nulls(r) == (set() if yarns else {"yarn_perm"})
    check_list(res, N, 1, D, yarns, (N, 1, D))
    for bad in ((i[:4], c, k), (i, c[:4], k), (i, c, k[:4])):
        with pytest.raises(ValueError):
            weaver.weave_lists_k128(OFF, *bad)
    with pytest.raises(ValueError):
        weaver.weave_lists_k128([0, 20, 20, 31], i, c, k)


OUT6 = {f: 0x9000 + 0x100 * n for n, f in enumerate(LIST_FIELDS)}
OUT_SPARSE = {"weave_perm": 0x9000, "visible_bits": None, "visible_count": 0x9200, "status": 0x9400,
              "yarn_perm": 0}  # no max_ts key, a None and a 0: all NULL


def list_out_want(out_ptrs, never=()):
    return {f: (None if f in never else out_ptrs.get(f) or None) for f in LIST_FIELDS}


@pytest.mark.parametrize("out_ptrs", [OUT6, OUT_SPARSE])
@pytest.mark.parametrize("form", ["k64", "k32", "k32p16", "k128"])
def test_weave_lists_device(weaver, form, out_ptrs):
    weaver._L.play = lambda call: call.seen.update(
        off=rd(call.snaps[0]["doc_offsets"], U64, D + 1))
    if form == "k64":
        ret = weaver.weave_lists_device(OFF, 0x1000, 0x2000, 0x3000, LAY2, out_ptrs, key_bits=9)
        name, cls, extra = "cw_weave_lists", abi.CwListBatch, {"key_bits": 9}
    elif form == "k32":
        ret = weaver.weave_lists_k32_device(OFF, 0x1000, 0x2000, 0x3000, LAY2, out_ptrs)
        name, cls, extra = "cw_weave_lists_k32", abi.CwListBatchK32, {"key_bits": 40, "perm16": 0}
    elif form == "k32p16":
        ret = weaver.weave_lists_k32_device(OFF, 0x1000, 0x2000, 0x3000, LAY2, out_ptrs, 11, True)
        name, cls, extra = "cw_weave_lists_k32", abi.CwListBatchK32, {"key_bits": 11, "perm16": 1}
    else:
        ret = weaver.weave_lists_k128_device(OFF, 0x1000, 0x2000, 0x3000, out_ptrs)
        name, cls, extra = "cw_weave_lists_k128", abi.CwListBatchK128, None
    assert ret is None
    call = one_call(weaver, name, abi.CW_MEM_DEVICE)
    assert call.types == [cls, abi.CwListResult]
    b, r = call.snaps
    want = {"n_docs": D, "id_key": 0x1000, "cause_key": 0x2000, "kind": 0x3000}
    if extra is not None:
        want.update(extra, ts_shift=20, site_shift=18, site_bits=2)
    assert {f: b[f] for f in want} == want and len(b) == len(want) + 1
    same(call.seen["off"], np.array(OFF, U64))
    assert r == list_out_want(out_ptrs)


@pytest.mark.parametrize("form", ["ranked", "linked"])
@pytest.mark.parametrize("out_ptrs", [OUT6, OUT_SPARSE])
def test_weave_ranked_and_linked_device(weaver, form, out_ptrs):
    if form == "ranked":
        weaver.weave_ranked_device(77, 0x1000, 0x2000, 0x3000, out_ptrs)
        call = one_call(weaver, "cw_weave_ranked")
        assert call.types == [abi.CwRankedList, abi.CwListResult]
        assert call.snaps[0] == {"n": 77, "par": 0x1000, "kind": 0x2000, "val": 0x3000}
    else:
        weaver.weave_linked_device(77, 0x1000, 0x2000, None, out_ptrs)
        call = one_call(weaver, "cw_weave_linked")
        assert call.types == [abi.CwLinkedList, abi.CwListResult]
        assert call.snaps[0] == {"n": 77, "succ": 0x1000, "thr": 0x2000, "val": None}
    assert call.snaps[1] == list_out_want(out_ptrs, never=("max_ts", "yarn_perm"))


# ------------------------------------------------------------------- list merge
A_OFF, B_OFF, M_OFF = [0, 20, 20, 30], [0, 10, 10, 13], [0, 24, 24, 32]  # 43 nodes in, 32 merged


@pytest.mark.parametrize("lay,yarns", [(LAY2, True), (LAY2, False), (LAY0, True)])
def test_merge_lists_host(weaver, lay, yarns):
    a = (A_OFF,) + nodes(30) + (np.arange(30, dtype=U64) + U64(500),)
    b = (B_OFF,) + nodes(13) + (np.arange(13, dtype=U64) + U64(900),)

    def play(call):
        mb, r = call.snaps
        for side in "ab":
            s = mb[side]
            off = rd(s["doc_offsets"], U64, s["n_docs"] + 1)
            call.seen[side] = (off, rd(s["id_key"], U64, int(off[-1])),
                               rd(s["cause_key"], U64, int(off[-1])),
                               rd(s["kind"], U8, int(off[-1])),
                               rd(mb[side + "_value"], U64, int(off[-1])))
        wr(r["merged_offsets"], np.array(M_OFF, U64))
        wr(r["merged_src"], np.arange(32, dtype=U32) + U32(600))
        fill_list(r["weave"], 32, 1, D)
    weaver._L.play = play
    res = weaver.merge_lists(a, b, lay, yarns)
    call = one_call(weaver, "cw_merge_lists", abi.CW_MEM_HOST)
    assert call.types == [abi.CwMergeBatch, abi.CwMergeResult]
    mb, r = call.snaps
    for side, t in (("a", a), ("b", b)):
        s = mb[side]
        assert {f: s[f] for f in ("n_docs", "key_bits", "ts_shift", "site_shift", "site_bits")} == {
            "n_docs": D, "key_bits": lay.key_bits, "ts_shift": lay.ts_shift,
            "site_shift": lay.site_shift, "site_bits": lay.site_bits}
        assert nulls(s) == set() and mb[side + "_value"] is not None
        for got, want in zip(call.seen[side], t):
            same(got, np.asarray(want, got.dtype))
    has_yarn = bool(yarns and lay.site_bits)
    assert r["merged_offsets"] and r["merged_src"]
    assert nulls(r["weave"]) == (set() if has_yarn else {"yarn_perm"})
    assert isinstance(res, abi.MergeResult)
    same(res.offsets, np.array(M_OFF, U64))
    same(res.src, np.arange(32, dtype=U32) + U32(600))
    assert cap(res.src) == 43
    check_list(res.weave, 32, 1, D, has_yarn, (43, (43 + 31) // 32 + 1, D))


def test_merge_lists_host_floors_and_errors(weaver):
    empty = ([0], [], [], [], [])
    weaver._L.play = lambda call: None
    res = weaver.merge_lists(empty, empty, LAY2)
    same(res.offsets, np.zeros(1, U64))
    assert len(res.src) == 0 and cap(res.src) == 1
    w = res.weave
    assert [len(getattr(w, f)) for f in LIST_FIELDS] == [0] * 6
    assert [cap(getattr(w, f)) for f in LIST_FIELDS] == [1, 1, 1, 1, 1, 1]
    assert [getattr(w, f).dtype for f in LIST_FIELDS] == [U32, U32, U32, U64, U32, U32]
    i, c, k = nodes(5)
    v = np.zeros(5, U64)
    with pytest.raises(ValueError):
        weaver.merge_lists(([0, 5], i, c, k, v), ([0, 2, 5], i, c, k, v), LAY2)
    with pytest.raises(ValueError):
        weaver.merge_lists(([0, 4], i, c, k, v), ([0, 5], i, c, k, v), LAY2)
    assert len(weaver._L.calls) == 1


@pytest.mark.parametrize("out_ptrs", [OUT6, OUT_SPARSE])
def test_merge_lists_device(weaver, out_ptrs):
    def play(call):
        mb, r = call.snaps
        call.seen = {s: rd(mb[s]["doc_offsets"], U64, D + 1) for s in "ab"}
        wr(r["merged_offsets"], np.array(M_OFF, U64))
    weaver._L.play = play
    mo = weaver.merge_lists_device(A_OFF, (0x1000, 0x1100, 0x1200, 0x1300), B_OFF,
                                   (0x2000, 0x2100, 0, None), LAY2, 0x7000, out_ptrs)
    call = one_call(weaver, "cw_merge_lists", abi.CW_MEM_DEVICE)
    assert call.types == [abi.CwMergeBatch, abi.CwMergeResult]
    mb, r = call.snaps
    lay = {"key_bits": 40, "ts_shift": 20, "site_shift": 18, "site_bits": 2}
    off_a, off_b = mb["a"].pop("doc_offsets"), mb["b"].pop("doc_offsets")
    assert off_a and off_b
    assert mb == {"a": dict(lay, n_docs=D, id_key=0x1000, cause_key=0x1100, kind=0x1200),
                  "a_value": 0x1300,
                  "b": dict(lay, n_docs=D, id_key=0x2000, cause_key=0x2100, kind=None),
                  "b_value": None}
    same(call.seen["a"], np.array(A_OFF, U64)), same(call.seen["b"], np.array(B_OFF, U64))
    assert r["merged_src"] == 0x7000 and r["weave"] == list_out_want(out_ptrs)
    same(mo, np.array(M_OFF, U64))
    with pytest.raises(ValueError):
        weaver.merge_lists_device(A_OFF, (1, 2, 3, 4), [0, 13], (1, 2, 3, 4), LAY2, 5, OUT6)
    assert len(weaver._L.calls) == 1


# -------------------------------------------------------------------- list weft
K_OFF = [0, 10, 10, 33]  # more kept nodes than inputs: [id] nodes


@pytest.mark.parametrize("lay,yarns", [(LAY2, True), (LAY2, False), (LAY0, True)])
def test_weft_lists_host(weaver, lay, yarns):
    i, c, k = nodes(N)
    cut = np.arange(D << lay.site_bits, dtype=U64) + U64(50)
    room = N + (D << lay.site_bits)  # 44 or 35

    def play(call):
        read_list_batch(call)
        wb, r = call.snaps
        call.seen["cut"] = rd(wb["cut"], U64, D << lay.site_bits)
        wr(r["kept_offsets"], np.array(K_OFF, U64))
        wr(r["kept_src"], np.arange(33, dtype=U32) + U32(600))
        fill_list(r["weave"], 33, 2, D)
    weaver._L.play = play
    res = weaver.weft_lists(OFF, i, c, k, lay, list(map(int, cut)), yarns)
    call = one_call(weaver, "cw_weft_lists", abi.CW_MEM_HOST)
    assert call.types == [abi.CwWeftBatch, abi.CwWeftResult]
    wb, r = call.snaps
    s = wb["nodes"]
    assert {f: s[f] for f in ("n_docs", "key_bits", "ts_shift", "site_shift", "site_bits")} == {
        "n_docs": D, "key_bits": lay.key_bits, "ts_shift": lay.ts_shift,
        "site_shift": lay.site_shift, "site_bits": lay.site_bits}
    assert nulls(s) == set() and wb["cut"]
    same(call.seen["off"], np.array(OFF, U64)), same(call.seen["id"], i)
    same(call.seen["cause"], c), same(call.seen["kind"], k), same(call.seen["cut"], cut)
    has_yarn = bool(yarns and lay.site_bits)
    assert r["kept_offsets"] and r["kept_src"]
    assert nulls(r["weave"]) == (set() if has_yarn else {"yarn_perm"})
    assert isinstance(res, abi.MergeResult)
    same(res.offsets, np.array(K_OFF, U64))
    same(res.src, np.arange(33, dtype=U32) + U32(600))
    assert cap(res.src) == room
    check_list(res.weave, 33, 2, D, has_yarn, (room, (room + 31) // 32 + 1, D))


def test_weft_lists_host_floors_and_errors(weaver):
    weaver._L.play = lambda call: None
    res = weaver.weft_lists([0], [], [], [], LAY2, [])
    same(res.offsets, np.zeros(1, U64))
    assert len(res.src) == 0 and cap(res.src) == 1
    assert [cap(getattr(res.weave, f)) for f in LIST_FIELDS] == [1, 2, 1, 1, 1, 1]
    i, c, k = nodes(N)
    with pytest.raises(ValueError):
        weaver.weft_lists(OFF, i, c, k, LAY2, np.zeros(11, U64))
    with pytest.raises(ValueError):
        weaver.weft_lists([0, 20, 20, 31], i, c, k, LAY2, np.zeros(12, U64))
    assert len(weaver._L.calls) == 1


@pytest.mark.parametrize("out_ptrs", [OUT6, OUT_SPARSE])
def test_weft_lists_device(weaver, out_ptrs):
    def play(call):
        call.seen["off"] = rd(call.snaps[0]["nodes"]["doc_offsets"], U64, D + 1)
        wr(call.snaps[1]["kept_offsets"], np.array(K_OFF, U64))
    weaver._L.play = play
    ko = weaver.weft_lists_device(OFF, (0x1000, 0x1100, 0x1200), LAY2, 0x5000, 0x7000, out_ptrs)
    call = one_call(weaver, "cw_weft_lists_dev")
    assert call.types == [abi.CwWeftBatch, abi.CwWeftResult]
    wb, r = call.snaps
    assert wb["nodes"].pop("doc_offsets")
    assert wb == {"nodes": {"n_docs": D, "id_key": 0x1000, "cause_key": 0x1100, "kind": 0x1200,
                            "key_bits": 40, "ts_shift": 20, "site_shift": 18, "site_bits": 2},
                  "cut": 0x5000}
    same(call.seen["off"], np.array(OFF, U64))
    assert r["kept_src"] == 0x7000 and r["weave"] == list_out_want(out_ptrs)
    same(ko, np.array(K_OFF, U64))


# ------------------------------------------------------------------------- maps
C_OFF = [0, 3, 3, 5]


def map_nodes(n):
    i, c, k = nodes(n)
    return i, c, (np.arange(n) % 3).astype(U8), k


def read_map_batch(b):
    off = rd(b["coll_offsets"], U64, b["n_colls"] + 1)
    n = int(off[-1])
    return (off, rd(b["id_key"], U64, n), rd(b["cause"], U64, n), rd(b["cause_is_id"], U8, n),
            rd(b["kind"], U8, n))


MOUT = {f: 0xA000 + 0x100 * n for n, f in enumerate(MAP_FIELDS)}


def test_weave_maps_host(weaver):
    cols = map_nodes(5)

    def play(call):
        call.seen["in"] = read_map_batch(call.snaps[0])
        call.structs[1].n_segs = 2
        fill_map(call.snaps[1], 2, 7, D)
    weaver._L.play = play
    res = weaver.weave_maps(C_OFF, *cols, token_bits=13, key_bits=21)
    call = one_call(weaver, "cw_weave_maps", abi.CW_MEM_HOST)
    assert call.types == [abi.CwMapBatch, abi.CwMapResult]
    b, r = call.snaps
    assert (b["n_colls"], b["key_bits"], b["token_bits"]) == (D, 21, 13) and nulls(b) == set()
    for got, want in zip(call.seen["in"], (np.array(C_OFF, U64),) + cols):
        same(got, want)
    assert (r["cap_segs"], r["n_segs"]) == (5, 0) and nulls(r) == set()
    assert isinstance(res, abi.MapResult)
    check_map(res, 2, 7, D, (5, 10, D))
    weaver.weave_maps(C_OFF, *cols, token_bits=13)
    assert weaver._L.calls[1].snaps[0]["key_bits"] == 0
    with pytest.raises(ValueError):
        weaver.weave_maps([0, 3, 3, 4], *cols, token_bits=13)
    # no collection at all: the floors of one element
    weaver._L.play = lambda call: None
    res = weaver.weave_maps([0], [], [], [], [], 13)
    assert [cap(getattr(res, f)) for f in MAP_FIELDS] == [2, 1, 1, 1, 1, 1]
    assert [len(getattr(res, f)) for f in MAP_FIELDS] == [1, 0, 0, 0, 0, 0]
    assert weaver._L.calls[2].snaps[1]["cap_segs"] == 1


def test_weave_maps_device(weaver):
    def play(call):
        call.seen["off"] = rd(call.snaps[0]["coll_offsets"], U64, D + 1)
        call.structs[1].n_segs = 4
    weaver._L.play = play
    S = weaver.weave_maps_device(C_OFF, (0x1000, 0x1100, 0x1200, 0x1300), 13, 21, MOUT, 99)
    call = one_call(weaver, "cw_weave_maps", abi.CW_MEM_DEVICE)
    assert call.types == [abi.CwMapBatch, abi.CwMapResult]
    b, r = call.snaps
    assert b.pop("coll_offsets")
    assert b == {"n_colls": D, "id_key": 0x1000, "cause": 0x1100, "cause_is_id": 0x1200,
                 "kind": 0x1300, "key_bits": 21, "token_bits": 13}
    same(call.seen["off"], np.array(C_OFF, U64))
    assert r == dict(MOUT, cap_segs=99, n_segs=0)
    assert S == 4 and type(S) is int


CA_OFF, CB_OFF, CM_OFF = [0, 3, 3, 5], [0, 2, 2, 3], [0, 4, 4, 6]  # 8 nodes in, 6 merged


def test_merge_maps_host(weaver):
    a = (CA_OFF,) + map_nodes(5) + (np.arange(5, dtype=U64) + U64(500),)
    b = (CB_OFF,) + map_nodes(3) + (np.arange(3, dtype=U64) + U64(900),)

    def play(call):
        mb, r = call.snaps
        for side in "ab":
            got = read_map_batch(mb[side])
            call.seen[side] = got + (rd(mb[side + "_value"], U64, len(got[1])),)
        wr(r["merged_offsets"], np.array(CM_OFF, U64))
        wr(r["merged_src"], np.arange(6, dtype=U32) + U32(600))
        call.structs[1].maps.n_segs = 3
        fill_map(r["maps"], 3, 9, D)
    weaver._L.play = play
    res = weaver.merge_maps(a, b, token_bits=13, key_bits=21)
    call = one_call(weaver, "cw_merge_maps", abi.CW_MEM_HOST)
    assert call.types == [abi.CwMapMergeBatch, abi.CwMapMergeResult]
    mb, r = call.snaps
    for side, t in (("a", a), ("b", b)):
        s = mb[side]
        assert (s["n_colls"], s["key_bits"], s["token_bits"]) == (D, 21, 13)
        assert nulls(s) == set() and mb[side + "_value"]
        for got, want in zip(call.seen[side], t):
            same(got, np.asarray(want, got.dtype))
    assert r["merged_offsets"] and r["merged_src"]
    assert (r["maps"]["cap_segs"], r["maps"]["n_segs"]) == (8, 0) and nulls(r["maps"]) == set()
    assert isinstance(res, abi.MapMergeResult)
    same(res.offsets, np.array(CM_OFF, U64))
    same(res.src, np.arange(6, dtype=U32) + U32(600))
    assert cap(res.src) == 8
    check_map(res.maps, 3, 9, D, (8, 16, D))
    assert weaver.merge_maps(a, b, 13) and weaver._L.calls[1].snaps[0]["a"]["key_bits"] == 0
    for bad in ((CA_OFF,) + a[1:5] + (a[5][:4],), ([0, 3, 3, 4],) + a[1:], ([0, 5],) + a[1:]):
        with pytest.raises(ValueError):
            weaver.merge_maps(bad, b, 13)
    weaver._L.play = lambda call: None
    empty = ([0], [], [], [], [], [])
    res = weaver.merge_maps(empty, empty, 13)
    assert cap(res.src) == 1 and len(res.src) == 0
    assert [cap(getattr(res.maps, f)) for f in MAP_FIELDS] == [2, 1, 1, 1, 1, 1]
    assert [len(getattr(res.maps, f)) for f in MAP_FIELDS] == [1, 0, 0, 0, 0, 0]


def test_merge_maps_device(weaver):
    def play(call):
        mb, r = call.snaps
        call.seen = {s: rd(mb[s]["coll_offsets"], U64, D + 1) for s in "ab"}
        wr(r["merged_offsets"], np.array(CM_OFF, U64))
        call.structs[1].maps.n_segs = 3
    weaver._L.play = play
    mo, S = weaver.merge_maps_device(CA_OFF, (0x1000, 0x1100, 0x1200, 0x1300, 0x1400), CB_OFF,
                                     (0x2000, 0x2100, 0x2200, 0, None), 13, 21, 0x7000, MOUT, 99)
    call = one_call(weaver, "cw_merge_maps", abi.CW_MEM_DEVICE)
    assert call.types == [abi.CwMapMergeBatch, abi.CwMapMergeResult]
    mb, r = call.snaps
    assert mb["a"].pop("coll_offsets") and mb["b"].pop("coll_offsets")
    assert mb == {"a": {"n_colls": D, "id_key": 0x1000, "cause": 0x1100, "cause_is_id": 0x1200,
                        "kind": 0x1300, "key_bits": 21, "token_bits": 13}, "a_value": 0x1400,
                  "b": {"n_colls": D, "id_key": 0x2000, "cause": 0x2100, "cause_is_id": 0x2200,
                        "kind": None, "key_bits": 21, "token_bits": 13}, "b_value": None}
    same(call.seen["a"], np.array(CA_OFF, U64)), same(call.seen["b"], np.array(CB_OFF, U64))
    assert r["merged_src"] == 0x7000 and r["maps"] == dict(MOUT, cap_segs=99, n_segs=0)
    same(mo, np.array(CM_OFF, U64))
    assert S == 3 and type(S) is int
    with pytest.raises(ValueError):
        weaver.merge_maps_device(CA_OFF, (1, 2, 3, 4, 5), [0, 3], (1, 2, 3, 4, 5), 13, 21, 6, MOUT, 9)
    assert len(weaver._L.calls) == 1


CK_OFF = [0, 2, 2, 7]  # 7 kept of 5 inputs: [id] nodes


@pytest.mark.parametrize("site_bits", [1, 0])
def test_weft_maps_host(weaver, site_bits):
    cols = map_nodes(5)
    cut = np.arange(6, dtype=U64) + U64(50)  # D << 1; any length passes with site_bits 0
    room = 5 + (D << site_bits)  # 11 or 8

    def play(call):
        wb, r = call.snaps
        call.seen["in"] = read_map_batch(wb["nodes"])
        call.seen["cut"] = rd(wb["cut"], U64, 6)
        wr(r["kept_offsets"], np.array(CK_OFF, U64))
        wr(r["kept_src"], np.arange(7, dtype=U32) + U32(600))
        call.structs[1].maps.n_segs = 2
        fill_map(r["maps"], 2, 9, D)
    weaver._L.play = play
    res = weaver.weft_maps(C_OFF, *cols, 13, 17, site_bits, list(map(int, cut)), key_bits=21)
    call = one_call(weaver, "cw_weft_maps", abi.CW_MEM_HOST)
    assert call.types == [abi.CwMapWeftBatch, abi.CwMapWeftResult]
    wb, r = call.snaps
    s = wb["nodes"]
    assert (s["n_colls"], s["key_bits"], s["token_bits"]) == (D, 21, 13) and nulls(s) == set()
    assert (wb["site_shift"], wb["site_bits"]) == (17, site_bits) and wb["cut"]
    for got, want in zip(call.seen["in"], (np.array(C_OFF, U64),) + cols):
        same(got, want)
    same(call.seen["cut"], cut)
    assert r["kept_offsets"] and r["kept_src"]
    assert (r["maps"]["cap_segs"], r["maps"]["n_segs"]) == (room, 0) and nulls(r["maps"]) == set()
    assert isinstance(res, abi.MapWeftResult)
    same(res.offsets, np.array(CK_OFF, U64))
    same(res.src, np.arange(7, dtype=U32) + U32(600))
    assert cap(res.src) == room
    check_map(res.maps, 2, 9, D, (room, 2 * room, D))


def test_weft_maps_host_floors_and_errors(weaver):
    weaver._L.play = lambda call: None
    res = weaver.weft_maps([0], [], [], [], [], 13, 17, 1, [])
    assert weaver._L.calls[0].snaps[0]["nodes"]["key_bits"] == 0
    assert cap(res.src) == 1 and len(res.src) == 0
    assert [cap(getattr(res.maps, f)) for f in MAP_FIELDS] == [2, 1, 1, 1, 1, 1]
    assert [len(getattr(res.maps, f)) for f in MAP_FIELDS] == [1, 0, 0, 0, 0, 0]
    i, c, ci, k = map_nodes(5)
    cut = np.zeros(6, U64)
    for bad in ((i[:4], c, ci, k), (i, c[:4], ci, k), (i, c, ci[:4], k), (i, c, ci, k[:4])):
        with pytest.raises(ValueError):
            weaver.weft_maps(C_OFF, *bad, 13, 17, 1, cut)
    with pytest.raises(ValueError):
        weaver.weft_maps([0, 3, 3, 4], i, c, ci, k, 13, 17, 1, cut)
    with pytest.raises(ValueError):
        weaver.weft_maps(C_OFF, i, c, ci, k, 13, 17, 1, cut[:5])
    with pytest.raises(ValueError):
        weaver.weft_maps(C_OFF, i, c, ci, k, 13, 17, 10, cut)
    assert len(weaver._L.calls) == 1
    weaver.weft_maps(C_OFF, i, c, ci, k, 13, 17, 11, cut)  # out of 1..10: the library's error
    assert weaver._L.calls[1].snaps[1]["maps"]["cap_segs"] == 5 + (D << 11)


def test_weft_maps_device(weaver):
    def play(call):
        call.seen["off"] = rd(call.snaps[0]["nodes"]["coll_offsets"], U64, D + 1)
        wr(call.snaps[1]["kept_offsets"], np.array(CK_OFF, U64))
        call.structs[1].maps.n_segs = 2
    weaver._L.play = play
    ko, S = weaver.weft_maps_device(C_OFF, (0x1000, 0x1100, 0, 0x1300), 13, 21, 17, 3, 0x5000,
                                    0x7000, MOUT, 99)
    call = one_call(weaver, "cw_weft_maps", abi.CW_MEM_DEVICE)
    assert call.types == [abi.CwMapWeftBatch, abi.CwMapWeftResult]
    wb, r = call.snaps
    assert wb["nodes"].pop("coll_offsets")
    assert wb == {"nodes": {"n_colls": D, "id_key": 0x1000, "cause": 0x1100, "cause_is_id": None,
                            "kind": 0x1300, "key_bits": 21, "token_bits": 13},
                  "site_shift": 17, "site_bits": 3, "cut": 0x5000}
    same(call.seen["off"], np.array(C_OFF, U64))
    assert r["kept_src"] == 0x7000 and r["maps"] == dict(MOUT, cap_segs=99, n_segs=0)
    same(ko, np.array(CK_OFF, U64))
    assert S == 2 and type(S) is int


# ----------------------------------------------------------------------- render
R_OFF = [0, 5, 5, 9]


@pytest.mark.parametrize("perm_dt", [U32, U16, np.int64])
@pytest.mark.parametrize("val_dt", [None, U8, np.float32, np.int64])
def test_render_lists_host(weaver, perm_dt, val_dt):
    perm = (np.arange(N) % 20).astype(perm_dt)
    bits = np.array([0xF0F0F0F0, 0xFFFF], U32)  # a word more than needed is legal
    val = None if val_dt is None else (np.arange(N) + 65).astype(val_dt)
    vsize = 0 if val is None else val.dtype.itemsize
    udt = None if val is None else {1: U8, 4: U32, 8: U64}[vsize]
    pdt = U16 if perm_dt == U16 else U32

    def play(call):
        b, r = call.snaps
        call.seen = {"off": rd(b["doc_offsets"], U64, D + 1), "perm": rd(b["weave_perm"], pdt, N),
                     "bits": rd(b["visible_bits"], U32, 1)}
        if vsize:
            call.seen["val"] = rd(b["value"], udt, N)
            wr(r["rendered_value"], (np.arange(9) + 33).astype(udt))
        wr(r["rendered_offsets"], np.array(R_OFF, U64))
        wr(r["rendered_src"], np.arange(9, dtype=U32) + U32(600))
    weaver._L.play = play
    res = weaver.render_lists(OFF, perm, bits, val)
    call = one_call(weaver, "cw_render_lists", abi.CW_MEM_HOST)
    assert call.types == [abi.CwRenderBatch, abi.CwRenderResult]
    b, r = call.snaps
    assert (b["n_docs"], b["perm16"], b["value_size"]) == (D, int(perm_dt == U16), vsize)
    assert nulls(b) == (set() if vsize else {"value"})
    assert nulls(r) == (set() if vsize else {"rendered_value"})
    same(call.seen["off"], np.array(OFF, U64)), same(call.seen["perm"], perm.astype(pdt))
    same(call.seen["bits"], bits[:1])
    assert isinstance(res, abi.RenderResult)
    same(res.offsets, np.array(R_OFF, U64))
    same(res.src, np.arange(9, dtype=U32) + U32(600))
    assert cap(res.src) == N
    if vsize:
        same(call.seen["val"], val.view(udt))
        same(res.value, (np.arange(9) + 33).astype(udt))
        assert cap(res.value) == N
    else:
        assert res.value is None


def test_render_lists_host_floors_and_errors(weaver):
    weaver._L.play = lambda call: None
    res = weaver.render_lists([0], [], [], np.zeros(0, U16))
    assert (cap(res.src), cap(res.value), len(res.src), len(res.value)) == (1, 1, 0, 0)
    assert res.value.dtype == U16 and weaver._L.calls[0].snaps[0]["value_size"] == 2
    perm, bits = np.zeros(33, U32), np.zeros(2, U32)
    off = [0, 33]
    with pytest.raises(ValueError):
        weaver.render_lists([0, 32], perm, bits)
    with pytest.raises(ValueError):
        weaver.render_lists(off, perm, bits[:1])
    with pytest.raises(ValueError):
        weaver.render_lists(off, perm, bits, np.zeros(32, U8))
    with pytest.raises(ValueError):
        weaver.render_lists(off, perm, bits, np.zeros(33, np.complex128))
    assert len(weaver._L.calls) == 1


@pytest.mark.parametrize("perm16", [False, True])
def test_render_lists_device(weaver, perm16):
    def play(call):
        call.seen["off"] = rd(call.snaps[0]["doc_offsets"], U64, D + 1)
        wr(call.snaps[1]["rendered_offsets"], np.array(R_OFF, U64))
    weaver._L.play = play
    ro = weaver.render_lists_device(OFF, 0x1000, 0x2000, 0x3000, 0x4000, 4, 0x5000, perm16)
    call = one_call(weaver, "cw_render_lists", abi.CW_MEM_DEVICE)
    assert call.types == [abi.CwRenderBatch, abi.CwRenderResult]
    b, r = call.snaps
    assert b.pop("doc_offsets") and r.pop("rendered_offsets")
    assert b == {"n_docs": D, "weave_perm": 0x1000, "visible_bits": 0x2000, "perm16": int(perm16),
                 "value_size": 4, "value": 0x4000}
    assert r == {"rendered_src": 0x3000, "rendered_value": 0x5000}
    same(call.seen["off"], np.array(OFF, U64)), same(ro, np.array(R_OFF, U64))
    weaver.render_lists_device(OFF, 0x1000, 0x2000)  # the count-only call
    b, r = weaver._L.calls[1].snaps
    assert (b["perm16"], b["value_size"], b["value"]) == (0, 0, None)
    assert (r["rendered_src"], r["rendered_value"]) == (None, None)


E_OFF = [0, 2, 2, 3]


@pytest.mark.parametrize("val_dt", [None, U16, np.float64])
def test_render_maps_host(weaver, val_dt):
    sc, sk = np.array([0, 0, 2, 2], U32), np.arange(4, dtype=U64) + U64(70)
    sa = np.array([1, -1, 0, 1], I64)
    val = None if val_dt is None else (np.arange(5) + 65).astype(val_dt)
    vsize = 0 if val is None else val.dtype.itemsize
    udt = None if val is None else {2: U16, 8: U64}[vsize]

    def play(call):
        b, r = call.snaps
        call.seen = {"coll": rd(b["seg_coll"], U32, 4), "key": rd(b["seg_key"], U64, 4),
                     "active": rd(b["seg_active"], I64, 4)}
        if vsize:
            call.seen["off"] = rd(b["coll_offsets"], U64, D + 1)
            call.seen["val"] = rd(b["value"], udt, 5)
            wr(r["entry_value"], (np.arange(3) + 33).astype(udt))
        wr(r["entry_offsets"], np.array(E_OFF, U64))
        wr(r["entry_key"], np.arange(3, dtype=U64) + U64(800))
        wr(r["entry_src"], np.arange(3, dtype=U32) + U32(600))
    weaver._L.play = play
    res = weaver.render_maps(D, list(map(int, sc)), sk, sa, C_OFF, val)
    call = one_call(weaver, "cw_render_maps", abi.CW_MEM_HOST)
    assert call.types == [abi.CwMapRenderBatch, abi.CwMapRenderResult]
    b, r = call.snaps
    assert (b["n_colls"], b["n_segs"], b["value_size"]) == (D, 4, vsize)
    assert nulls(b) == (set() if vsize else {"coll_offsets", "value"})
    assert nulls(r) == (set() if vsize else {"entry_value"})
    same(call.seen["coll"], sc), same(call.seen["key"], sk), same(call.seen["active"], sa)
    assert isinstance(res, abi.MapRenderResult)
    same(res.offsets, np.array(E_OFF, U64))
    same(res.key, np.arange(3, dtype=U64) + U64(800))
    same(res.src, np.arange(3, dtype=U32) + U32(600))
    assert (cap(res.key), cap(res.src)) == (4, 4)
    if vsize:
        same(call.seen["off"], np.array(C_OFF, U64)), same(call.seen["val"], val.view(udt))
        same(res.value, (np.arange(3) + 33).astype(udt))
        assert cap(res.value) == 4
    else:
        assert res.value is None


def test_render_maps_host_floors_and_errors(weaver):
    weaver._L.play = lambda call: None
    res = weaver.render_maps(2, [], [], [], [0, 0, 0], np.zeros(0, U32))
    assert [cap(x) for x in (res.key, res.src, res.value)] == [1, 1, 1]
    assert [len(x) for x in (res.offsets, res.key, res.src, res.value)] == [3, 0, 0, 0]
    assert weaver._L.calls[0].snaps[0]["n_segs"] == 0
    sc, sk, sa = np.zeros(4, U32), np.zeros(4, U64), np.zeros(4, I64)
    val = np.zeros(5, U8)
    for bad in ((sc, sk[:3], sa), (sc, sk, sa[:3])):
        with pytest.raises(ValueError):
            weaver.render_maps(D, *bad)
    with pytest.raises(ValueError):
        weaver.render_maps(D, sc, sk, sa, [0, 3, 5], val)
    with pytest.raises(ValueError):
        weaver.render_maps(D, sc, sk, sa, [0, 3, 3, 4], val)
    with pytest.raises(ValueError):
        weaver.render_maps(D, sc, sk, sa, C_OFF, np.zeros(5, np.complex128))
    assert len(weaver._L.calls) == 1


def test_render_maps_device(weaver):
    def play(call):
        b, r = call.snaps
        if b["coll_offsets"]:
            call.seen["off"] = rd(b["coll_offsets"], U64, D + 1)
        wr(r["entry_offsets"], np.array(E_OFF, U64))
    weaver._L.play = play
    eo = weaver.render_maps_device(D, 4, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, C_OFF, 0x6000, 2,
                                   0x7000)
    call = one_call(weaver, "cw_render_maps", abi.CW_MEM_DEVICE)
    assert call.types == [abi.CwMapRenderBatch, abi.CwMapRenderResult]
    b, r = call.snaps
    assert b.pop("coll_offsets") and r.pop("entry_offsets")
    assert b == {"n_colls": D, "n_segs": 4, "seg_coll": 0x1000, "seg_key": 0x2000,
                 "seg_active": 0x3000, "value_size": 2, "value": 0x6000}
    assert r == {"entry_key": 0x4000, "entry_src": 0x5000, "entry_value": 0x7000}
    same(call.seen["off"], np.array(C_OFF, U64)), same(eo, np.array(E_OFF, U64))
    eo = weaver.render_maps_device(D, 4, 0x1000, 0x2000, 0x3000)  # the count-only call
    b, r = weaver._L.calls[1].snaps
    assert (b["coll_offsets"], b["value_size"], b["value"]) == (None, 0, None)
    assert (r["entry_key"], r["entry_src"], r["entry_value"]) == (None, None, None)
    same(eo, np.array(E_OFF, U64))


# ------------------------------------------------- context calls and primitives
def test_context_calls(weaver):
    weaver.set_stream(0x77)
    weaver.set_async(True)
    weaver.set_profiling(False)
    weaver.set_profile_only("list_union")
    weaver.set_profile_only(None)
    weaver.set_option("list_merge_fused", 0)
    weaver.reset_kernel_stats()
    calls = weaver._L.calls
    assert [c.name for c in calls] == [
        "cw_ctx_set_stream", "cw_ctx_set_async", "cw_ctx_set_profiling", "cw_ctx_set_profile_only",
        "cw_ctx_set_profile_only", "cw_ctx_set_option", "cw_reset_kernel_stats"]
    assert all(c.h is H for c in calls)
    assert calls[0].plain[0].value == 0x77
    assert [c.plain for c in calls[1:]] == [[1], [0], [b"list_union"], [None],
                                            [b"list_merge_fused", 0], []]


def test_counter_and_kernel_stats(weaver):
    def play(call):
        if call.name == "cw_get_counter":
            call.structs[0].value = 41
        elif call.plain[0] is not None:  # the second call: an array of two stats
            arr = call.plain[0]
            arr[0].name, arr[0].launches, arr[0].total_ms, arr[0].bytes_alg = b"k_a", 3, 1.5, 64.0
            arr[1].name, arr[1].launches, arr[1].total_ms, arr[1].bytes_alg = b"k_b", 1, 0.25, 8.0
        return 0 if call.name == "cw_get_counter" else 2
    weaver._L.play = play
    assert weaver.counter("continued_sublists") == 41
    assert weaver._L.calls[0].plain == [b"continued_sublists"]
    assert weaver.kernel_stats() == {"k_a": (3, 1.5, 64.0), "k_b": (1, 0.25, 8.0)}
    first, second = weaver._L.calls[1:]
    assert first.plain == [None, 0] and second.plain[1] == 2 and len(second.plain[0]) == 2


def test_primitives_pass_their_arguments_through(weaver):
    weaver.sort_keys_device(1, 2, 3, 4, 5)
    weaver.sort_keys32_device(1, 2, 3, 4, 5)
    weaver.lookup_keys_device(1, 2, 3, 4, 5, 6)
    weaver.lookup_keys_device(1, 2, 3, 4, 5, 6, 7)
    weaver.partition_keys_dev(1, 2, 3, 4, 5, 6)
    weaver.gather_device(1, 2, 3, 4, 5)
    weaver.scatter32_device(1, 2, 3, 4)
    weaver.dist("rs_top", 1, 2, 3, 4, 5)
    got = [(c.name, c.plain) for c in weaver._L.calls]
    assert got == [("cw_sort_keys", [1, 2, 3, 4, 5]), ("cw_sort_keys32", [1, 2, 3, 4, 5]),
                   ("cw_lookup_keys", [1, 2, 3, 4, 5, 6, None]),
                   ("cw_lookup_keys", [1, 2, 3, 4, 5, 6, 7]),
                   ("cw_partition_keys_dev", [1, 2, 3, 4, 5, 6]), ("cw_gather", [1, 2, 3, 4, 5]),
                   ("cw_scatter32", [1, 2, 3, 4]), ("cw_dist_rs_top", [1, 2, 3, 4, 5])]
    assert all(c.h is H for c in weaver._L.calls)


def test_partition_keys_device_returns_the_counts(weaver):
    weaver._L.play = lambda call: wr(call.plain[5], np.array([4, 0, 9, 1], U64))
    counts = weaver.partition_keys_device(0x1000, 14, 0x2000, 3, 0x3000)
    call = one_call(weaver, "cw_partition_keys", ...)
    assert call.plain[:5] == [0x1000, 14, 0x2000, 3, 0x3000]
    same(counts, np.array([4, 0, 9, 1], U64))


def test_a_nonzero_return_raises_with_the_library_text(weaver):
    weaver._L.play = lambda call: b"cut is required" if call.name == "cw_last_error" else -1
    with pytest.raises(abi.WeaveError, match="cw_weave_maps: cut is required"):
        weaver.weave_maps_device(C_OFF, (1, 2, 3, 4), 13, 21, MOUT, 9)
    assert [c.name for c in weaver._L.calls] == ["cw_weave_maps", "cw_last_error"]
