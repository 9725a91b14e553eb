"""cw_weft_lists_dev / k_list_weft vs the CPU model of weft, array for array (-m gpu).

The device call gets torch tensors: the node columns, the cut table, kept_src
and every weave array, the result tensors at exactly the header's capacity
(N + (n_docs << site_bits)) plus guard words that must come back untouched.
Inputs and expected arrays are those of tests/weft_model.py; every comparison
is equality, for every document and every array.

Covered: the 64-bit words of the keep bitmap and the 1,024-thread rows, site_bits
1 / 4 / 10, the exact capacity, the two routes (fused kernel, general select) in
device and in host memory, the 65,535 / 65,536 boundary between them, the
look-back over 64 .. 200 documents, the layout cache against changing cut
tables, NULL outputs, empty shapes and the error returns.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from cause_amd import abi, pack
from tests import test_gpu_weft as T
from tests import weft_model as M

pytestmark = pytest.mark.gpu

GENERAL = {"weft_count", "weft_write"}
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
OUTPUTS = ("src", "weave_perm", "visible_bits", "visible_count", "max_ts", "status", "yarn_perm")


@pytest.fixture(scope="module")
def weaver():
    with abi.Weaver(0) as w:
        yield w


def _up(x):
    import torch

    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(SIGNED[x.dtype])).to(torch.device("cuda", 0))


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def dev_weft(weaver, off, idk, ck, kd, layout, cut, yarns=True, bits=True, max_ts=True,
             site_bits=None, null_cut=False, drop=None, stream=None, wrapper=False):
    """cw_weft_lists_dev on device copies of the inputs, the result tensors of
    exactly the header's capacity (+ the guard), filled beforehand.  -> (return
    code, T.Out holding what came back)."""
    import torch

    off = np.ascontiguousarray(off, np.uint64)
    gi, gc, gk = _up(np.asarray(idk, np.uint64)), _up(np.asarray(ck, np.uint64)), _up(np.asarray(kd, np.uint8))
    # (an empty table still gets an allocation: a null cut is an error of its own)
    gcut = _up(np.asarray(cut, np.uint64) if len(cut) else np.zeros(1, np.uint64))
    D, N = len(off) - 1, len(idk)
    o = T.Out(D, N + (D << layout.site_bits), yarns, bits, max_ts)
    g = {f: _up(getattr(o, f)) for f in OUTPUTS if getattr(o, f) is not None}
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    ptr = lambda f: None if f == drop or f not in g else _dp(g[f])
    if wrapper:
        ko = weaver.weft_lists_device(
            off, [t.data_ptr() if t.numel() else 0 for t in (gi, gc, gk)], layout, gcut.data_ptr(),
            g["src"].data_ptr(), {f: g[f].data_ptr() for f in g if f != "src"})
        o.kept_offsets[:D + 1] = ko
        rc = 0
    else:
        b, off = abi.Weaver._batch(off, _dp(gi), _dp(gc), _dp(gk), layout)
        if site_bits is not None:
            b.site_bits = site_bits
        wb = abi.CwWeftBatch(b, None if null_cut else C.cast(C.c_void_p(gcut.data_ptr()),
                                                             C.POINTER(C.c_uint64)))
        r = abi.CwWeftResult(o.kept_offsets.ctypes.data_as(C.POINTER(C.c_uint64)), ptr("src"),
                             abi.CwListResult(ptr("weave_perm"), ptr("visible_bits"),
                                              ptr("visible_count"), ptr("max_ts"), ptr("status"),
                                              ptr("yarn_perm")))
        rc = weaver._L.cw_weft_lists_dev(weaver._h, C.byref(wb), C.byref(r))
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    for f, t in g.items():
        a = getattr(o, f)
        a[:] = t.cpu().numpy().view(a.dtype)
    return rc, o


def compare(o, exp, yarns=True, bits=True, max_ts=True):
    """A call's arrays == the model's, for every document and every array, and
    nothing written past the kept nodes."""
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


def check_dev(weaver, args, exp, **kw):
    rc, o = dev_weft(weaver, *args, **kw)
    assert rc == 0, T.last_error(weaver)
    flags = {k: kw[k] for k in ("yarns", "bits", "max_ts") if k in kw}
    return compare(o, exp, **flags)


def check_case(weaver, name, **kw):
    return check_dev(weaver, M.CASES[name](), M.expected(name), **kw)


def ran(weaver, call):
    """Kernel stat names of one call."""
    weaver.set_profiling(True)
    weaver.reset_kernel_stats()
    try:
        call()
        return set(weaver.kernel_stats())
    finally:
        weaver.set_profiling(False)
        weaver.reset_kernel_stats()


# ------------------------------------------------- 1. device call == model ----
MODEL_CASES = ["small", "tiles", "bits1", "bits10", "all_ranks_absent", "upper_words", "empty_named"]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_device_call_equals_the_model(weaver, name):
    exp = M.expected(name)
    if name == "all_ranks_absent":  # the kept size is the capacity itself
        off, idk, _, _, lay, _ = M.case_all_ranks_absent()
        assert int(exp.offsets[-1]) == len(idk) + (1 << lay.site_bits)
    if name == "empty_named":  # a document that is only an [id] node
        assert list(np.diff(exp.offsets.astype(np.int64))) == [1, 1, 0] and exp.src[1] == M.NO_SRC
    check_case(weaver, name)


@pytest.mark.parametrize("name", MODEL_CASES)
def test_async_device_call_equals_the_model(name):
    import torch

    s = torch.cuda.Stream()
    with abi.Weaver(0) as w:
        w.set_stream(s.cuda_stream)
        w.set_async(True)
        check_case(w, name, stream=s)
        check_case(w, name, stream=s)


def test_wrapper_returns_the_kept_offsets(weaver):
    rc, o = dev_weft(weaver, *M.case_small(), wrapper=True)
    compare(o, M.expected("small"))


# ------------------------------------------------------------------ 2. routes ----
def test_routes_in_device_and_host_memory():
    exp = M.expected("tiles")
    with abi.Weaver(0) as wf, abi.Weaver(0, options={"list_weft_fused": 0}) as wg:
        outs = {}
        for mem, call in (("device", check_case), ("host", T.check_case)):
            res = {}
            names = ran(wf, lambda: res.update(o=call(wf, "tiles")))
            assert "list_weft" in names and not names & GENERAL, (mem, sorted(names))
            outs[mem, "fused"] = res["o"]
            names = ran(wg, lambda: res.update(o=call(wg, "tiles")))
            assert GENERAL <= names and "list_weft" not in names, (mem, sorted(names))
            outs[mem, "general"] = res["o"]
        first = outs["device", "fused"]
        for key, o in outs.items():
            compare(o, exp)
            T.assert_same_arrays(first, o)
    with pytest.raises(abi.WeaveError, match="unknown option"):
        abi.Weaver(0, options={"list_weft_fusedx": 0})


# ----------------------------------------------------------- 3. size boundary ----
@functools.lru_cache(maxsize=None)
def boundary(n):
    """One document of n nodes, 3 sites, a consistent cut; -> (args, expected)."""
    args = M._case(3, (n,), ("closed",), 300 + n % 7)
    return args, M.weft_expected(*args)


@pytest.mark.parametrize("n,fused", [(65535, True), (65536, False)])
def test_the_largest_fused_document(weaver, n, fused):
    args, exp = boundary(n)
    names = ran(weaver, lambda: check_dev(weaver, args, exp))
    if fused:
        assert "list_weft" in names and not names & GENERAL, sorted(names)
    else:
        assert GENERAL <= names and "list_weft" not in names, sorted(names)


@pytest.mark.parametrize("name", ["giant_whole", "giant_batch"])
def test_larger_documents_take_the_general_route(weaver, name):
    names = ran(weaver, lambda: check_case(weaver, name))
    assert GENERAL <= names and "list_weft" not in names, sorted(names)


# ---------------------------------------------------------------- 4. look-back ----
LB_MODES = ("random", "closed", "whole", "nodes")


@functools.lru_cache(maxsize=None)
def many_documents(D, every_tenth_empty=False):
    rng = np.random.default_rng(400 + D)
    sizes = [int(x) for x in rng.integers(2, 6, D)]
    modes = [LB_MODES[int(x)] for x in rng.integers(0, len(LB_MODES), D)]
    if every_tenth_empty:
        for d in range(0, D, 10):
            sizes[d], modes[d] = 0, "none"
    args = M._case(8, sizes, modes, 401 + D)
    return args, M.weft_expected(*args)


@pytest.mark.parametrize("D", [64, 65, 66, 128, 129, 130, 200])
def test_look_back_windows(weaver, D):
    args, exp = many_documents(D)
    assert len(exp.offsets) == D + 1 and np.all(np.diff(exp.offsets.astype(np.int64)) > 0)
    names = ran(weaver, lambda: check_dev(weaver, args, exp))
    assert "list_weft" in names


def test_documents_that_keep_nothing(weaver):
    args, exp = many_documents(200, True)
    kept = np.diff(exp.offsets.astype(np.int64))
    assert np.all(kept[::10] == 0) and np.all(np.delete(kept, np.s_[::10]) > 0)
    assert np.all(exp.status[::10] == abi.STATUS_ROOT)
    check_dev(weaver, args, exp)


# --------------------------------------------------------- 5. caches, epochs ----
@functools.lru_cache(maxsize=None)
def tiles_with_other_cuts(k):
    off, idk, ck, kd, lay, _ = M.case_tiles()
    rng = np.random.default_rng(500 + k)
    pattern = ("random", "closed", "whole", "nodes", "absent", "none")
    modes = [pattern[(d + k) % len(pattern)] for d in range(len(off) - 1)]
    args = (off, idk, ck, kd, lay, M.make_cuts(off, idk, lay, rng, modes))
    return args, M.weft_expected(*args)


def test_one_layout_three_cut_tables_then_other_layouts():
    tables = [tiles_with_other_cuts(k) for k in range(3)]
    assert not np.array_equal(tables[0][0][5], tables[1][0][5])
    assert not np.array_equal(tables[1][0][5], tables[2][0][5])
    with abi.Weaver(0) as w:
        for args, exp in tables:  # the layout repeats, the cut table does not
            check_dev(w, args, exp)
        check_case(w, "small")  # another document count
        first = check_dev(w, *tables[0])
        for v in (0, 1, 0, 1):  # the two routes in turn
            w.set_option("list_weft_fused", v)
            T.assert_same_arrays(first, check_dev(w, *tables[0]))
            check_case(w, "small")


def test_alternating_with_weave_and_the_host_call():
    import torch

    off, idk, ck, kd, lay, cut = M.case_tiles()
    perm, vis, st = oracle.batch_lists(off, idk, ck, kd, method=oracle.METHOD_LITERAL)
    D, N = len(off) - 1, len(idk)
    gi, gc, gk = _up(idk), _up(ck), _up(kd)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=gi.device)

    def weave(w):
        o = {"weave_perm": z(N, torch.int32), "visible_bits": z((N + 31) // 32, torch.int32),
             "visible_count": z(D, torch.int32), "max_ts": z(D, torch.int64),
             "status": z(D, torch.int32), "yarn_perm": z(N, torch.int32)}
        torch.cuda.synchronize()
        w.weave_lists_device(off, gi.data_ptr(), gc.data_ptr(), gk.data_ptr(), lay,
                             {k: v.data_ptr() for k, v in o.items()})
        torch.cuda.synchronize()
        assert np.array_equal(o["status"].cpu().numpy().view(np.uint32)[:D], st)
        assert np.array_equal(o["weave_perm"].cpu().numpy().view(np.uint32)[:N], perm)
        b = np.unpackbits(o["visible_bits"].cpu().numpy().view(np.uint8), bitorder="little")[:N]
        assert np.array_equal(b, vis)

    with abi.Weaver(0) as w:
        first = check_case(w, "tiles")
        weave(w)
        T.assert_same_arrays(first, check_case(w, "tiles"))
        T.assert_same_arrays(first, T.check_case(w, "tiles"))  # the host call, same layout
        T.check_case(w, "small")
        T.assert_same_arrays(first, check_case(w, "tiles"))
        weave(w)
        check_case(w, "small")


# ----------------------------------------- 6. optional outputs and empties ----
@pytest.mark.parametrize("null", [("bits",), ("max_ts",), ("yarns",), ("bits", "max_ts", "yarns")],
                         ids=lambda t: "+".join(t))
def test_optional_outputs_null(weaver, null):
    full = check_case(weaver, "tiles")
    o = check_case(weaver, "tiles", **{k: False for k in null})
    gone = {"bits": "visible_bits", "max_ts": "max_ts", "yarns": "yarn_perm"}
    T.assert_same_arrays(full, o, skip=[gone[k] for k in null])


def test_no_documents(weaver):
    lay = pack.KeyLayout(8, 4, 0)
    z64 = np.zeros(0, np.uint64)
    rc, o = dev_weft(weaver, np.zeros(1, np.uint64), z64, z64, np.zeros(0, np.uint8), lay, z64)
    assert rc == 0, T.last_error(weaver)
    assert o.kept_offsets[0] == 0 and o.untouched("kept_offsets", 1)
    for f in OUTPUTS:
        assert o.untouched(f, 0), f


def test_every_document_empty(weaver):
    lay = pack.KeyLayout(8, 4, 0)
    D = 5
    z64 = np.zeros(0, np.uint64)
    args = (np.zeros(D + 1, np.uint64), z64, z64, np.zeros(0, np.uint8), lay,
            np.zeros(D << lay.site_bits, np.uint64))
    exp = M.weft_expected(*args)
    assert list(exp.status) == [abi.STATUS_ROOT] * D
    o = check_dev(weaver, args, exp)
    assert list(o.status[:D]) == [abi.STATUS_ROOT] * D and not o.kept_offsets[:D + 1].any()


# ------------------------------------------------------------------ 7. errors ----
def _bad_calls():
    off, idk, ck, kd, lay, cut = M.case_small()
    shifted = off.copy()
    shifted[0] = 1
    falling = off.copy()
    falling[2] = falling[3] + np.uint64(5)  # offsets[2] > offsets[3]
    assert falling[2] <= len(idk)
    return {
        "site_bits 0": dict(site_bits=0),
        "site_bits 11": dict(site_bits=11),
        "null cut": dict(null_cut=True),
        "offsets[0] != 0": dict(off=shifted),
        "offsets decrease": dict(off=falling),
        "null weave_perm": dict(drop="weave_perm"),
        "null kept_src": dict(drop="src"),
    }


@pytest.mark.parametrize("bad", sorted(_bad_calls()))
def test_error_returns_and_the_context_lives_on(weaver, bad):
    """Every pointer handed over is device memory (or NULL): only the batch's
    numbers are wrong."""
    off, idk, ck, kd, lay, cut = M.case_small()
    kw = dict(_bad_calls()[bad])
    rc, o = dev_weft(weaver, kw.pop("off", off), idk, ck, kd, lay, cut, **kw)
    assert rc < 0 and T.last_error(weaver), (bad, rc)
    for f in OUTPUTS:
        assert o.untouched(f, 0), f"{f} written by a refused call"
    check_case(weaver, "small")
