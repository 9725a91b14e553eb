"""Calls that share staging buffers and cache objects on one context.

The host code keeps one set of staging buffers for map results (hm_*), one for
list results (hs_*), one cached device layout per list call and one cached pack
table per map call.  Nothing here is about a kernel: every case runs the eight
calls next to each other on ONE Weaver -- in host memory, through the _device
forms, in reverse order, with layouts that grow and shrink, after a rejected
call -- and compares every array with the same call on a fresh Weaver, with the
models of tests/ (mapweft_model, weft_model, render_model, the host unions of
the merge tests) and with the oracle's folds.
"""
import dataclasses
import pathlib
import re

import numpy as np
import pytest

import oracle
from cause_amd import abi
from tests import mapweft_model as MM
from tests import render_model as RM
from tests import test_gpu_list_merge as LM
from tests import test_gpu_map_merge as UM
from tests import weft_model as W
from tests.test_gpu_maps import gpu_maps, oracle_maps

pytestmark = pytest.mark.gpu

CSRC = pathlib.Path(__file__).resolve().parents[1] / "cause_amd" / "csrc"


def constant(file, name):
    """A constexpr uint32_t of the sources, e.g. MPK = 2048 or LW_MAXDOC = 0xFFFFu."""
    m = re.search(rf"constexpr\s+uint32_t\s+{name}\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\s*;", (CSRC / file).read_text())
    assert m, f"{name} not found in {file}"
    return int(m.group(1), 0)


MPK = constant("mappack.hip", "MPK")
MU_MAXCOLL = constant("mapmerge.hip", "MU_MAXCOLL")
MW_MAXCOLL = constant("mapweft.hip", "MW_MAXCOLL")
LW_MAXDOC = constant("listweft.hip", "LW_MAXDOC")
LU_MAXDOC = constant("listmerge.hip", "LU_MAXDOC")

ORDER = ("weave_maps", "merge_maps", "weft_maps", "weave_lists", "merge_lists", "weft_lists",
         "render_maps", "render_lists")
# the kernel stat of each map call's fused route, and of its general route
ROUTE = {"weave_maps": ("m_pack", "m_key"), "merge_maps": ("map_union", "mm_concat"),
         "weft_maps": ("map_weft", "mw_count")}


# ------------------------------------------------------------------ inputs ----
@dataclasses.dataclass
class Inputs:
    """One map batch and one list batch with everything the eight calls take."""
    m: tuple        # maps: off, id, cause, cis, kind, site_shift, site_bits, cut, token_bits
    ma: tuple       # ... split in two replicas (cw_merge_maps' sides)
    mb: tuple
    seg: tuple      # a map weave of m to render: n_colls, seg_coll, seg_key, seg_active
    mval: np.ndarray
    l: tuple        # lists: off, id, cause, kind, layout, cut
    la: tuple       # ... split in two replicas (cw_merge_lists' sides)
    lb: tuple
    woven: tuple    # a list weave of l to render: weave_perm, visible_bits
    lval: np.ndarray


def make_inputs(map_sizes, list_sizes, seed, split_seed=None):
    """seed: the ids, causes and cuts; split_seed (default: seed): which nodes go to
    which replica, so the two merge layouts too."""
    modes = lambda n: [MM.MODES[(seed + d) % len(MM.MODES)] for d in range(n)]
    m = MM._case(8, map_sizes, modes(len(map_sizes)), seed)
    rng = np.random.default_rng(seed if split_seed is None else split_seed)
    ma, mb, _, _ = UM.split(m[0], m[1:5], 0.3, rng)
    l = W._case(8, list_sizes, [("random", "closed", "nodes", "whole")[d % 4] for d in range(len(list_sizes))],
                seed + 1)
    na = [int(n) // 2 for n in np.diff(l[0].astype(np.int64))]
    la, lb = LM.split_at(*l[:4], rng, na)
    # what the render calls read comes from the models, not from a weave on the GPU
    D = len(m[0]) - 1
    folds = oracle_maps(*m[:5])
    seg = [(d, k, act) for d in range(D) for k, (act, _) in sorted(folds[d].items())]
    col = lambda j, dt: np.array([s[j] for s in seg], dt)
    perm, vis, _ = oracle.batch_lists(*l[:4], method=oracle.METHOD_LITERAL)
    return Inputs(m, ma, mb, (D, col(0, np.uint32), col(1, np.uint64), col(2, np.int64)),
                  rng.integers(1, 1 << 32, int(m[0][-1])).astype(np.uint32),
                  l, la, lb, (perm.astype(np.uint32), RM.pack_bits(vis)),
                  rng.integers(1, 1 << 62, int(l[0][-1])).astype(np.uint64))


def sizes_of(x):
    return np.diff(np.asarray(x[0]).astype(np.int64))


@pytest.fixture(scope="module")
def big():
    """Maps of 0, 1, 37 and MPK + 1 nodes: the last one sends all three map calls
    down their general routes.  Lists of 0, 1 and 300 nodes."""
    i = make_inputs((0, 1, 37, MPK + 1), (0, 1, 300), 11)
    assert sizes_of(i.m).max() > MPK and (sizes_of(i.ma) + sizes_of(i.mb)).max() > MPK
    assert sizes_of(i.l).max() <= LW_MAXDOC and (sizes_of(i.la) + sizes_of(i.lb)).max() <= LU_MAXDOC
    return i


@pytest.fixture(scope="module")
def small():
    """The first three collections only: every map call stays on its fused route."""
    i = make_inputs((0, 1, 37), (0, 1, 300), 12)
    assert (sizes_of(i.ma) + sizes_of(i.mb)).max() <= MPK and len(i.m[0]) - 1 <= min(MU_MAXCOLL, MW_MAXCOLL)
    return i


# ------------------------------------------------------------------ the calls ----
def flat(x, pre=""):
    """Every array of a result, by name."""
    out = {}
    for f in dataclasses.fields(x):
        v = getattr(x, f.name)
        if dataclasses.is_dataclass(v):
            out.update(flat(v, pre + f.name + "."))
        elif v is not None:
            out[pre + f.name] = np.asarray(v)
    return out


def same(x, y, what):
    fx, fy = flat(x), flat(y)
    assert fx.keys() == fy.keys(), what
    for k in fx:
        np.testing.assert_array_equal(fx[k], fy[k], err_msg=f"{what}: {k}")


def host_call(w, name, i):
    m, l = i.m, i.l
    if name == "weave_maps":
        return w.weave_maps(*m[:5], m[8])
    if name == "merge_maps":
        return w.merge_maps(i.ma, i.mb, m[8])
    if name == "weft_maps":
        return w.weft_maps(*m[:5], m[8], m[5], m[6], m[7])
    if name == "weave_lists":
        return w.weave_lists(*l[:5])
    if name == "merge_lists":
        return w.merge_lists(i.la, i.lb, l[4])
    if name == "weft_lists":
        return w.weft_lists(*l[:6])
    if name == "render_maps":
        return w.render_maps(*i.seg, coll_offsets=m[0], value=i.mval)
    assert name == "render_lists"
    return w.render_lists(l[0], *i.woven, value=i.lval)


SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.int64): np.int64,
          np.dtype(np.uint8): np.uint8}


def up(x):
    import torch

    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(SIGNED[x.dtype])).to(torch.device("cuda", 0))


def dp(t):
    return t.data_ptr() if t is not None and t.numel() else 0


def zeros(n, dtype):
    return up(np.zeros(max(int(n), 1), dtype))


def down(t, dtype, n):
    return t.cpu().numpy().view(dtype)[:n].copy()


def map_out(n, D):
    cap = max(n, 1)
    return {"seg_offsets": zeros(cap + 1, np.uint64), "seg_coll": zeros(cap, np.uint32),
            "seg_key": zeros(cap, np.uint64), "seg_active": zeros(cap, np.int64),
            "seg_perm": zeros(n + cap, np.uint32), "status": zeros(D, np.uint32)}, cap


def map_result(o, n, S, D):
    return abi.MapResult(down(o["seg_offsets"], np.uint64, S + 1), down(o["seg_coll"], np.uint32, S),
                         down(o["seg_key"], np.uint64, S), down(o["seg_active"], np.int64, S),
                         down(o["seg_perm"], np.uint32, n + S), down(o["status"], np.uint32, D))


def list_out(n, D):
    return {"weave_perm": zeros(n, np.uint32), "visible_bits": zeros((n + 31) // 32 + 1, np.uint32),
            "visible_count": zeros(D, np.uint32), "max_ts": zeros(D, np.uint64), "status": zeros(D, np.uint32),
            "yarn_perm": zeros(n, np.uint32)}


def list_result(o, n, D):
    return abi.ListResult(down(o["weave_perm"], np.uint32, n), down(o["visible_bits"], np.uint32, (n + 31) // 32),
                          down(o["visible_count"], np.uint32, D), down(o["max_ts"], np.uint64, D),
                          down(o["status"], np.uint32, D), down(o["yarn_perm"], np.uint32, n))


def device_call(w, name, i, cap_segs=None):
    """The _device form of a call on device copies of the inputs; the result in
    the shape of the host call's.  cap_segs: a capacity other than the wrappers'."""
    import torch

    m, l = i.m, i.l
    ptrs = lambda xs: [dp(t) for t in xs]
    ptr_dict = lambda o: {k: v.data_ptr() for k, v in o.items()}
    D, LD = len(m[0]) - 1, len(l[0]) - 1
    keep = []  # (the tensors stay alive until the call has been waited for)

    def ups(xs):
        keep.append([up(x) for x in xs])
        return keep[-1]

    try:
        if name == "weave_maps":
            n = int(m[0][-1])
            o, cap = map_out(n, D)
            S = w.weave_maps_device(m[0], ptrs(ups(m[1:5])), m[8], 0, ptr_dict(o), cap_segs or cap)
            torch.cuda.synchronize()
            return map_result(o, n, S, D)
        if name == "merge_maps":
            n = int(i.ma[0][-1] + i.mb[0][-1])
            o, cap = map_out(n, D)
            src = zeros(n, np.uint32)
            mo, S = w.merge_maps_device(i.ma[0], ptrs(ups(i.ma[1:])), i.mb[0], ptrs(ups(i.mb[1:])), m[8], 0,
                                        src.data_ptr(), ptr_dict(o), cap_segs or cap)
            torch.cuda.synchronize()
            M = int(mo[-1])
            return abi.MapMergeResult(mo, down(src, np.uint32, M), map_result(o, M, S, D))
        if name == "weft_maps":
            n = int(m[0][-1]) + (D << m[6])
            o, cap = map_out(n, D)
            src, cut = zeros(n, np.uint32), up(m[7] if len(m[7]) else np.zeros(1, np.uint64))
            ko, S = w.weft_maps_device(m[0], ptrs(ups(m[1:5])), m[8], 0, m[5], m[6], cut.data_ptr(),
                                       src.data_ptr(), ptr_dict(o), cap_segs or cap)
            torch.cuda.synchronize()
            M = int(ko[-1])
            return abi.MapWeftResult(ko, down(src, np.uint32, M), map_result(o, M, S, D))
        if name == "weave_lists":
            n = int(l[0][-1])
            o = list_out(n, LD)
            w.weave_lists_device(l[0], *ptrs(ups(l[1:4])), l[4], ptr_dict(o))
            torch.cuda.synchronize()
            return list_result(o, n, LD)
        if name == "merge_lists":
            n = int(i.la[0][-1] + i.lb[0][-1])
            o, src = list_out(n, LD), zeros(n, np.uint32)
            mo = w.merge_lists_device(i.la[0], ptrs(ups(i.la[1:])), i.lb[0], ptrs(ups(i.lb[1:])), l[4],
                                      src.data_ptr(), ptr_dict(o))
            torch.cuda.synchronize()
            M = int(mo[-1])
            return abi.MergeResult(mo, down(src, np.uint32, M), list_result(o, M, LD))
        if name == "weft_lists":
            n = int(l[0][-1]) + (LD << l[4].site_bits)
            o, src, cut = list_out(n, LD), zeros(n, np.uint32), up(l[5])
            ko = w.weft_lists_device(l[0], ptrs(ups(l[1:4])), l[4], cut.data_ptr(), src.data_ptr(), ptr_dict(o))
            torch.cuda.synchronize()
            M = int(ko[-1])
            return abi.MergeResult(ko, down(src, np.uint32, M), list_result(o, M, LD))
        if name == "render_maps":
            n, sc, sk, sa = i.seg
            S = len(sc)
            key, src, val = zeros(S, np.uint64), zeros(S, np.uint32), zeros(S, np.uint32)
            g = ups((sc, sk, sa, i.mval))
            eo = w.render_maps_device(n, S, dp(g[0]), dp(g[1]), dp(g[2]), key.data_ptr(), src.data_ptr(), m[0],
                                      dp(g[3]), 4, val.data_ptr())
            torch.cuda.synchronize()
            R = int(eo[-1])
            return abi.MapRenderResult(eo, down(key, np.uint64, R), down(src, np.uint32, R), down(val, np.uint32, R))
        assert name == "render_lists"
        n = int(l[0][-1])
        src, val = zeros(n, np.uint32), zeros(n, np.uint64)
        g = ups((i.woven[0], i.woven[1], i.lval))
        ro = w.render_lists_device(l[0], dp(g[0]), dp(g[1]), src.data_ptr(), dp(g[2]), 8, val.data_ptr())
        torch.cuda.synchronize()
        R = int(ro[-1])
        return abi.RenderResult(ro, down(src, np.uint32, R), down(val, np.uint64, R))
    finally:
        torch.cuda.synchronize()


def fresh(name, i, call=host_call):
    with abi.Weaver(0) as w:
        return call(w, name, i)


def stats_of(w, fn):
    """The result of fn() and the kernel stat names it left."""
    w.set_profiling(True)
    w.reset_kernel_stats()
    try:
        res = fn()
        return res, set(w.kernel_stats())
    finally:
        w.set_profiling(False)
        w.reset_kernel_stats()


# ------------------------------------------------------------------ the models ----
class Replay:
    """A weaver whose `name` call returns a result already computed; every other
    call goes to a weaver of its own.  The checkers of the neighbouring tests make
    the call under test themselves: this hands them the one made in the chain."""

    def __init__(self, name, res, ref):
        self._name, self._res, self._ref = name, res, ref

    def __getattr__(self, attr):
        if attr == self._name:
            return lambda *a, **k: self._res
        return getattr(self._ref, attr)


def check_model(name, res, i, ref):
    """One result against the model of its call (ref: a weaver for the reference
    weaves some checkers make)."""
    m, l = i.m, i.l
    D = len(m[0]) - 1
    if name == "weave_maps":
        got, want = gpu_maps(res, D), oracle_maps(*m[:5])
        for d in range(D):
            if not res.status[d] & (abi.STATUS_DUP | abi.STATUS_MAP_KEY):
                assert got[d] == want[d], f"collection {d}"
    elif name == "merge_maps":
        UM.check(Replay(name, res, ref), i.ma, i.mb, m[8])
    elif name == "weft_maps":
        e = MM.weft_maps_expected(*m[:8])
        np.testing.assert_array_equal(res.offsets, e.offsets)
        np.testing.assert_array_equal(res.src, e.src)
        np.testing.assert_array_equal(res.maps.status & abi.STATUS_WEFT, e.weft)
        got = gpu_maps(res.maps, D)
        for d in np.flatnonzero(~e.dup):
            assert got[d] == e.folds[d], f"collection {d}"
    elif name == "weave_lists":
        perm, vis, st = oracle.batch_lists(*l[:4], method=oracle.METHOD_LITERAL)
        empty = np.diff(l[0].astype(np.int64)) == 0
        np.testing.assert_array_equal(res.status[~empty], st[~empty])
        np.testing.assert_array_equal(res.weave_perm, perm)
        np.testing.assert_array_equal(res.visible(), vis)
    elif name == "merge_lists":
        LM.check(Replay(name, res, ref), i.la, i.lb, l[4])
    elif name == "weft_lists":
        e = W.weft_expected(*l[:6])
        np.testing.assert_array_equal(res.offsets, e.offsets)
        np.testing.assert_array_equal(res.src, e.src)
        np.testing.assert_array_equal(res.weave.status, e.status)
        # (the weave of a kept document the oracle flags -- an [id] node is an
        # orphan -- is not specified: the merge checkers skip those as well)
        ko, vis = e.offsets.astype(np.int64), res.weave.visible()
        for d in np.flatnonzero(e.oracle_status == 0):
            lo, hi = ko[d], ko[d + 1]
            np.testing.assert_array_equal(res.weave.weave_perm[lo:hi], e.weave_perm[lo:hi], err_msg=f"document {d}")
            np.testing.assert_array_equal(vis[lo:hi], e.visible[lo:hi], err_msg=f"document {d}")
            assert res.weave.visible_count[d] == e.visible_count[d]
    elif name == "render_maps":
        e = RM.render_maps(*i.seg, coll_offsets=m[0], value=i.mval)
        for f in ("offsets", "key", "src", "value"):
            np.testing.assert_array_equal(getattr(res, f), getattr(e, f), err_msg=f)
    else:
        e = RM.render_lists(l[0], *i.woven, value=i.lval)
        for f in ("offsets", "src", "value"):
            np.testing.assert_array_equal(getattr(res, f), getattr(e, f), err_msg=f)


def test_the_models_alone_give_every_expectation(big):
    """No GPU result enters an expectation: the render inputs are the oracle's
    folds, and each model runs here without a Weaver."""
    e = MM.weft_maps_expected(*big.m[:8])
    assert int(e.offsets[-1]) > 0 and len(big.seg[1]) > 0
    assert int(W.weft_expected(*big.l[:6]).offsets[-1]) > 0
    assert int(RM.render_maps(*big.seg, coll_offsets=big.m[0], value=big.mval).offsets[-1]) > 0
    assert int(RM.render_lists(big.l[0], *big.woven, value=big.lval).offsets[-1]) > 0


# ------------------------------------------------------------------ 1. interleaved calls
@pytest.fixture(scope="module")
def alone(big, small):
    """Every call on a Weaver of its own, in host and in device memory."""
    return {(k, mem, name): fresh(name, i, call)
            for k, i in (("big", big), ("small", small))
            for mem, call in (("host", host_call), ("device", device_call)) for name in ORDER}


@pytest.mark.parametrize("which", ["big", "small"])
def test_interleaved_calls_on_one_context(which, big, small, alone):
    i = big if which == "big" else small
    general = which == "big"
    with abi.Weaver(0) as w, abi.Weaver(0) as ref:
        for mem, call, order in (("host", host_call, ORDER), ("device", device_call, ORDER),
                                 ("host", host_call, ORDER[::-1])):
            first = order is ORDER
            for name in order:
                res, stats = stats_of(w, lambda: call(w, name, i))
                same(res, alone[which, mem, name], f"{name} ({mem})")
                if first:
                    check_model(name, res, i, ref)
                if name in ROUTE:
                    fused, gen = ROUTE[name]
                    assert (gen in stats) == general and (fused in stats) == (not general), (name, stats)


# ------------------------------------------------------------------ 2. growing and shrinking
GROW = ("merge_maps", "weft_maps", "weft_lists", "merge_lists", "render_lists")


def test_layouts_that_grow_and_shrink():
    five = make_inputs((3, 0, 40, 1, 17), (9, 0, 1, 120, 33), 21)
    D = MU_MAXCOLL + 3
    assert D > MW_MAXCOLL  # more than one pack in both map stages
    rng = np.random.default_rng(5)
    many = make_inputs(tuple(int(x) for x in rng.integers(1, 4, D)), tuple(int(x) for x in rng.integers(1, 4, D)), 22)
    # the D = 5 layout again with other ids and cuts
    other = make_inputs((3, 0, 40, 1, 17), (9, 0, 1, 120, 33), 23, split_seed=21)
    for a, b in ((five.m, other.m), (five.ma, other.ma), (five.mb, other.mb), (five.l, other.l),
                 (five.la, other.la), (five.lb, other.lb)):
        np.testing.assert_array_equal(a[0], b[0])
    assert not np.array_equal(five.m[1], other.m[1]) and not np.array_equal(five.l[5], other.l[5])
    failures = []

    def step(what, name, fn):  # (every step runs: one failing call does not hide the others)
        try:
            fn()
        except AssertionError as err:
            failures.append(f"{name}, {what}: {str(err).strip()[:400]}")

    with abi.Weaver(0) as w, abi.Weaver(0) as ref:
        first = {name: host_call(w, name, five) for name in GROW}
        for name in GROW:
            step("D = 5 against the model", name, lambda: check_model(name, first[name], five, ref))
        for name in GROW:
            step(f"D = {D} against the model", name, lambda: check_model(name, host_call(w, name, many), many, ref))
        for name in GROW:
            step("D = 5 again against the first", name, lambda: same(host_call(w, name, five), first[name], name))
        for name in GROW:  # the layout repeats and the data do not
            step("D = 5, other contents, against the model", name,
                 lambda: check_model(name, host_call(w, name, other), other, ref))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ 3. a failure is not sticky
def last_error(w):
    return w._L.cw_last_error(w._h).decode()


@pytest.mark.parametrize("name", ["weave_maps", "merge_maps", "weft_maps"])
def test_cap_segs_too_small_then_enough(name, small):
    with abi.Weaver(0) as w, abi.Weaver(0) as ref:
        with pytest.raises(abi.WeaveError, match="cap_segs too small"):
            device_call(w, name, small, cap_segs=1)
        for call in (device_call, host_call):
            check_model(name, call(w, name, small), small, ref)


def broken(t):
    """The batch with its second offset past its third."""
    off = t[0].copy()
    off[1], off[2] = off[2] + 1, off[1]
    assert off[2] < off[1]
    return (off,) + tuple(t[1:])


def test_non_monotone_layout_then_the_good_one(small):
    i = small
    bad = dataclasses.replace(i, m=broken(i.m), ma=broken(i.ma), l=broken(i.l), la=broken(i.la))
    with abi.Weaver(0) as w, abi.Weaver(0) as ref:
        for name in ("weave_maps", "merge_maps", "weft_maps", "weave_lists", "merge_lists", "weft_lists",
                     "render_lists"):
            good = host_call(w, name, i)
            with pytest.raises(abi.WeaveError, match="not monotone"):
                host_call(w, name, bad)
            after = host_call(w, name, i)
            same(after, good, name)
            check_model(name, after, i, ref)
