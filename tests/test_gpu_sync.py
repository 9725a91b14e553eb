"""cw_version and cw_delta on the GPU against tests/sync_model.py, array for
array, bit for bit: in host and in device memory, on every route (asserted
through cw_get_kernel_stats), at every size where the code takes another path;
every error of the header; the chains into the weft and merge calls in device
memory; and the host mirror (causal.versions / deltas / sync_lists / sync_maps)
against merge_lists / merge_maps.
"""
import ctypes as C
import functools
import random
from types import SimpleNamespace as NS

import numpy as np
import pytest

from cause_amd import abi, abi_sync, causal
from tests import mapweft_model as MM
from tests import sync_model as SM
from tests import weft_model as WM
from tests.test_gpu_call_chain import constant, down, dp, list_out, map_out, map_result, up
from tests.test_gpu_maps import gpu_maps

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
WAVE_CAP = abi_sync.WAVE_CAP  # CW_SYNC_WAVE_CAP (tests/test_sync_abi.py pins it to the header)
WG_CAP = constant("listweft.hip", "LW_MAXDOC")
ROUTES = {"default": {}, "no_wave": {"sync_wave": 0}, "general": {"sync_fused": 0}}
FILL = 0x55


# ------------------------------------------------------------------ inputs ----
def list_case(n_sites, sizes, seed):
    """-> (off, (id, cause, kind, None), layout)"""
    rng = np.random.default_rng(seed)
    spec = WM.spec_for(n_sites, max(max(sizes) - 1, 1))
    off, idk, ck, kd = WM.ragged(spec, list(sizes), rng)
    return off, (idk, ck, kd, None), spec.layout()


def map_case(n_sites, sizes, seed):
    """-> (off, (id, cause, kind, cause_is_id), layout)"""
    off, idk, ck, ci, kd, lay, tb = MM.ragged_maps(n_sites, list(sizes), seed, p_bad=0.0)
    return off, (idk, ck, kd, ci), lay


def by_hand():
    """Ids with bit 63 set next to small ones in one site (a signed compare
    fails), a rank whose only node is the root, most ranks absent."""
    lay = NS(ts_shift=20, site_shift=16, site_bits=4)
    pk = lambda ts, r, tx=0: (ts << 20) | (r << 16) | tx
    top = (1 << 44) - 17                                  # ts field: below the 16 reserved top values
    docs = [[0, pk(3, 2), pk(top, 2), pk(1, 2), pk(1 << 43, 2, 5), pk(7, 9)],
            [0],
            [],
            [pk(5, 15), pk(top, 15), pk(top - 1, 1), 0, pk(2, 1)]]
    ids = np.array([x for d in docs for x in d], U64)
    off = np.zeros(len(docs) + 1, U64)
    off[1:] = np.cumsum([len(d) for d in docs])
    assert (ids >> U64(63)).any()
    return off, (ids, ids[::-1].copy(), (np.arange(len(ids)) % 5).astype(U8), None), lay


SMALL = (0, 0, 1, 63, 64, 65, WAVE_CAP - 1, WAVE_CAP, 40, 0, 100, 0)
MIXED = (0, 1, 63, 64, 65, 0, WAVE_CAP - 1, WAVE_CAP, WAVE_CAP + 1, 1023, 1024, 1025, 0)
CASES = {
    "small": lambda: list_case(8, SMALL, 1),                       # wave route
    "mixed": lambda: list_case(8, MIXED, 2),                       # workgroup route
    "maps_small": lambda: map_case(8, SMALL, 3),
    "maps_mixed": lambda: map_case(8, MIXED, 4),
    "bits1": lambda: list_case(1, (1, 2, 3, 0, 300, 64, 700), 5),
    "bits10_wave": lambda: list_case(1000, (100, 0, 256, 1, 17), 6),  # most ranks absent
    "bits10": lambda: list_case(1000, (2001, 1, 0, 300), 7),
    "by_hand": by_hand,
    "all_empty": lambda: (np.zeros(4, U64), (np.zeros(0, U64), np.zeros(0, U64), np.zeros(0, U8), None),
                          NS(ts_shift=20, site_shift=16, site_bits=3)),
    "d0": lambda: (np.zeros(1, U64), (np.zeros(0, U64), np.zeros(0, U64), np.zeros(0, U8), None),
                   NS(ts_shift=20, site_shift=16, site_bits=3)),
    "wg_cap": lambda: list_case(3, (WG_CAP,), 8),                  # the largest workgroup document
    "giant": lambda: list_case(3, (WG_CAP, WG_CAP + 1), 9),        # one document past it: general route
}
# the stats a case shows under the default options: (version, delta)
DEFAULT_STATS = {
    "small": ("sync_ver_wave", "sync_delta_wave"), "mixed": ("sync_ver_wg", "sync_delta_wg"),
    "maps_small": ("sync_ver_wave", "sync_delta_wave"), "maps_mixed": ("sync_ver_wg", "sync_delta_wg"),
    "bits1": ("sync_ver_wg", "sync_delta_wg"), "bits10_wave": ("sync_ver_wave", "sync_delta_wave"),
    "bits10": ("sync_ver_wg", "sync_delta_wg"), "by_hand": ("sync_ver_wave", "sync_delta_wave"),
    "all_empty": (None, "sync_ahead"), "d0": (None, None),
    "wg_cap": ("sync_ver_wg", "sync_delta_wg"), "giant": ("sync_ver_tiled", "sync_delta_write"),
}


def make_have(off, ids, lay, seed):
    """have rows of every kind, by (document + rank) % 6: zero; the head; one
    below a node; between two nodes (no node); above the head; a word carrying
    another rank's site field."""
    rng = np.random.default_rng(seed)
    D, S = len(off) - 1, 1 << lay.site_bits
    ver = SM.version(off, ids, lay)[0]
    have = np.zeros(D * S, U64)
    o = off.astype(np.int64)
    for d in range(D):
        doc = np.sort(ids[o[d]:o[d + 1]])
        site = ((doc >> U64(lay.site_shift)) & U64(S - 1)).astype(np.int64)
        for r in range(S):
            y, k, e = doc[site == r], (d + r) % 6, d * S + r
            if k == 1:
                have[e] = ver[e]
            elif k == 2 and len(y) and int(y[-1]) > 0:
                pick = int(y[int(rng.integers(len(y)))])
                have[e] = max(pick, 1) - 1
            elif k == 3 and len(y) > 1:
                j = int(rng.integers(len(y) - 1))
                have[e] = int(y[j]) + 1 if int(y[j]) + 1 < int(y[j + 1]) else int(y[j])
            elif k == 4:
                have[e] = int(ver[e]) + 1
            elif k == 5:
                ts = (int(doc[int(rng.integers(len(doc)))]) >> lay.ts_shift) if len(doc) else 3
                have[e] = (ts << lay.ts_shift) | (((r + 1) % S) << lay.site_shift)
    return have


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(off, cols, layout, have, the model's version, the model's delta), computed
    once a process; callers leave it unchanged."""
    off, cols, lay = CASES[name]()
    have = make_have(off, cols[0], lay, 77)
    return (off, cols, lay, have, SM.version(off, cols[0], lay),
            SM.delta(off, cols[0], lay, have, cause=cols[1], kind=cols[2], cause_is_id=cols[3]))


@pytest.fixture(scope="module")
def weavers():
    ws = {}
    for route, opts in ROUTES.items():
        ws[route] = abi.Weaver(0, opts)
        ws[route].set_profiling(True)
    yield ws
    for w in ws.values():
        w.close()


# ------------------------------------------------------------------- calls ----
PAD = 8  # elements past the end of every device output, which must stay as filled


def filled(n, dtype):
    return up(np.full(int(n) + PAD, FILL, U8).repeat(np.dtype(dtype).itemsize).view(dtype))


def untouched(t, dtype, n):
    tail = t.cpu().numpy().view(U8)[int(n) * np.dtype(dtype).itemsize:]
    return bool((tail == FILL).all())


def version_call(w, off, ids, lay, mem):
    """-> (ver, yarn_len, max_ts)"""
    import torch

    if mem == "host":
        r = abi_sync.version(w, off, ids, lay)
        return r.ver, r.yarn_len, r.max_ts
    D = len(off) - 1
    words = D << lay.site_bits
    d_ids = up(ids)
    o = {"ver": filled(words, U64), "yarn_len": filled(words, U32), "max_ts": filled(D, U64)}
    abi_sync.version_device(w, off, dp(d_ids), lay, {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    for k, dt, n in (("ver", U64, words), ("yarn_len", U32, words), ("max_ts", U64, D)):
        assert untouched(o[k], dt, n), f"{k}: written past its end"
    return down(o["ver"], U64, words), down(o["yarn_len"], U32, words), down(o["max_ts"], U64, D)


OUT_DT = {"delta_src": U32, "delta_id": U64, "delta_cause": U64, "delta_kind": U8, "delta_cause_is_id": U8}


def delta_call(w, off, cols, lay, have, mem, ahead=True):
    """cols = (id, cause, kind, cause_is_id), None = that column is not given.
    -> the model's tuple (offsets, src, id, cause, kind, cause_is_id, ahead)."""
    import torch

    if mem == "host":
        r = abi_sync.delta(w, off, cols[0], cols[1], cols[2], cols[3], lay, have)
        return (r.delta_offsets, r.delta_src, r.delta_id, r.delta_cause, r.delta_kind, r.delta_cause_is_id, r.ahead)
    D, N = len(off) - 1, len(cols[0])
    dev = [None if c is None else up(c if len(c) else np.zeros(1, c.dtype)) for c in cols]  # (never NULL)
    d_have = up(have if len(have) else np.zeros(1, U64))  # (never NULL, D = 0 included)
    present = {"delta_src": True, "delta_id": True, "delta_cause": cols[1] is not None,
               "delta_kind": cols[2] is not None, "delta_cause_is_id": cols[3] is not None}
    o = {k: filled(N, OUT_DT[k]) for k, yes in present.items() if yes}
    if ahead:
        o["ahead"] = filled(D, U32)
    do = abi_sync.delta_device(w, off, [t.data_ptr() if t is not None else 0 for t in dev], lay, dp(d_have),
                               {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    P = int(do[-1])
    for k in present:
        if k in o:
            assert untouched(o[k], OUT_DT[k], P), f"{k}: written past delta_offsets[D]"
    if ahead:
        assert untouched(o["ahead"], U32, D)
    get = lambda k: down(o[k], OUT_DT[k], P) if k in o else None
    return (do, get("delta_src"), get("delta_id"), get("delta_cause"), get("delta_kind"),
            get("delta_cause_is_id"), down(o["ahead"], U32, D) if ahead else None)


def same_arrays(got, want, what):
    assert len(got) == len(want)
    for j, (g, x) in enumerate(zip(got, want)):
        assert (g is None) == (x is None), f"{what}: array {j}"
        if g is not None:
            assert g.dtype == x.dtype, f"{what}: array {j} is {g.dtype}"
            np.testing.assert_array_equal(g, x, err_msg=f"{what}: array {j}")


def sync_stats(w):
    return {k for k in w.kernel_stats() if k.startswith("sync_")}


def expected_stats(name, route):
    """The stat names of cw_version and of cw_delta (with ahead) for a case."""
    ver, dl = DEFAULT_STATS[name]
    if ver is None:
        return set(), ({dl} if dl else set())
    if route == "no_wave":
        ver, dl = ver.replace("_wave", "_wg"), dl.replace("_wave", "_wg")
    if route == "general" or dl == "sync_delta_write":
        return {"sync_ver_tiled"}, {"sync_ver_tiled", "sync_ahead", "sync_delta_count", "sync_delta_write"}
    return {ver}, {dl}


# ------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_version_and_delta_match_the_model(weavers, name, route, mem):
    off, cols, lay, have, want_v, want_d = prepared(name)
    w = weavers[route]
    vstats, dstats = expected_stats(name, route)
    w.reset_kernel_stats()
    same_arrays(version_call(w, off, cols[0], lay, mem), want_v, f"version {name}")
    assert sync_stats(w) == vstats
    w.reset_kernel_stats()
    same_arrays(delta_call(w, off, cols, lay, have, mem), want_d, f"delta {name}")
    assert sync_stats(w) == dstats


def test_the_cases_cover_what_they_claim():
    sizes = lambda name: np.diff(prepared(name)[0].astype(np.int64))
    assert sizes("small").max() == WAVE_CAP and sizes("mixed").max() > WAVE_CAP
    assert sizes("wg_cap").max() == WG_CAP and sorted(sizes("giant")) == [WG_CAP, WG_CAP + 1]
    for name in ("small", "mixed"):
        s = sizes(name)
        assert s[0] == 0 and s[-1] == 0 and 0 in s[1:-1] and 1 in s      # empty: front, middle, end; root alone
    assert {63, 64, 65, WAVE_CAP - 1, WAVE_CAP, WAVE_CAP + 1, 1023, 1024, 1025} <= set(sizes("mixed"))
    assert prepared("bits1")[2].site_bits == 1 and prepared("bits10")[2].site_bits == 10
    off, cols, lay, have, (ver, ylen, _), (do, *_, ahead) = prepared("bits10_wave")
    assert (ylen == 0).mean() > 0.9                                      # most ranks absent
    off, cols, lay, have, (ver, ylen, _), _ = prepared("mixed")
    S = 1 << lay.site_bits
    assert all(ylen[d * S] == 1 and ver[d * S] == 0 for d in range(len(off) - 1) if off[d + 1] > off[d])
    for name in ("small", "mixed", "maps_mixed", "by_hand"):             # every kind of have row bites
        off, cols, lay, have, (ver, *_), (do, *_, ahead) = prepared(name)
        assert (have == 0).any() and (have == ver).any() and (have > ver).any() and ((have < ver) & (have > 0)).any()
        assert ahead.any() and 0 < int(do[-1]) < len(cols[0])


@pytest.mark.parametrize("mem", ["host", "device"])
def test_optional_outputs_may_be_left_out(weavers, mem):
    """No yarn_len / max_ts; ids only (no gathered column, no delta_id, no ahead)."""
    import torch

    off, cols, lay, have, want_v, want_d = prepared("mixed")
    w = weavers["default"]
    D, N = len(off) - 1, len(cols[0])
    words = D << lay.site_bits
    if mem == "device":
        d_ids, d_have = up(cols[0]), up(have)
        ver, src = filled(words, U64), filled(N, U32)
        abi_sync.version_device(w, off, dp(d_ids), lay, {"ver": ver.data_ptr()})
        do = abi_sync.delta_device(w, off, (dp(d_ids),), lay, dp(d_have), {"delta_src": src.data_ptr()})
        torch.cuda.synchronize()
        got_ver, got_src = down(ver, U64, words), down(src, U32, int(do[-1]))
        assert untouched(src, U32, int(do[-1]))
    else:
        b, keep = abi_sync._host_batch(off, cols[0], None, None, None, lay)
        got_ver, do, got_src = np.full(words, FILL, U64), np.zeros(D + 1, U64), np.full(N, FILL, U32)
        abi_sync.bind(w._L)
        r = abi_sync.CwVersionResult(abi._ptr(got_ver), None, None)
        w._check(w._L.cw_version(w._h, C.byref(b), C.byref(r), abi.CW_MEM_HOST), "cw_version")
        r = abi_sync.CwDeltaResult(abi._u64p(do), abi._ptr(got_src), None, None, None, None, None)
        w._check(w._L.cw_delta(w._h, C.byref(b), abi._ptr(have), C.byref(r), abi.CW_MEM_HOST), "cw_delta")
        assert (got_src[int(do[-1]):] == U32(FILL)).all()
        got_src = got_src[:int(do[-1])]
    np.testing.assert_array_equal(got_ver, want_v[0])
    np.testing.assert_array_equal(do, want_d[0])
    np.testing.assert_array_equal(got_src, want_d[1])


def test_three_thousand_ragged_documents_twice(weavers):
    """0 to 40 nodes a document: the look-back crosses hundreds of workgroups and
    the wave route packs four documents a workgroup.  Twice: equal arrays."""
    rng = np.random.default_rng(11)
    sizes = [int(x) for x in rng.integers(0, 41, 3000)]
    off, cols, lay = map_case(5, sizes, 12)
    have = make_have(off, cols[0], lay, 13)
    want_v = SM.version(off, cols[0], lay)
    want_d = SM.delta(off, cols[0], lay, have, cause=cols[1], kind=cols[2], cause_is_id=cols[3])
    for route in ("default", "no_wave"):
        w = weavers[route]
        w.reset_kernel_stats()
        for _ in range(2):
            same_arrays(version_call(w, off, cols[0], lay, "device"), want_v, "version")
            same_arrays(delta_call(w, off, cols, lay, have, "device"), want_d, "delta")
        tag = "wave" if route == "default" else "wg"
        assert sync_stats(w) == {f"sync_ver_{tag}", f"sync_delta_{tag}"}
        assert w.kernel_stats()[f"sync_delta_{tag}"][0] == 2


def test_delta_from_nothing_and_from_the_own_version(weavers):
    off, cols, lay, _, (ver, *_), _ = prepared("mixed")
    ids = cols[0]
    for route in sorted(ROUTES):
        w = weavers[route]
        do, src, did, *_, ahead = delta_call(w, off, cols, lay, np.zeros_like(ver), "device")
        np.testing.assert_array_equal(did, ids[ids != 0])
        assert not ahead.any()
        do, src, did, *_, ahead = delta_call(w, off, cols, lay, ver, "device")
        assert not do.any() and not ahead.any()


# ------------------------------------------------------------------ errors ----
def raw(w, fn, b, r, have=None, mem=abi.CW_MEM_HOST):
    bind = abi_sync.bind(w._L)
    pb, pr = (C.byref(b) if b is not None else None), (C.byref(r) if r is not None else None)
    rc = bind.cw_version(w._h, pb, pr, mem) if fn == "version" else bind.cw_delta(w._h, pb, have, pr, mem)
    return rc, w._L.cw_last_error(w._h).decode()


def test_every_error_of_the_header(weavers):
    w = weavers["default"]
    lay = NS(ts_shift=20, site_shift=16, site_bits=2)
    off = np.array([0, 2, 3], U64)
    ids, ca, kd, ci = np.array([0, 5 << 20, 9 << 20], U64), np.zeros(3, U64), np.zeros(3, U8), np.ones(3, U8)
    have = np.zeros(8, U64)
    outs, keep = {}, []

    def fresh():
        fill = lambda n, dt: np.full(n * np.dtype(dt).itemsize, FILL, U8).view(dt)  # (every byte)
        outs.update(ver=fill(8, U64), do=fill(3, U64), src=fill(3, U32), oid=fill(3, U64), oca=fill(3, U64),
                    okd=fill(3, U8), oci=fill(3, U8), ahead=fill(2, U32))

    def batch(off=off, ids=ids, cause=ca, kind=kd, cii=ci, n_docs=None, **lay_kw):
        l = NS(**{**vars(lay), **lay_kw})
        keep.append(off)  # (the struct holds addresses only)
        return abi_sync.CwSyncBatch(len(off) - 1 if n_docs is None else n_docs, abi._u64p(off), abi._ptr(ids),
                                    abi._ptr(cause), abi._ptr(kind), abi._ptr(cii), l.ts_shift, l.site_shift,
                                    l.site_bits, 0)

    def vres(ver=True):
        return abi_sync.CwVersionResult(abi._ptr(outs["ver"]) if ver else None, None, None)

    def dres(do=True, src=True, oca=True, okd=True, oci=True):
        p = lambda k, yes: abi._ptr(outs[k]) if yes else None
        return abi_sync.CwDeltaResult(abi._u64p(outs["do"]) if do else None, p("src", src), p("oid", True),
                                      p("oca", oca), p("okd", okd), p("oci", oci), p("ahead", True))

    def refused(fn, b, r, why, have=abi._ptr(have), mem=abi.CW_MEM_HOST):
        rc, err = raw(w, fn, b, r, have, mem)
        assert rc < 0 and why in err, (fn, why, rc, err)
        for k, v in outs.items():
            assert (v.view(U8) == FILL).all(), f"{fn} ({why}) wrote {k}"

    fresh()
    assert raw(w, "version", batch(), vres())[0] == 0 and raw(w, "delta", batch(), dres(), abi._ptr(have))[0] == 0
    assert list(outs["do"]) == [0, 1, 2] and list(outs["src"][:2]) == [1, 0]
    fresh()
    big, wide = np.array([0, 0xFFFFFFFF], U64), np.zeros(1, U64)
    for fn, res in (("version", vres), ("delta", dres)):
        refused(fn, None, res(), "null batch")
        refused(fn, batch(), None, "null batch")
        refused(fn, batch(), res(), "memspace", mem=7)
        refused(fn, batch(site_bits=0), res(), "site_bits")
        refused(fn, batch(site_bits=11), res(), "site_bits")
        refused(fn, batch(site_shift=64), res(), "key layout")
        refused(fn, batch(ts_shift=64), res(), "key layout")
        refused(fn, batch(off=np.array([1, 2, 3], U64)), res(), "must be 0")
        refused(fn, batch(off=np.array([0, 3, 2], U64)), res(), "monotone")
        refused(fn, batch(ids=None), res(), "id_key")
        refused(fn, batch(off=big), res(), "N=")
        refused(fn, batch(off=wide, n_docs=1 << 30), res(), "documents of")        # (1 << 30) << 2 = 2^32
        refused(fn, batch(off=wide, n_docs=1 << 22, site_bits=10), res(), "documents of")
        refused(fn, batch(off=wide, n_docs=1 << 22), res(), "in one dispatch")              # a workgroup a document
    b = batch()
    b.doc_offsets = None
    refused("version", b, vres(), "doc_offsets")
    refused("version", batch(), vres(ver=False), "ver")
    refused("delta", batch(), dres(), "have", have=None)
    refused("delta", batch(off=wide, ids=None), dres(), "have", have=None)                  # with no document too
    refused("delta", batch(), dres(do=False), "delta_offsets")
    refused("delta", batch(), dres(src=False), "delta_src")
    # a gathered output exactly when its input column
    refused("delta", batch(cause=None), dres(), "delta_cause")
    refused("delta", batch(), dres(oca=False), "delta_cause")
    refused("delta", batch(kind=None), dres(), "delta_kind")
    refused("delta", batch(), dres(okd=False), "delta_kind")
    refused("delta", batch(cii=None), dres(), "delta_cause_is_id")
    refused("delta", batch(), dres(oci=False), "delta_cause_is_id")
    # the context still works
    assert raw(w, "delta", batch(cii=None), dres(oci=False), abi._ptr(have))[0] == 0


# ------------------------------------------------------------------ chains ----
def id_weaves(off, ids, perm):
    """Per document the ids in weave order."""
    o = np.asarray(off, U64).astype(np.int64)
    return [ids[o[d]:o[d + 1]][perm[o[d]:o[d + 1]].astype(np.int64)].tolist() for d in range(len(o) - 1)]


def weft_lists_dev(w, off, d_cols, lay, d_cut, n_cap):
    """cw_weft_lists_dev -> (kept offsets, kept_src, weave_perm), host arrays."""
    import torch

    D = len(off) - 1
    o, src = list_out(n_cap, D), up(np.zeros(max(n_cap, 1), U32))
    ko = w.weft_lists_device(off, [dp(t) for t in d_cols[:3]], lay, dp(d_cut), src.data_ptr(),
                             {k: v.data_ptr() for k, v in o.items()})
    torch.cuda.synchronize()
    M = int(ko[-1])
    return ko, down(src, U32, M), down(o["weave_perm"], U32, M), down(o["status"], U32, D)


def test_the_version_is_the_cut_of_now_lists(weavers):
    """ver as the cut of cw_weft_lists_dev, in device memory: every node kept,
    the weave that of cw_weave_lists."""
    import torch

    off, cols, lay = list_case(8, (0, 1, 63, 300, 0, 1025, 40), 21)
    w = weavers["default"]
    D, N = len(off) - 1, len(cols[0])
    words = D << lay.site_bits
    d_cols = [up(c) for c in cols[:3]]
    ver = up(np.zeros(words, U64))
    abi_sync.version_device(w, off, dp(d_cols[0]), lay, {"ver": ver.data_ptr()})
    ko, src, perm, st = weft_lists_dev(w, off, d_cols, lay, ver, N + words)
    np.testing.assert_array_equal(ko, off)
    o = off.astype(np.int64)
    np.testing.assert_array_equal(src, np.concatenate([np.arange(o[d + 1] - o[d]) for d in range(D)]).astype(U32))
    assert not (st & abi.STATUS_WEFT).any()
    full = w.weave_lists(off, *cols[:3], lay)
    assert id_weaves(off, cols[0], perm) == id_weaves(off, cols[0], full.weave_perm)
    torch.cuda.synchronize()


def map_id_weaves(res, D, off, ids):
    """Per collection {key: (id of the active node or -1, ids in weave order)}."""
    o = np.asarray(off, U64).astype(np.int64)
    out = []
    for d, folds in enumerate(gpu_maps(res, D)):
        doc = ids[o[d]:o[d + 1]]
        out.append({k: (int(doc[a]) if a >= 0 else -1, [int(doc[p]) for p in perm]) for k, (a, perm) in folds.items()})
    return out


def test_the_version_is_the_cut_of_now_maps(weavers):
    import torch

    off, idk, ck, ci, kd, lay, tb = MM.ragged_maps(8, [0, 1, 37, 300, 0, 64], 22, p_bad=0.0)
    w = weavers["default"]
    D, N = len(off) - 1, len(idk)
    words = D << lay.site_bits
    d_cols = [up(c) for c in (idk, ck, ci, kd)]
    ver = up(np.zeros(words, U64))
    abi_sync.version_device(w, off, dp(d_cols[0]), lay, {"ver": ver.data_ptr()})
    n = N + words
    o, cap = map_out(n, D)
    src = up(np.zeros(max(n, 1), U32))
    ko, S = w.weft_maps_device(off, [dp(t) for t in d_cols], tb, 0, lay.site_shift, lay.site_bits, dp(ver),
                               src.data_ptr(), {k: v.data_ptr() for k, v in o.items()}, cap)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ko, off)
    got = map_result(o, N, S, D)
    assert not (got.status & abi.STATUS_WEFT).any()
    full = w.weave_maps(off, idk, ck, ci, kd, tb)
    assert map_id_weaves(got, D, off, idk) == map_id_weaves(full, D, off, idk)


def node_cuts(off, ids, lay, seed):
    D = len(off) - 1
    return WM.make_cuts(off, ids, lay, np.random.default_rng(seed), ["closed", "whole", "none", "nodes"] * D)


def test_weft_plus_delta_is_the_document_lists(weavers):
    """For cuts that are nodes: the kept nodes of cw_weft_lists_dev (side a) and
    cw_delta's gathered columns at the same table (side b), merged by
    cw_merge_lists, weave as the full document.  All in device memory."""
    import torch

    off, cols, lay = list_case(8, (0, 1, 63, 300, 0, 1025, 40, 257), 23)
    w = weavers["default"]
    D, N = len(off) - 1, len(cols[0])
    words = D << lay.site_bits
    cut = node_cuts(off, cols[0], lay, 24)
    d_cols, d_cut = [up(c) for c in cols[:3]], up(cut)
    ko, ksrc, _, st = weft_lists_dev(w, off, d_cols, lay, d_cut, N + words)
    assert not (st & abi.STATUS_WEFT).any()
    o = off.astype(np.int64)
    kb = ko.astype(np.int64)
    glob = up(np.concatenate([o[d] + ksrc[kb[d]:kb[d + 1]].astype(np.int64) for d in range(D)]).astype(np.int64))
    side_a = [t[glob.view(torch.int64)] if len(ksrc) else t[:0] for t in d_cols]
    outs = {k: up(np.zeros(N, dt)) for k, dt in (("delta_src", U32), ("delta_id", U64), ("delta_cause", U64),
                                                 ("delta_kind", U8))}
    do = abi_sync.delta_device(w, off, [dp(t) for t in d_cols], lay, dp(d_cut), {k: v.data_ptr() for k, v in outs.items()})
    assert int(ko[-1]) + int(do[-1]) == N and 0 < int(do[-1]) < N
    mo, msrc = list_out(N, D), up(np.zeros(N, U32))
    a_ptrs = [dp(t) for t in side_a] + [dp(side_a[0])]                       # (the ids as value tokens)
    b_ptrs = [dp(outs["delta_id"]), dp(outs["delta_cause"]), dp(outs["delta_kind"]), dp(outs["delta_id"])]
    moff = w.merge_lists_device(ko, a_ptrs, do, b_ptrs, lay, msrc.data_ptr(), {k: v.data_ptr() for k, v in mo.items()})
    torch.cuda.synchronize()
    np.testing.assert_array_equal(moff, off)
    a_ids, b_ids, src = side_a[0].cpu().numpy().view(U64), down(outs["delta_id"], U64, int(do[-1])), down(msrc, U32, N)
    db = do.astype(np.int64)
    merged = np.concatenate([np.concatenate([a_ids[kb[d]:kb[d + 1]], b_ids[db[d]:db[d + 1]]])[src[o[d]:o[d + 1]]]
                             for d in range(D)])
    full = w.weave_lists(off, *cols[:3], lay)
    np.testing.assert_array_equal(down(mo["status"], U32, D), full.status)
    assert not full.status[np.diff(o) > 0].any()
    assert id_weaves(off, merged, down(mo["weave_perm"], U32, N)) == id_weaves(off, cols[0], full.weave_perm)


def test_weft_plus_delta_is_the_document_maps(weavers):
    import torch

    off, idk, ck, ci, kd, lay, tb = MM.ragged_maps(8, [0, 1, 37, 300, 0, 64, 257], 25, p_bad=0.0)
    w = weavers["default"]
    D, N = len(off) - 1, len(idk)
    words = D << lay.site_bits
    cut = node_cuts(off, idk, lay, 26)
    d_cols, d_cut = [up(c) for c in (idk, ck, ci, kd)], up(cut)
    n = N + words
    wo, cap = map_out(n, D)
    wsrc = up(np.zeros(max(n, 1), U32))
    ko, _ = w.weft_maps_device(off, [dp(t) for t in d_cols], tb, 0, lay.site_shift, lay.site_bits, dp(d_cut),
                               wsrc.data_ptr(), {k: v.data_ptr() for k, v in wo.items()}, cap)
    torch.cuda.synchronize()
    ksrc = down(wsrc, U32, int(ko[-1]))
    o, kb = off.astype(np.int64), ko.astype(np.int64)
    glob = up(np.concatenate([o[d] + ksrc[kb[d]:kb[d + 1]].astype(np.int64) for d in range(D)]).astype(np.int64))
    side_a = [t[glob.view(torch.int64)] for t in d_cols]
    outs = {k: up(np.zeros(N, dt)) for k, dt in (("delta_src", U32), ("delta_id", U64), ("delta_cause", U64),
                                                 ("delta_kind", U8), ("delta_cause_is_id", U8))}
    do = abi_sync.delta_device(w, off, [dp(d_cols[0]), dp(d_cols[1]), dp(d_cols[3]), dp(d_cols[2])], lay, dp(d_cut),
                               {k: v.data_ptr() for k, v in outs.items()})
    assert int(ko[-1]) + int(do[-1]) == N and 0 < int(do[-1]) < N
    mo, mcap = map_out(N, D)
    msrc = up(np.zeros(N, U32))
    a_ptrs = [dp(t) for t in side_a] + [dp(side_a[0])]
    b_ptrs = [dp(outs[k]) for k in ("delta_id", "delta_cause", "delta_cause_is_id", "delta_kind", "delta_id")]
    moff, S = w.merge_maps_device(ko, a_ptrs, do, b_ptrs, tb, 0, msrc.data_ptr(),
                                  {k: v.data_ptr() for k, v in mo.items()}, mcap)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(moff, off)
    got = map_result(mo, N, S, D)
    a_ids, b_ids, src = side_a[0].cpu().numpy().view(U64), down(outs["delta_id"], U64, int(do[-1])), down(msrc, U32, N)
    db = do.astype(np.int64)
    merged = np.concatenate([np.concatenate([a_ids[kb[d]:kb[d + 1]], b_ids[db[d]:db[d + 1]]])[src[o[d]:o[d + 1]]]
                             for d in range(D)])
    full = w.weave_maps(off, idk, ck, ci, kd, tb)
    assert map_id_weaves(got, D, off, merged) == map_id_weaves(full, D, off, idk)


# ------------------------------------------------------------- host mirror ----
def replica_pairs(kind, n_pairs, seed):
    """A common history, after which each replica appends from its own site and
    takes a prefix of the other's appends: each holds a prefix of every yarn."""
    rng = random.Random(seed)
    pairs = []
    for p in range(n_pairs):
        sites = sorted(causal.new_site_id(rng) for _ in range(4))
        sa, sb = sites[0], sites[1]
        nodes, ts = ([causal.ROOT_NODE] if kind == "list" else []), 0

        def grow(have, site, count):
            nonlocal ts
            made = []
            for _ in range(count):
                ts += 1
                if kind == "list":
                    cause = rng.choice(have + made)[0]
                else:
                    ids = [n[0] for n in have + made]
                    cause = rng.choice(ids) if ids and rng.random() < 0.3 else f"k{rng.randrange(5)}"
                value = causal.HIDE if rng.random() < 0.15 and kind == "list" and cause != causal.ROOT_ID else f"v{ts}"
                made.append((( ts, site, 0), cause, value))
            return made

        for _ in range(rng.randrange(0, 12)):
            nodes += grow(nodes, rng.choice(sites), 1)
        own_a = grow(nodes, sa, rng.randrange(0, 8 + 5 * p))
        own_b = grow(nodes, sb, rng.randrange(0, 8 + 5 * p))
        a = nodes + own_a + own_b[:rng.randrange(0, len(own_b) + 1)]
        b = nodes + own_b + own_a[:rng.randrange(0, len(own_a) + 1)]
        new = causal.new_list_ct if kind == "list" else causal.new_map_ct
        uuid = causal._uid(rng, 21)
        cts = []
        for site, ns in ((sa, a), (sb, b)):
            ct = new(site_id=site, uuid=uuid)
            rng.shuffle(ns)
            ct["nodes"] = {n[0]: (n[1], n[2]) for n in ns}
            ct["lamport_ts"] = max([0] + [n[0][0] for n in ns])
            cts.append(ct)
        pairs.append(tuple(cts))
    return pairs


@pytest.mark.parametrize("kind", ["list", "map"])
def test_sync_equals_merge(kind, monkeypatch):
    pairs = replica_pairs(kind, 20, 31 if kind == "list" else 32)
    merge, sync, call = ((causal.merge_lists, causal.sync_lists, "merge_lists") if kind == "list" else
                         (causal.merge_maps, causal.sync_maps, "merge_maps"))
    want = merge(pairs)
    back = merge([(b, a) for a, b in pairs])
    w = causal.weaver()
    seen = []
    orig = getattr(w, call)
    monkeypatch.setattr(w, call, lambda a, b, *rest: (seen.append((a, b)), orig(a, b, *rest))[1])
    got = sync(pairs, both=True)
    assert [g[0] for g in got] == want
    assert [g[1] for g in got] == back
    assert sync(pairs) == want
    # each replica met only the other's delta
    (a, b), _ = seen
    lacks = [len(set(y["nodes"]) - set(x["nodes"])) for p in pairs for x, y in (p, p[::-1])]
    assert np.diff(np.asarray(b[0]).astype(np.int64)).tolist() == lacks
    assert len(b[1]) == sum(lacks) and 0 < sum(lacks) < len(a[1]) / 2
    assert len(a[1]) == sum(len(x["nodes"]) for p in pairs for x in p)


def test_versions_and_deltas_of_a_mixed_batch():
    lists, maps = replica_pairs("list", 6, 41), replica_pairs("map", 6, 42)
    pairs = [p for two in zip(lists, maps) for p in two]
    cts = [ct for p in pairs for ct in p]
    vers = causal.versions(cts)
    key = lambda i: (i[0], i[2])
    for ct, ver in zip(cts, vers):
        want = {}
        for i in ct["nodes"]:
            if i != causal.ROOT_ID and (i[1] not in want or key(i) > key(want[i[1]])):
                want[i[1]] = i
        assert ver == want
    items = [(x, vers[2 * p + 1 - j]) for p, pair in enumerate(pairs) for j, x in enumerate(pair)]
    got = causal.deltas(items)
    for (x, _), y, nodes in zip(items, [ct for p in pairs for ct in p[::-1]], got):
        lacking = sorted(set(x["nodes"]) - set(y["nodes"]), key=lambda i: (i[0], i[1].encode("utf-16-be"), i[2]))
        assert [n[0] for n in nodes] == lacking
        assert all(tuple(n[1:]) == tuple(x["nodes"][n[0]]) for n in nodes)
    assert sum(len(n) for n in got) > 20
    assert causal.deltas([(cts[0], {})])[0] == sorted(
        ((i,) + tuple(b) for i, b in cts[0]["nodes"].items() if i != causal.ROOT_ID), key=lambda n: key(n[0]))
