"""cw_weave_lists_k128's own front end (k128.hip) at the shapes and words where
it can go wrong (run on the MI355X box: -m gpu): the segmented radix sorts over
documents longer than a tile with 63-bit hi words and lo words that use bit
63, documents decided by one word alone, an all-zero lo column, causes that
match an id in one word only, a repeated id across a tile edge, the one-array
thresholds at 65,535 / 65,536 nodes, several large documents in one call, the
device-memory call with outputs left NULL, and one context across K128 and
K64 calls.

The batches and what is expected of them come from tests/k128_gen.py (proved
on the CPU by tests/test_k128_gen.py): K64 batches widened by strictly
increasing maps per id component, so the oracle's outputs for the K64 batch
are the expectation, computed once per batch and shared.  Every comparison is
equality, per document, of weave_perm, rendered bits, visible_count, status,
max_ts and yarn_perm; only the document deliberately given a repeated id is
skipped for order and visibility (k128_gen.compare asserts that the skipped
set is exactly that one).
"""
import dataclasses

import numpy as np
import pytest

from cause_amd import abi, gen
from tests import k128_gen as K

pytestmark = pytest.mark.gpu

OPTIONS = {"default": {}, "global-sort": {"pack_sort": 0}, "radix": {"front": 0}}
FIELDS = ("weave_perm", "visible_bits", "visible_count", "max_ts", "status", "yarn_perm")


def weave(w, wide, yarns=True):
    return w.weave_lists_k128(wide.off, wide.id2, wide.ca2, wide.kd, yarns=yarns)


def check(options, name, widening, yarns=True):
    wide = K.wide(name, widening)
    with abi.Weaver(0, options=options) as w:
        res = weave(w, wide, yarns)
    K.compare(res, wide, K.expected(name), yarns=yarns)
    return res


# --- tile edges, several documents -------------------------------------------

@pytest.mark.parametrize("widening", ["top", "sparse", "hi_only"])
@pytest.mark.parametrize("config", sorted(OPTIONS))
def test_tile_edges(config, widening):
    """Documents of 0, 1, 2, TILE - 1, TILE, TILE + 1, 2 TILE + 1 and 20,000
    nodes in one batch: the histogram-scan-scatter passes over hi and lo and the
    gather between them, across tile edges."""
    res = check(OPTIONS[config], "edges", widening)
    assert list(res.status) == [abi.STATUS_ROOT] + [0] * 7  # (the empty document has no root)


@pytest.mark.parametrize("name,widening", [("shapes", "top"), ("shapes_one_ts", "lo_only")])
@pytest.mark.parametrize("config", ["default", "radix"])
def test_chain_star_comb_at_tile_edges(config, name, widening):
    """Chain, star and comb at TILE - 1 and TILE + 1 nodes; with one ts for every
    non-root node the order is lo's alone (pairs that differ in bit 63 only, and
    in bit 0 only)."""
    res = check(OPTIONS[config], name, widening)
    assert not res.status.any()


# --- one array: the thresholds -----------------------------------------------

@pytest.mark.parametrize("name,widening,options",
                         [("n65535", "top", {}), ("n65536", "top", {}), ("n65535", "sparse", {}),
                          ("n65536", "sparse", {}), ("n5000", "top", {"giant_min": 0})],
                         ids=["65535-top", "65536-top", "65535-sparse", "65536-sparse", "5000-giant"])
def test_one_document_thresholds(name, widening, options):
    """65,535 nodes: the segmented passes and the per-document tree; 65,536: the
    one-sweep sort and the giant tree; 5,000 under giant_min 0: the giant tree
    behind the segmented passes.  (Under top every non-root hi has bit 62 set, so
    only the root tells whether the sort saw that bit; sparse spreads the hi words
    over all 63.)"""
    res = check(options, name, widening)
    assert not res.status.any()


def test_several_large_documents():
    """70,001, 3,000, 0 and 66,000 nodes: the 64-bit pipeline weaves the large
    documents one by one with tables of their own, and the yarn sort afterwards
    needs the batch's tables again."""
    res = check({}, "several", "sparse")
    assert list(res.status) == [0, 0, abi.STATUS_ROOT, 0]


# --- causes --------------------------------------------------------------------

def test_causes_one_word_hits():
    """Eight 9,000-node documents, each with one cause or id corrupted on the
    wide words (k128_gen.CORRUPTIONS), and a clean one: the literal fold's
    outputs, document by document."""
    wide, e = K.wide("causes", "top"), K.expected("causes")
    res = check({}, "causes", "top")
    want = [bits for _, bits in (wide.claims.get(d, (None, 0)) for d in range(wide.k64.D))]
    assert list(res.status) == want
    assert int((res.status != 0).sum()) == len(K.CORRUPTIONS)  # 8 of 9, as tests/test_k128_gen.py establishes
    dup = K.CAUSE_PLAN.index("dup")
    assert wide.dup_docs == {dup}
    gvis = res.visible()
    for d in (dup - 1, dup + 1, K.CAUSE_PLAN.index(None)):  # the neighbours of the DUP document, the clean one
        lo, hi = wide.k64.span(d)
        assert np.array_equal(res.weave_perm[lo:hi], e.perm[lo:hi]), d
        assert np.array_equal(gvis[lo:hi], e.vis[lo:hi]), d


# --- optional outputs, memory spaces -----------------------------------------

GUARD = 16
_DT = {"weave_perm": "int32", "visible_bits": "int32", "visible_count": "int32", "max_ts": "int64",
       "status": "int32", "yarn_perm": "int32"}


def device_call(w, wide, null=(), stream=None):
    """cw_weave_lists_k128 in device memory: every output filled with 0x55, 16
    guard elements before and after each.  -> name -> numpy array (None for
    an output left NULL); the guards are checked here."""
    import torch

    dev = torch.device("cuda", 0)
    N, D = len(wide.kd), wide.k64.D
    size = {"weave_perm": N, "visible_bits": (N + 31) // 32, "visible_count": D, "max_ts": D,
            "status": D, "yarn_perm": N}
    t = lambda a: torch.from_numpy(np.array(a.view(np.int64) if a.dtype == np.uint64 else a)).to(dev)
    ti, tc, tk = t(wide.id2.reshape(-1)), t(wide.ca2.reshape(-1)), t(wide.kd)
    bufs, ptrs = {}, {}
    for f in FIELDS:
        dt = getattr(torch, _DT[f])
        fill = int.from_bytes(b"\x55" * torch.empty(0, dtype=dt).element_size(), "little")
        bufs[f] = torch.full((size[f] + 2 * GUARD,), fill, dtype=dt, device=dev)
        ptrs[f] = None if f in null else bufs[f].data_ptr() + GUARD * bufs[f].element_size()
    torch.cuda.synchronize()
    w.weave_lists_k128_device(wide.off, ti.data_ptr(), tc.data_ptr(), tk.data_ptr(), ptrs)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    out = {}
    for f in FIELDS:
        a = bufs[f].cpu().numpy()
        fill = np.frombuffer(b"\x55" * a.dtype.itemsize, a.dtype)[0]
        assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all(), f"{f}: guard overwritten"
        body = a[GUARD:len(a) - GUARD]
        if f in null:
            assert (body == fill).all(), f"{f}: NULL output written"
            out[f] = None
        else:
            out[f] = body.view(np.dtype(_DT[f].replace("int", "uint")))
    return out


def as_result(out):
    return abi.ListResult(*[out[f] for f in FIELDS])


@pytest.mark.parametrize("null", [(), ("max_ts",), ("yarn_perm",)], ids=["all", "no-max_ts", "no-yarns"])
def test_device_memory_optional_outputs(null):
    wide = K.wide("edges", "top")
    with abi.Weaver(0) as w:
        out = device_call(w, wide, null)
    K.compare(as_result(out), wide, K.expected("edges"), max_ts="max_ts" not in null,
              yarns="yarn_perm" not in null)


def test_device_memory_async():
    import torch

    wide = K.wide("edges", "top")
    s = torch.cuda.Stream(torch.device("cuda", 0))
    with abi.Weaver(0) as w:
        w.set_stream(s.cuda_stream)
        w.set_async(True)
        out = device_call(w, wide, stream=s)
        again = device_call(w, wide, stream=s)  # the cached tables
    K.compare(as_result(out), wide, K.expected("edges"))
    K.compare(as_result(again), wide, K.expected("edges"))


def test_host_call_without_yarns():
    wide = K.wide("edges", "top")
    with abi.Weaver(0) as w:
        a = weave(w, wide, yarns=True)
        b = weave(w, wide, yarns=False)
    assert b.yarn_perm is None
    K.compare(a, wide, K.expected("edges"))
    K.compare(b, wide, K.expected("edges"), yarns=False)
    for f in FIELDS[:-1]:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


# --- one context, changing calls -----------------------------------------------

def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f"{what}: {f}"


def test_one_context_changing_calls():
    """K128 tile-edge batch, a K64 batch of another layout, the K128 threshold
    document, the tile-edge batch again, all on one context: each result is the
    same call's on a fresh context (the table cache and the sort scratch shared
    with the 64-bit pipeline)."""
    edges, big = K.wide("edges", "sparse"), K.wide("n65536", "top")
    spec = dataclasses.replace(gen.CONFIG2, nodes_per_doc=5_000, n_sites=20, seed=99)
    off, idk, ck, kd = gen.generate(spec, 0, 3)
    lay = spec.layout()
    calls = [("edges", lambda w: weave(w, edges)),
             ("k64", lambda w: w.weave_lists(off, idk, ck, kd, lay)),
             ("n65536", lambda w: weave(w, big)),
             ("edges again", lambda w: weave(w, edges))]
    with abi.Weaver(0) as w:
        got = [call(w) for _, call in calls]
    K.compare(got[0], edges, K.expected("edges"))
    K.compare(got[2], big, K.expected("n65536"))
    K.compare(got[3], edges, K.expected("edges"))
    for (what, call), g in zip(calls, got):
        with abi.Weaver(0) as fresh:
            _same(g, call(fresh), what)
