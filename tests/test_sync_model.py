"""The CPU model of cw_version / cw_delta (tests/sync_model.py) against the
restatements the project already has -- no GPU.

tests/test_gpu_sync.py compares the library with the model array for array;
these tests make the model something independent to compare with: its version
rows are the ends of the yarns of the oracle's spin (group by site, sort by
id), its max_ts the oracle side's, and its delta the complement of what
tests/weft_model.weft_select keeps.
"""
import numpy as np
import pytest

import oracle
from cause_amd import abi_sync, pack  # noqa: F401  (abi_sync: the feature under test)
from tests import sync_model as SM
from tests import weft_model as WM

SIZES = (0, 1, 2, 63, 0, 64, 65, 255, 256, 257, 1023, 1024, 1025, 0)


def batch(n_sites, sizes, seed):
    rng = np.random.default_rng(seed)
    spec = WM.spec_for(n_sites, max(max(sizes) - 1, 1))
    off, idk, ck, kd = WM.ragged(spec, list(sizes), rng)
    return off, idk, ck, kd, spec.layout(), rng


BATCHES = {"bits4": (8, SIZES, 1), "bits1": (1, (1, 2, 3, 0, 300, 700), 2), "bits10": (1000, (2001, 1, 0, 777), 3)}


@pytest.fixture(scope="module", params=sorted(BATCHES))
def case(request):
    return batch(*BATCHES[request.param])


def test_version_rows_are_the_ends_of_the_yarns(case):
    off, idk, ck, kd, lay, _ = case
    ver, ylen, mts = SM.version(off, idk, lay)
    S = 1 << lay.site_bits
    o = off.astype(np.int64)
    for d in range(len(o) - 1):
        ids = idk[o[d]:o[d + 1]]
        yarn = ids[oracle.list_yarns(ids, lay.site_shift, S - 1)]  # the spin: by site, then by id
        site = ((yarn >> np.uint64(lay.site_shift)) & np.uint64(S - 1)).astype(np.int64)
        for r in range(S):
            y = yarn[site == r]
            assert ylen[d * S + r] == len(y)
            assert ver[d * S + r] == (y[-1] if len(y) else 0)          # (peek yarn)
    assert ver.dtype == np.uint64 and ylen.dtype == np.uint32 and mts.dtype == np.uint64
    assert int(ylen.sum()) == len(idk)


def test_the_version_as_a_cut_keeps_every_node_and_max_ts_is_the_oracles(case):
    off, idk, ck, kd, lay, _ = case
    ver, _, mts = SM.version(off, idk, lay)
    e = WM.weft_expected(off, idk, ck, kd, lay, ver)
    assert np.array_equal(e.offsets, off) and np.array_equal(e.kept[0], idk)
    assert np.array_equal(mts, e.max_ts)
    assert not (e.status & 64).any()                                    # no [id] node: every cut is a node


def split_by_doc(off, src):
    o = np.asarray(off, np.uint64).astype(np.int64)
    return [np.asarray(src[o[d]:o[d + 1]]).astype(np.int64) for d in range(len(o) - 1)]


@pytest.mark.parametrize("mode", ["nodes", "closed", "whole", "none"])
def test_delta_is_the_complement_of_the_weft(case, mode):
    """Cut tables whose every named cut is a node of its document: kept_src and
    delta_src are disjoint and together every node (the root is kept)."""
    off, idk, ck, kd, lay, rng = case
    D = len(off) - 1
    cut = WM.make_cuts(off, idk, lay, rng, [mode] * D)
    ko, _, _, _, ksrc, weft = WM.weft_select(off, idk, ck, kd, lay, cut)
    assert not weft.any()
    do, dsrc, did, dca, dkd, dci, ahead = SM.delta(off, idk, lay, cut, cause=ck, kind=kd)
    assert dci is None
    o = off.astype(np.int64)
    for d, (k, dl) in enumerate(zip(split_by_doc(ko, ksrc), split_by_doc(do, dsrc))):
        n = int(o[d + 1] - o[d])
        assert not set(k) & set(dl) and sorted(list(k) + list(dl)) == list(range(n))
        assert list(dl) == sorted(dl)                                   # input order
        root = [i for i in range(n) if kd[o[d] + i] & pack.KIND_ROOT]
        assert set(root) <= set(k)
        assert np.array_equal(did[int(do[d]):int(do[d + 1])], idk[o[d] + dl])
        assert np.array_equal(dca[int(do[d]):int(do[d + 1])], ck[o[d] + dl])
        assert np.array_equal(dkd[int(do[d]):int(do[d + 1])], kd[o[d] + dl])
    assert not ahead.any()                                              # every cut is a node: none above ver


def test_delta_from_nothing_and_from_the_version(case):
    off, idk, ck, kd, lay, _ = case
    D, S = len(off) - 1, 1 << lay.site_bits
    do, dsrc, did, *_, ahead = SM.delta(off, idk, lay, np.zeros(D * S, np.uint64))
    assert np.array_equal(did, idk[idk != 0]) and not ahead.any()
    assert int(do[-1]) == int((idk != 0).sum())
    ver = SM.version(off, idk, lay)[0]
    do, dsrc, did, *_, ahead = SM.delta(off, idk, lay, ver)
    assert not do.any() and len(dsrc) == 0 and len(did) == 0 and not ahead.any()


def test_ahead_counts_the_ranks_raised_above_the_version(case):
    off, idk, ck, kd, lay, rng = case
    D, S = len(off) - 1, 1 << lay.site_bits
    ver = SM.version(off, idk, lay)[0]
    have = ver.copy()
    raised = rng.random(D * S) < 0.3
    have[raised] += np.uint64(1)
    lowered = ~raised & (ver > 0) & (rng.random(D * S) < 0.3)
    have[lowered] -= np.uint64(1)
    do, dsrc, did, *_, ahead = SM.delta(off, idk, lay, have)
    assert np.array_equal(ahead, raised.reshape(D, S).sum(axis=1).astype(np.uint32))
    # one below a head: exactly the head of each lowered rank comes back
    assert sorted(did.tolist()) == sorted(ver[lowered].tolist())


def test_compares_are_unsigned_and_a_foreign_word_is_a_number():
    lay = WM.spec_for(3, 1).layout()
    hi = (1 << 63) | lay.pack(5, 1, 0)                                  # bit 63 set, site rank 1
    ids = np.array([0, lay.pack(1, 1, 0), hi, lay.pack(2, 2, 0), lay.pack(9, 2, 0)], np.uint64)
    off = np.array([0, 5], np.uint64)
    S = 1 << lay.site_bits
    assert ((int(ids[2]) >> lay.site_shift) & (S - 1)) == 1
    ver, ylen, mts = SM.version(off, ids, lay)
    assert ver[1] == hi and ylen[0] == 1 and ver[0] == 0 and ylen[1] == 2 and mts[0] == hi >> lay.ts_shift
    have = np.zeros(S, np.uint64)
    have[1] = lay.pack(1, 1, 0)
    have[2] = lay.pack(3, 1, 0)                                         # rank 2's word carries rank 1's site field
    do, dsrc, did, *_, ahead = SM.delta(off, ids, lay, have)
    assert list(dsrc) == [2, 4] and list(ahead) == [0]
