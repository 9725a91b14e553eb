"""CPU model of cw_version and cw_delta at array level (a helper, not a test).

Plain numpy / Python, one document at a time, written from the rules of
include/causeweave_sync.h; it shares no code with sync.hip.
tests/test_sync_model.py pins it to the restatements the project already has
(the spin of oracle/causal_ref.py, tests/weft_model.weft_select),
tests/test_gpu_sync.py compares the library with it array for array.
"""
from __future__ import annotations

import numpy as np


def _rank(ids, layout):
    return ((ids >> np.uint64(layout.site_shift)) & np.uint64((1 << layout.site_bits) - 1)).astype(np.int64)


def version(offsets, id_key, layout):
    """-> (ver u64[D << site_bits], yarn_len u32[D << site_bits], max_ts u64[D])."""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    idk = np.asarray(id_key, np.uint64)
    D, S = len(off) - 1, 1 << layout.site_bits
    ver, ylen, mts = np.zeros(D * S, np.uint64), np.zeros(D * S, np.uint32), np.zeros(D, np.uint64)
    for d in range(D):
        ids = idk[off[d]:off[d + 1]]
        for x, r in zip(ids.tolist(), _rank(ids, layout).tolist()):  # Python ints: unsigned by nature
            ver[d * S + r] = max(int(ver[d * S + r]), x)
            ylen[d * S + r] += 1
        mts[d] = (max(ids.tolist()) >> layout.ts_shift) if len(ids) else 0
    return ver, ylen, mts


def delta(offsets, id_key, layout, have, cause=None, kind=None, cause_is_id=None):
    """-> (delta_offsets u64[D+1], delta_src u32[P], delta_id u64[P], delta_cause,
    delta_kind, delta_cause_is_id (None where the column is), ahead u32[D])."""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    idk, have = np.asarray(id_key, np.uint64), np.asarray(have, np.uint64)
    D, S = len(off) - 1, 1 << layout.site_bits
    assert len(have) == D * S
    ver = version(offsets, id_key, layout)[0]
    do, src, glob = np.zeros(D + 1, np.uint64), [], []
    for d in range(D):
        ids = idk[off[d]:off[d + 1]]
        row = have[d * S:(d + 1) * S].tolist()
        k = [i for i, (x, r) in enumerate(zip(ids.tolist(), _rank(ids, layout).tolist())) if x > row[r]]
        src += k
        glob += [int(off[d]) + i for i in k]
        do[d + 1] = do[d] + np.uint64(len(k))
    g = np.array(glob, np.int64)
    col = lambda x, dt: None if x is None else np.asarray(x, dt)[g]
    ahead = np.array([sum(h > v for h, v in zip(have[d * S:(d + 1) * S].tolist(), ver[d * S:(d + 1) * S].tolist()))
                      for d in range(D)], np.uint32)
    return (do, np.array(src, np.uint32), idk[g], col(cause, np.uint64), col(kind, np.uint8),
            col(cause_is_id, np.uint8), ahead)
