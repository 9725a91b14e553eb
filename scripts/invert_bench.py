"""Time cw_invert on the GPU: the undo of one tx per base, and a reset of whole histories.

    python scripts/invert_bench.py [--bases 10000] [--steps 20] [--out profiles/invert_bench.txt]

Config 4's shape (gen.CONFIG4: collections of 100 nodes) in device memory,
--bases bases of 100 collections each.  The generator's ids are unique per
collection only, so they are re-keyed into a layout with 14 tx bits, the
collection's index in its base as the tx-index: unique across the base, and
one (ts, site) is a tx of up to 100 nodes, one a collection.  ref_doc is given
(no node refers to a collection).

Two slices, one JSON line each (also appended to --out):
  undo   per base the newest (ts, site) of the base: sel_lo .. sel_hi is that
         tx-id's key range, sel_sites its site alone;
  reset  the whole history of every site: 10,000 candidates a base, above
         invert_cap, so the call takes the general route (the key sort).
Reported: the median, min, max and interquartile spread of --steps timed calls
(host clock, the call's wait included); per kernel stat the event time
(cw_ctx_set_profiling), the algorithmic bytes and GB/s on them; for
k_invert_mark also the fraction of the 8.0 TB/s HBM peak and, measured in the
same run, the time of a device-to-device copy that reads and writes as many
bytes as the pass's algorithmic bytes.  The parts of the first call are compared
with a numpy reading of the slice before anything is timed.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PER_BASE = 100
TX_BITS = 14


def spread(t):
    q = np.percentile(t, [25, 50, 75])
    return {"median": round(float(q[1]), 3), "min": round(float(np.min(t)), 3), "max": round(float(np.max(t)), 3),
            "iqr": round(float(q[2] - q[0]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import HBM_TBS, emit, timed, up, z
    from cause_amd import abi, abi_invert, gen
    from cause_amd.pack import KeyLayout

    note = lambda what: print(f"[invert_bench] {what}", file=sys.stderr, flush=True)
    spec = gen.CONFIG4
    old, _ = spec.layout()
    lay = KeyLayout(old.ts_bits + 1, old.site_bits, TX_BITS)
    G, D = a.bases, a.bases * PER_BASE
    note("generating the collections")
    off, idk, ck, ci, kd = gen.generate_maps(spec, 0, D, nthreads=16)
    N = len(idk)
    o64 = off.astype(np.int64)
    tx = np.repeat(np.arange(D, dtype=np.uint64) % np.uint64(PER_BASE), np.diff(o64))
    smask = np.uint64((1 << old.site_bits) - 1)
    rekey = lambda k: ((k >> np.uint64(old.ts_shift)) << np.uint64(lay.ts_shift)) | \
        (((k >> np.uint64(old.site_shift)) & smask) << np.uint64(lay.site_shift)) | tx
    idk = rekey(idk)
    ck = np.where((ci == 1) & (ck != 0), rekey(ck), ck)
    boff = (np.arange(G + 1, dtype=np.uint64) * np.uint64(PER_BASE))
    node_base = o64[boff.astype(np.int64)]
    top = np.maximum.reduceat(idk, node_base[:-1])                       # each base's newest id
    txmask = np.uint64((1 << TX_BITS) - 1)
    W = abi_invert.mask_words(lay.site_bits)
    new_tx = ((top >> np.uint64(lay.ts_shift)) + np.uint64(1)) << np.uint64(lay.ts_shift)
    slices = {
        "undo": (top & ~txmask, top | txmask,
                 (np.uint64(1) << ((top >> np.uint64(lay.site_shift)) & smask)).repeat(W).reshape(G, W)),
        "reset": (np.zeros(G, np.uint64), np.full(G, (1 << 63) - 1, np.uint64),
                  np.full((G, W), 2 ** 64 - 1, np.uint64)),
    }
    assert W == 1
    ref = np.full(N, 0xFFFFFFFF, np.uint32)
    torch.cuda.init()
    g = [up(x) for x in (idk, ck, kd, ci, ref)]
    gtx = up(new_tx)
    o = {"inv_id": z(N, torch.int64), "inv_cause": z(N, torch.int64), "inv_cause_is_id": z(N, torch.uint8),
         "inv_kind": z(N, torch.uint8), "inv_src": z(N, torch.int32), "base_parts": z(G, torch.int32),
         "status": z(D, torch.int32)}
    ptrs = {k: v.data_ptr() for k, v in o.items()}
    w = abi.Weaver(0)
    for name, (lo, hi, sites) in slices.items():
        note(name)
        gs = [up(lo), up(hi), up(np.ascontiguousarray(sites).reshape(-1))]
        torch.cuda.synchronize()
        call = lambda: abi_invert.invert_device(w, off, [t.data_ptr() for t in g[:3]], lay, boff,
                                                [t.data_ptr() for t in gs] + [gtx.data_ptr()], ptrs,
                                                cause_is_id_ptr=g[3].data_ptr(), ref_doc_ptr=g[4].data_ptr())
        po = call()                                                    # warm-up, and the comparison
        torch.cuda.synchronize()
        rank = (idk >> np.uint64(lay.site_shift)) & smask
        nb = np.repeat(np.arange(G), np.diff(node_base))
        sel = (idk >= lo[nb]) & (idk <= hi[nb]) & (((sites[nb, 0] >> rank) & np.uint64(1)) == 1)
        status = o["status"].cpu().numpy()
        parts = o["base_parts"].cpu().numpy().view(np.uint32)
        assert int(po[-1]) == int(parts.sum())
        if int(sel.sum()) <= 5_000_000 and not status.any():
            # the parts are the distinct (collection, cause_is_id, cause) of the inverted selected nodes
            at = np.flatnonzero(sel)
            normal = (kd[at] & 3) == 0
            kci = np.where(normal, 1, ci[at]).astype(np.uint64)
            kca = np.where(normal, idk[at], np.where(ci[at] == 2, np.uint64(0), ck[at]))
            doc = (np.searchsorted(o64, at, side="right") - 1).astype(np.uint64)
            want = len(np.unique(np.stack([doc, kci, kca], axis=1), axis=0))
            assert int(po[-1]) == want, (int(po[-1]), want)
        times = [timed(call)[0] for _ in range(a.steps)]
        w.reset_kernel_stats()
        w.set_profiling(True)
        for _ in range(a.steps):
            call()
        w.set_profiling(False)
        kernels = {}
        for kname, (launches, ms, by) in sorted(w.kernel_stats().items()):
            ms, by = ms / launches, by / launches
            kernels[kname] = {"launches_a_call": launches / a.steps, "ms": round(ms, 4), "bytes_alg": by,
                              "gb_per_s": round(by / (ms / 1e3) / 1e9, 1)}
        w.reset_kernel_stats()
        mark = kernels["k_invert_mark"]
        mark["frac_of_hbm_peak"] = round(mark["gb_per_s"] / 1e3 / HBM_TBS, 3)
        nbytes = int(mark["bytes_alg"])
        src_, dst_ = z(nbytes, torch.uint8), z(nbytes, torch.uint8)
        dst_.copy_(src_)
        copies = [timed(lambda: dst_.copy_(src_))[0] for _ in range(a.steps)]
        del src_, dst_
        emit({"what": f"cw_invert, {name}: {G} bases of {PER_BASE} config-4 collections, device memory",
              "bases": G, "docs": D, "nodes": N, "selected": int(sel.sum()), "parts": int(po[-1]),
              "bases_over_the_tx_field": int((status.reshape(G, PER_BASE)[:, 0] != 0).sum()),
              "steps": a.steps, "build": abi.build_id(), "call_ms": spread(times), "kernels": kernels,
              "mark_bytes_a_node": round(mark["bytes_alg"] / N, 3),
              "d2d_copy_of_mark_bytes_ms": spread(copies)}, a.out)
    w.close()


if __name__ == "__main__":
    main()
