"""cw_insert_maps against the parent's only route for "every map receives one tx":
cw_merge_maps with the tx as side b (a union, a dedup and a full reweave).

Config 4's shape (gen.CONFIG4: 10^6 collections of 100 nodes), woven once by
cw_weave_maps, everything resident in device memory.  Two workloads: one
1-node tx a collection (an assoc on one of the collection's keys, a fresh
Lamport id) and one 8-node tx over distinct keys (a transacted map literal).
The two calls alternate in one process; before timing their results are
compared: key weaves as id sequences, and active ids (merged_src is in id
order, so the indices differ).  Times are on the host clock around the
synchronised call; per kernel the event time, the algorithmic bytes and the
fraction of the HBM peak.  One JSON line a workload.

    python scripts/map_insert_bench.py [--colls 1000000] [--steps 20] [--out profiles/map_insert_bench.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(t):
    q = np.percentile(t, [25, 50, 75])
    return {"median": round(float(q[1]), 3), "min": round(float(np.min(t)), 3), "max": round(float(np.max(t)), 3),
            "iqr": round(float(q[2] - q[0]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--colls", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import emit, hbm, kernel_ms, map_outs, timed, up, z
    from cause_amd import abi, abi_map_insert, gen

    torch.cuda.init()
    spec = gen.CONFIG4
    lay, tb = spec.layout()
    off, idk, ck, ci, kd = gen.generate_maps(spec, 0, a.colls, nthreads=16)
    N, D = len(idk), a.colls
    o64 = off.astype(np.int64)
    val = np.arange(N, dtype=np.uint64)
    g = [up(x) for x in (idk, ck, ci, kd, val)]
    w = abi.Weaver(0)
    so, souts = map_outs(N, N, D)
    S = w.weave_maps_device(off, [t.data_ptr() for t in g[:4]], tb, lay.key_bits, souts, N)
    assert int(so["status"].max().item()) == 0
    segp = [so[k].data_ptr() for k in ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm")]
    rng = np.random.default_rng(4)
    n_d = np.diff(o64)
    top = np.maximum.reduceat(idk >> np.uint64(lay.ts_shift), o64[:-1]) if N else np.zeros(D, np.uint64)
    first_key = np.array([0])
    for k in (1, 8):
        T = D * k
        toff = (np.arange(D + 1, dtype=np.uint64) * np.uint64(k))
        j = np.tile(np.arange(k, dtype=np.uint64), D)
        tid = (np.repeat(top, k) + np.uint64(1) + j) << np.uint64(lay.ts_shift)
        if k == 1:   # a key of the collection: the cause of one of its key-caused nodes
            pick = o64[:-1] + rng.integers(0, np.maximum(n_d, 1))
            tca = np.where(ci[pick] == 0, ck[pick], np.uint64(0)).astype(np.uint64)
        else:        # k distinct keys
            tca = (np.repeat(rng.integers(0, 1 << tb, D).astype(np.uint64), k) + j) & np.uint64((1 << tb) - 1)
        tci, tkd, tval = np.zeros(T, np.uint8), np.zeros(T, np.uint8), np.arange(T, dtype=np.uint64) + np.uint64(N)
        gt = [up(x) for x in (tid, tca, tci, tkd, tval)]
        cap = S + T
        io, iouts = map_outs(cap, N + T, D)
        mo_, mouts = map_outs(cap, N + T, D)
        cols = [z(N + T, torch.int64), z(N + T, torch.int64), z(N + T, torch.uint8), z(N + T, torch.uint8)]
        src = z(N + T, torch.int32)
        torch.cuda.synchronize()
        ins = lambda: abi_map_insert.insert_maps_device(
            w, off, [t.data_ptr() for t in g[:4]], S, segp, toff, [t.data_ptr() for t in gt], iouts, cap,
            value_ptr=g[4].data_ptr(), col_ptrs=[t.data_ptr() for t in cols])
        mrg = lambda: w.merge_maps_device(off, [t.data_ptr() for t in g], toff, [t.data_ptr() for t in gt], tb,
                                          lay.key_bits, src.data_ptr(), mouts, cap)
        (noff, Si), (moff, Sm) = ins(), mrg()  # warm-up, and the comparison
        torch.cuda.synchronize()
        assert np.array_equal(noff, moff) and Si == Sm and int(io["status"].max().item()) == 0
        dev = g[0].device

        def id_view(o, n_segs, ids_of):
            lens = torch.diff(o["seg_offsets"][:n_segs + 1])
            coll = torch.repeat_interleave(o["seg_coll"][:n_segs].long(), lens)
            perm = o["seg_perm"][:int(noff[-1]) + n_segs].long() & 0xFFFFFFFF
            root = perm == 0xFFFFFFFF
            ids = torch.where(root, torch.zeros_like(perm), ids_of(coll, torch.where(root, torch.zeros_like(perm), perm)))
            act = o["seg_active"][:n_segs]
            aid = torch.where(act < 0, act, ids_of(o["seg_coll"][:n_segs].long(), act.clamp(min=0)))
            return ids, aid, o["seg_key"][:n_segs]

        t_no, t_off, t_toff = (torch.from_numpy(x.astype(np.int64)).to(dev) for x in (noff, off, toff))

        def merged_ids(coll, s):
            m = src[:int(noff[-1])].long()[t_no[coll] + s]
            na = (t_off[coll + 1] - t_off[coll])
            return torch.where(m < na, g[0][(t_off[coll] + m).clamp(max=N - 1)],
                               gt[0][(t_toff[coll] + m - na).clamp(min=0, max=T - 1)])

        vi = id_view(io, Si, lambda coll, s: cols[0][t_no[coll] + s])
        vm = id_view(mo_, Sm, merged_ids)
        for x, y, what in zip(vi, vm, ("key weaves", "active ids", "seg_key")):
            assert torch.equal(x, y), f"insert and merge differ: {what}"
        t_i, t_m = [], []
        for _ in range(a.steps):
            t_i.append(timed(ins)[0])
            t_m.append(timed(mrg)[0])
        k_ms, k_by = kernel_ms(w, "map_insert", ins, 5)
        w.set_profile_only(None)
        w.reset_kernel_stats()
        w.set_profiling(True)
        mrg()
        w.set_profiling(False)
        mk = {n: hbm(ms / l, by / l) for n, (l, ms, by) in w.kernel_stats().items() if l}
        si, sm = spread(t_i), spread(t_m)
        emit({"what": f"one {k}-node tx a collection, config-4 maps, device memory", "colls": D, "nodes": N,
              "tx_nodes": T, "key_weaves": S, "new_key_weaves": Si - S, "steps": a.steps, "build": abi.build_id(),
              "insert_ms": si, "merge_ms": sm, "merge_over_insert": round(sm["median"] / si["median"], 2),
              "map_insert": hbm(k_ms, k_by), "merge_kernels": mk}, a.out)
        del gt, io, mo_, cols, src
    w.close()


if __name__ == "__main__":
    main()
