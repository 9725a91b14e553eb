"""Time cw_merge_maps on the GPU against the map reweave it contains.

    python scripts/time_map_merge.py [--colls 1000000] [--steps 5] [--share 0.2]

Config 4's generator (gen.CONFIG4), --colls collections, each split into two
replicas that share --share of its nodes (the rest go to one side at random),
everything resident in device memory.  Reported, in one JSON line:

* map_union: the union kernel's time (cw_get_kernel_stats, timed alone with
  cw_ctx_set_profile_only) and its algorithmic bytes over that time, against
  8.0 TB/s;
* merge_ms: the whole cw_merge_maps call;
* weave_ms: cw_weave_maps on the already-merged collections (the same nodes
  per collection in id order), in the same process, the two calls alternating:
  the floor, since the merge contains that reweave;
* general_ms: the whole call through the general route (map_merge_fused = 0),
  once, for the record.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--colls", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.2)
    a = ap.parse_args()
    import torch

    from _common import emit, hbm, map_outs, timed, up, z
    from cause_amd import abi, gen

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    spec = gen.CONFIG4
    lay, tb = spec.layout()
    off, idk, ck, ci, kd = gen.generate_maps(spec, 0, a.colls, nthreads=16)
    N, D = len(idk), a.colls
    rng = np.random.default_rng(4)
    r = rng.random(N)
    in_a, in_b = r < a.share + (1 - a.share) / 2, (r < a.share) | (r >= a.share + (1 - a.share) / 2)
    o64 = off.astype(np.int64)
    offs = lambda m: np.concatenate([[0], np.cumsum(m)])[o64].astype(np.uint64)
    oa, ob = offs(in_a), offs(in_b)
    val = np.arange(N, dtype=np.uint64)
    ga = [up(x[in_a]) for x in (idk, ck, ci, kd, val)]
    gb = [up(x[in_b]) for x in (idk, ck, ci, kd, val)]
    Na, Nb = int(oa[-1]), int(ob[-1])
    NC = Na + Nb
    # the already-merged collections: every collection's nodes in id order
    coll = torch.from_numpy(np.repeat(np.arange(D, dtype=np.int64), np.diff(o64))).to(dev)
    gi = up(idk)
    order = torch.argsort((coll << lay.key_bits) | gi)
    del coll
    gm = [gi[order]] + [up(x)[order] for x in (ck, ci, kd)]
    del gi, order
    cap = NC
    o, outs = map_outs(cap, NC, D)
    src = z(NC, torch.int32)
    pa, pb, pm = ([x.data_ptr() for x in g] for g in (ga, gb, gm))
    torch.cuda.synchronize()

    w = abi.Weaver(0)
    merge = lambda ww=w: ww.merge_maps_device(oa, pa, ob, pb, tb, lay.key_bits, src.data_ptr(), outs, cap)
    weave = lambda: w.weave_maps_device(off, pm, tb, lay.key_bits, outs, cap)
    (mo, S), S2 = merge(), weave()  # warm-up: scratch, pack tables
    assert np.array_equal(mo, off) and S == S2, "the union is not the collection"
    assert int(o["status"].max().item()) == 0
    t_merge, t_weave = [], []
    for _ in range(a.steps):
        t_merge.append(timed(merge)[0])
        t_weave.append(timed(weave)[0])
    w.set_profile_only("map_union")
    w.reset_kernel_stats()
    w.set_profiling(True)
    for _ in range(a.steps):
        merge()
    w.set_profiling(False)
    launches, ms, by = w.kernel_stats()["map_union"]
    w.close()
    with abi.Weaver(0, options={"map_merge_fused": 0}) as wg:
        merge(wg)
        t_general = timed(lambda: merge(wg))[0]
    k_ms = ms / launches
    line = {
        "what": "cw_merge_maps, config-4 collections split into two replicas, device memory",
        "colls": D, "nodes": N, "na": Na, "nb": Nb, "share": a.share, "merged": int(mo[-1]),
        "key_weaves": S, "steps": a.steps, "build": abi.build_id(),
        "map_union": hbm(k_ms, by / launches),
        "merge_ms": {"median": round(float(np.median(t_merge)), 3), "all": [round(x, 3) for x in t_merge]},
        "weave_ms": {"median": round(float(np.median(t_weave)), 3), "all": [round(x, 3) for x in t_weave]},
        "general_ms": round(t_general, 3),
    }
    emit(line)


if __name__ == "__main__":
    main()
