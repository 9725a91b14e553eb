"""Time cw_merge_lists on the GPU against the list reweave it contains.

    python scripts/time_list_merge.py [--docs 1000] [--steps 5] [--share 0.2]

Config 2's generator (gen.CONFIG2: documents of 50,001 nodes), --docs documents,
each split into two replicas that share --share of its nodes (the others go to
one side; at 0.2 na + nb = 60,002), everything resident in device memory.
Reported, in one JSON line, all from this one process on one build:

* list_union: the fused union kernel's time (cw_get_kernel_stats, timed alone
  with cw_ctx_set_profile_only) and its algorithmic bytes over that time,
  against 8.0 TB/s;
* merge_ms: the whole cw_merge_lists call (median of --steps);
* weave_ms: cw_weave_lists on the already-merged documents (the same nodes per
  document in id order), the two calls alternating: the floor, since the merge
  contains that reweave;
* overhead_ms: merge_ms - (list_union + weave_ms), the call's host work;
* general_ms: the whole call through the general route (list_merge_fused = 0),
  median of --steps, and general_union_ms, the sum of that route's union
  launches (merge_concat, the m_idsort passes, merge_count, merge_write) per
  call, from a profiled call; general_stage_ms = general_ms - weave_ms is the
  stage with its host round trips.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNION = ("merge_concat", "m_idsort", "merge_count", "merge_write")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.2)
    a = ap.parse_args()
    import torch

    from _common import emit, hbm, list_outs, timed, up, z
    from cause_amd import abi, gen

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    spec = gen.CONFIG2
    lay = spec.layout()
    off, idk, ck, kd = gen.generate(spec, 0, a.docs, nthreads=16)
    D, n = a.docs, spec.doc_size
    N = D * n
    # per document: `both` random nodes on both sides, the others alternately
    rng = np.random.default_rng(2)
    order = np.argsort(rng.random((D, n)), axis=1)
    both = int(round(a.share * n)) + (1 if a.share else 0)
    only_a = (n - both) // 2
    rows = np.arange(D)[:, None]
    in_a, in_b = np.zeros((D, n), bool), np.zeros((D, n), bool)
    in_a[rows, order[:, :both + only_a]] = True
    in_b[rows, order[:, :both]] = True
    in_b[rows, order[:, both + only_a:]] = True
    del order
    in_a, in_b = in_a.ravel(), in_b.ravel()
    na, nb = both + only_a, n - only_a
    oa = (np.arange(D + 1) * na).astype(np.uint64)
    ob = (np.arange(D + 1) * nb).astype(np.uint64)
    val = np.arange(N, dtype=np.uint64)
    ga = [up(x[in_a]) for x in (idk, ck, kd, val)]
    gb = [up(x[in_b]) for x in (idk, ck, kd, val)]
    NC = D * (na + nb)
    # the already-merged documents: every document's nodes in id order
    doc = torch.arange(D, dtype=torch.int64, device=dev).repeat_interleave(n)
    gi = up(idk)
    perm = torch.argsort((doc << lay.key_bits) | gi)
    del doc
    gm = [gi[perm]] + [up(x)[perm] for x in (ck, kd)]
    del gi, perm
    o, outs = list_outs(NC, (NC + 31) // 32 + 1, D)
    src = z(NC, torch.int32)
    pa, pb, pm = ([x.data_ptr() for x in g] for g in (ga, gb, gm))
    torch.cuda.synchronize()

    w = abi.Weaver(0)
    wg = abi.Weaver(0, options={"list_merge_fused": 0})
    merge = lambda ww=w: ww.merge_lists_device(oa, pa, ob, pb, lay, src.data_ptr(), outs)
    weave = lambda: w.weave_lists_device(off, pm[0], pm[1], pm[2], lay, outs)
    mo = merge()  # warm-up: scratch, tables
    perm_merge = o["weave_perm"][:N].clone()
    weave()
    assert np.array_equal(mo, off), "the union is not the document"
    assert int(o["status"].max().item()) == 0
    assert torch.equal(perm_merge, o["weave_perm"][:N]), "merge and weave of the union differ"
    merge(wg)
    assert torch.equal(perm_merge, o["weave_perm"][:N]), "the two routes differ"
    t_merge, t_weave, t_general = [], [], []
    for _ in range(a.steps):
        t_merge.append(timed(merge)[0])
        t_weave.append(timed(weave)[0])
        t_general.append(timed(lambda: merge(wg))[0])
    w.set_profile_only("list_union")
    w.reset_kernel_stats()
    w.set_profiling(True)
    for _ in range(a.steps):
        merge()
    w.set_profiling(False)
    launches, ms, by = w.kernel_stats()["list_union"]
    w.close()
    wg.reset_kernel_stats()
    wg.set_profiling(True)
    merge(wg)
    wg.set_profiling(False)
    g_union = {k: 0.0 for k in UNION}
    for name, (_, kms, _) in wg.kernel_stats().items():
        for k in UNION:
            if name.startswith(k):
                g_union[k] += kms
    wg.close()
    k_ms = ms / launches
    med = lambda t: float(np.median(t))
    line = {
        "what": "cw_merge_lists, config-2 documents split into two replicas, device memory",
        "docs": D, "nodes": N, "na": int(oa[-1]), "nb": int(ob[-1]), "share": a.share,
        "merged": int(mo[-1]), "steps": a.steps, "build": abi.build_id(),
        "list_union": hbm(k_ms, by / launches),
        "merge_ms": {"median": round(med(t_merge), 3), "all": [round(x, 3) for x in t_merge]},
        "weave_ms": {"median": round(med(t_weave), 3), "all": [round(x, 3) for x in t_weave]},
        "overhead_ms": round(med(t_merge) - k_ms - med(t_weave), 3),
        "general_ms": {"median": round(med(t_general), 3), "all": [round(x, 3) for x in t_general]},
        "general_union_ms": {"sum": round(sum(g_union.values()), 3),
                             **{k: round(v, 3) for k, v in g_union.items()}},
        "general_stage_ms": round(med(t_general) - med(t_weave), 3),
    }
    emit(line)


if __name__ == "__main__":
    main()
