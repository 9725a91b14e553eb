"""Time cw_insert_lists on the GPU against the only other route to its arrays.

    python scripts/insert_bench.py [--docs 10000] [--steps 20] [--out FILE]

Config 2's shape (gen.CONFIG2: --docs documents of 50,001 nodes), woven once by
cw_weave_lists, everything resident in device memory.  Two workloads: one
1-node tx per document (a keystroke) and one 64-node tx per document (a pasted
run), under a random node of the document, Lamport ids.  Config 2's keys have
no tx bits (key = ts | site), and wider keys would push cw_merge_lists off its
dense-id union kernel, so the 64 nodes of a run take 64 consecutive timestamps
of one site: the same arrays, the same work.

The yardstick is cw_merge_lists (device memory) on the same documents with the
tx as side b: the union and the full reweave, timed in the same process, the
two calls alternating.  Before anything is timed the two results are compared:
the ids in weave order, the rendered bits and counts, max_ts.

Reported, in one JSON line per workload (also appended to --out): the median,
min, max and interquartile spread of --steps timed calls of each (host clock,
the call's wait included), their ratio, and per kernel of cw_insert_lists the
event time (cw_ctx_set_profiling), the algorithmic bytes, GB/s
on them and the fraction of the 8.0 TB/s HBM peak; `merge_kernels`: the event
times of one cw_merge_lists call, which name the route it took.  `columns`:
the insert call that also writes the new documents' id / cause / kind / value
columns.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_insert_mark", "k_insert_find", "k_insert_plan", "k_insert_splice")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import HBM_TBS, emit, list_outs, timed, up, z
    from cause_amd import abi, abi_insert, gen
    from cause_amd.pack import KeyLayout

    note = lambda what: print(f"[insert_bench] {what}", file=sys.stderr, flush=True)
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    spec = gen.CONFIG2
    old = spec.layout()
    lay = KeyLayout(old.ts_bits + 1, old.site_bits, 0)  # (room for the new timestamps)
    note("generating and weaving the documents")
    off, idk, ck, kd = gen.generate(spec, 0, a.docs, nthreads=16)
    D, n = a.docs, spec.doc_size
    N = D * n
    gi, gc, gk = up(idk), up(ck), up(kd)
    del idk, ck, kd
    gv = torch.arange(N, dtype=torch.int64, device=dev)
    w = abi.Weaver(0)
    o0, p0 = list_outs(N, (N + 31) // 32, D, yarns=True)
    torch.cuda.synchronize()
    w.weave_lists_device(off, gi.data_ptr(), gc.data_ptr(), gk.data_ptr(), lay, p0)
    torch.cuda.synchronize()
    assert int(o0["status"].max().item()) == 0
    ids2 = gi.view(D, n)
    top_ts = (ids2.max(dim=1).values >> lay.ts_shift) + 1
    g = torch.Generator(device="cpu").manual_seed(7)
    pick = torch.randint(0, n, (D,), generator=g).to(dev)
    cause0 = ids2[torch.arange(D, device=dev), pick]

    def kernels(fn, names=KERNELS, steps=None):
        w.reset_kernel_stats()
        w.set_profiling(True)
        for _ in range(steps or a.steps):
            fn()
        w.set_profiling(False)
        out = {}
        for name in names or sorted(w.kernel_stats()):
            launches, ms, by = w.kernel_stats()[name]
            ms, by = ms / launches, by / launches
            out[name] = {"ms": round(ms, 4), "bytes_alg": by, "gb_per_s": round(by / (ms / 1e3) / 1e9, 1),
                         "frac_of_hbm_peak": round(by / (ms / 1e3) / 1e12 / HBM_TBS, 3)}
        w.reset_kernel_stats()
        return out

    def spread(t):
        q = np.percentile(t, [25, 50, 75])
        return {"median": round(float(q[1]), 3), "min": round(float(np.min(t)), 3),
                "max": round(float(np.max(t)), 3), "iqr": round(float(q[2] - q[0]), 3)}

    for k in (1, 64):
        note(f"one tx of {k} node(s) per document")
        T, NT = D * k, N + D * k
        m = torch.arange(k, dtype=torch.int64, device=dev)
        tid = ((top_ts[:, None] + m[None, :]) << lay.ts_shift) | (1 << lay.site_shift)  # site rank 1
        tca = torch.cat([cause0[:, None], tid[:, :-1]], dim=1).contiguous().view(-1)
        tid = tid.contiguous().view(-1)
        tkd = torch.zeros(T, dtype=torch.uint8, device=dev)
        tv = torch.arange(N, N + T, dtype=torch.int64, device=dev)
        toff = (np.arange(D + 1) * k).astype(np.uint64)
        o, ptrs = list_outs(NT, (NT + 31) // 32 + 1, D, yarns=True)
        pos = z(D, torch.int32)
        cols = [z(NT, torch.int64), z(NT, torch.int64), z(NT, torch.uint8), z(NT, torch.int64)]
        src = z(NT, torch.int32)
        om, pm = list_outs(NT, (NT + 31) // 32 + 1, D, yarns=True)
        torch.cuda.synchronize()

        def insert(columns=False):
            return abi_insert.insert_lists_device(
                w, off, (gi.data_ptr(), gc.data_ptr(), gk.data_ptr()), o0["weave_perm"].data_ptr(),
                o0["visible_bits"].data_ptr(), toff, (tid.data_ptr(), tca.data_ptr(), tkd.data_ptr(), tv.data_ptr()),
                lay, ptrs, pos_ptr=pos.data_ptr(), yarn_ptr=o0["yarn_perm"].data_ptr(), value_ptr=gv.data_ptr(),
                col_ptrs=[c.data_ptr() for c in cols] if columns else None)

        merge = lambda: w.merge_lists_device(
            off, (gi.data_ptr(), gc.data_ptr(), gk.data_ptr(), gv.data_ptr()), toff,
            (tid.data_ptr(), tca.data_ptr(), tkd.data_ptr(), tv.data_ptr()), lay, src.data_ptr(), pm)
        # warm-up (scratch, layouts, code objects) and the comparison
        no = insert(True)
        mo = merge()
        torch.cuda.synchronize()
        assert np.array_equal(no, mo) and int(no[-1]) == NT
        assert int(o["status"].max().item()) == 0 and int(om["status"].max().item()) == 0
        base = (torch.arange(D, device=dev, dtype=torch.int64) * (n + k)).repeat_interleave(n + k)
        ins_ids = cols[0][base + o["weave_perm"][:NT].to(torch.int64)]
        s = src[:NT].to(torch.int64)
        doc = base // (n + k)
        from_a = s < n
        merged_ids = torch.where(from_a, gi[(doc * n + s).clamp(max=N - 1)], tid[(doc * k + s - n).clamp(0, T - 1)])
        mrg_ids = merged_ids[base + om["weave_perm"][:NT].to(torch.int64)]
        assert torch.equal(ins_ids, mrg_ids), "insert and merge weave differently"
        W = (NT + 31) // 32
        assert torch.equal(o["visible_bits"][:W], om["visible_bits"][:W]), "rendered bits differ"
        assert torch.equal(o["visible_count"], om["visible_count"]) and torch.equal(o["max_ts"], om["max_ts"])
        del base, ins_ids, s, doc, from_a, merged_ids, mrg_ids
        t_ins, t_mrg, t_col = [], [], []
        for _ in range(a.steps):
            t_ins.append(timed(insert)[0])
            t_mrg.append(timed(merge)[0])
            t_col.append(timed(lambda: insert(True))[0])
        line = {"what": f"cw_insert_lists, one {k}-node tx per config-2 document, device memory, "
                        "against cw_merge_lists with the tx as side b",
                "docs": D, "nodes": N, "tx_nodes": T, "steps": a.steps, "build": abi.build_id(),
                "insert_ms": spread(t_ins), "merge_ms": spread(t_mrg), "insert_columns_ms": spread(t_col),
                "merge_over_insert": round(float(np.median(t_mrg) / np.median(t_ins)), 2),
                "kernels": kernels(insert), "kernels_columns": kernels(lambda: insert(True)),
                "merge_kernels": {name: v["ms"] for name, v in kernels(merge, None, 1).items()}}
        emit(line, a.out)
        del o, om, cols, src, pos, tid, tca, tkd, tv
    w.close()


if __name__ == "__main__":
    main()
