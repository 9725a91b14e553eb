"""Time cw_version and cw_delta on the GPU, device memory.

    python scripts/sync_bench.py [--docs2 10000] [--docs4 1000000] [--steps 20] [--out profiles/sync_bench.txt]

Two shapes: config 2's (gen.CONFIG2: --docs2 lists of 50,001 nodes, the
workgroup route) and config 4's (gen.CONFIG4: --docs4 maps of 100 nodes, the
wave route).  Three cases a shape, one JSON line each (also appended to --out):
  version        cw_version with all three outputs;
  delta_behind   cw_delta against a peer ten nodes behind in every document
                 (its heads: cw_version of the batch without each document's
                 ten newest ids), every column gathered, with ahead;
  delta_nothing  cw_delta against a peer that has nothing (have all zero).
Reported per case: the median, min, max and interquartile spread of --steps
timed calls (host clock, the call's wait included); per kernel stat the event
time (cw_ctx_set_profiling), the algorithmic bytes and GB/s on them; and,
measured in the same run, a device-to-device copy that moves as many bytes
(half read, half written) with its GB/s.  For config 2's shape a fourth line:
cw_weave_lists with and without yarn_perm + max_ts, the only way to the heads
before cw_version.

Before anything is timed the first calls are compared with tests/sync_model.py
on the first documents of the batch, and the delta sizes with their counts.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEHIND = 10


def spread(t):
    q = np.percentile(t, [25, 50, 75])
    return {"median": round(float(q[1]), 3), "min": round(float(np.min(t)), 3), "max": round(float(np.max(t)), 3),
            "iqr": round(float(q[2] - q[0]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs2", type=int, default=10_000)
    ap.add_argument("--docs4", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import emit, list_outs, timed, up, z
    from cause_amd import abi, abi_sync, gen
    from tests import sync_model as SM

    note = lambda what: print(f"[sync_bench] {what}", file=sys.stderr, flush=True)
    torch.cuda.init()
    w = abi.Weaver(0)

    def measure(call):
        """-> (times of the timed calls, {stat: ms, bytes, GB/s} a call)"""
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
        return times, kernels

    def copy_of(nbytes):
        half = max(int(nbytes) // 2, 1)
        src_, dst_ = z(half, torch.uint8), z(half, torch.uint8)
        dst_.copy_(src_)
        t = [timed(lambda: dst_.copy_(src_))[0] for _ in range(a.steps)]
        del src_, dst_
        return {"bytes_moved": 2 * half, "ms": spread(t), "gb_per_s": round(2 * half / (np.median(t) / 1e3) / 1e9, 1)}

    for shape, D in (("config2", a.docs2), ("config4", a.docs4)):
        if D <= 0:
            continue
        note(f"{shape}: generating {D} documents")
        if shape == "config2":
            spec = gen.CONFIG2
            lay = spec.layout()
            off, idk, ck, kd = gen.generate(spec, 0, D, nthreads=16)
            cols, ci = [idk, ck, kd], None
            n = spec.doc_size
        else:
            spec = gen.CONFIG4
            lay, _ = spec.layout()
            off, idk, ck, ci, kd = gen.generate_maps(spec, 0, D, nthreads=16)
            cols = [idk, ck, kd, ci]
            n = spec.nodes_per_coll
        N, S = len(idk), 1 << lay.site_bits
        words = D << lay.site_bits
        g = [up(x) for x in cols]
        ptrs = [t.data_ptr() for t in g]
        vo = {"ver": z(words, torch.int64), "yarn_len": z(words, torch.int32), "max_ts": z(D, torch.int64)}
        version = lambda: abi_sync.version_device(w, off, ptrs[0], lay, {k: v.data_ptr() for k, v in vo.items()})
        # the peer ten nodes behind: the heads of the batch without each document's ten newest ids
        ids2 = g[0].view(D, n)
        thr = torch.topk(ids2, BEHIND, dim=1).values[:, -1:]
        older = torch.where(ids2 >= thr, torch.zeros_like(ids2), ids2).reshape(-1).contiguous()
        have_behind = z(words, torch.int64)
        abi_sync.version_device(w, off, older.data_ptr(), lay, {"ver": have_behind.data_ptr()})
        torch.cuda.synchronize()
        del older, thr
        have_nothing = torch.zeros(words, dtype=torch.int64, device=g[0].device)
        do_ = {"delta_src": z(N, torch.int32), "delta_id": z(N, torch.int64), "delta_cause": z(N, torch.int64),
               "delta_kind": z(N, torch.uint8), "ahead": z(D, torch.int32)}
        if ci is not None:
            do_["delta_cause_is_id"] = z(N, torch.uint8)
        dptrs = {k: v.data_ptr() for k, v in do_.items()}
        delta = lambda have: abi_sync.delta_device(w, off, ptrs, lay, have.data_ptr(), dptrs)

        # the first calls against the model (its first documents) and the counts
        note(f"{shape}: checking the first calls")
        K = min(D, max(2, 200_000 // n))
        version()
        torch.cuda.synchronize()
        want = SM.version(off[:K + 1], idk[:K * n], lay)
        for k, x in zip(("ver", "yarn_len", "max_ts"), want):
            got = vo[k].cpu().numpy().view(x.dtype)[:len(x)]
            assert np.array_equal(got, x), f"{shape}: {k} differs from the model"
        assert int(vo["yarn_len"].sum()) == N
        hb = have_behind.cpu().numpy().view(np.uint64)
        for name, have, count in (("behind", have_behind, BEHIND * D), ("nothing", have_nothing, int((idk != 0).sum()))):
            po = delta(have)
            torch.cuda.synchronize()
            assert int(po[-1]) == count, (shape, name, int(po[-1]), count)
            hv = hb[:K * S] if name == "behind" else np.zeros(K * S, np.uint64)
            m = SM.delta(off[:K + 1], idk[:K * n], lay, hv, cause=ck[:K * n], kind=kd[:K * n],
                         cause_is_id=None if ci is None else ci[:K * n])
            P = int(m[0][-1])
            assert np.array_equal(po[:K + 1], m[0]), f"{shape}: delta offsets ({name}) differ from the model"
            for k, x in zip(("delta_src", "delta_id", "delta_cause", "delta_kind", "delta_cause_is_id"), m[1:6]):
                if x is not None:
                    assert np.array_equal(do_[k][:P].cpu().numpy().view(x.dtype), x), f"{shape}: {k} ({name})"
            assert np.array_equal(do_["ahead"][:K].cpu().numpy().view(np.uint32), m[6])

        base = {"shape": shape, "docs": D, "nodes": N, "site_bits": lay.site_bits, "steps": a.steps,
                "build": abi.build_id()}
        for case, call, extra in (("version", version, {}),
                                  ("delta_behind", lambda: delta(have_behind), {"delta_nodes": BEHIND * D}),
                                  ("delta_nothing", lambda: delta(have_nothing),
                                   {"delta_nodes": int((idk != 0).sum())})):
            note(f"{shape}: {case}")
            times, kernels = measure(call)
            main_stat = max(kernels, key=lambda k: kernels[k]["bytes_alg"])
            emit({"what": f"{'cw_version' if case == 'version' else 'cw_delta'}, {case}: {D} x {n} nodes ({shape}), "
                          "device memory", **base, **extra, "call_ms": spread(times), "kernels": kernels,
                  "bytes_a_node": round(kernels[main_stat]["bytes_alg"] / N, 3),
                  "d2d_copy_of_as_many_bytes": copy_of(kernels[main_stat]["bytes_alg"])}, a.out)
        del do_, vo, have_behind, have_nothing

        if shape == "config2":
            # the heads before cw_version: the whole list weave with yarn_perm, the end of each yarn read by the host
            note("config2: cw_weave_lists with and without yarn_perm + max_ts")
            o, optrs = list_outs(N, (N + 31) // 32 + 1, D, yarns=True)
            bare = {k: v for k, v in optrs.items() if k not in ("yarn_perm", "max_ts")}
            weave = lambda p: w.weave_lists_device(off, ptrs[0], ptrs[1], ptrs[2], lay, p)
            weave(optrs), weave(bare)
            t_with = [timed(lambda: weave(optrs))[0] for _ in range(max(a.steps // 4, 3))]
            t_bare = [timed(lambda: weave(bare))[0] for _ in range(max(a.steps // 4, 3))]
            emit({"what": f"cw_weave_lists, {D} x {n} nodes (config2), device memory: with and without yarn_perm + "
                          "max_ts", **base, "with_ms": spread(t_with), "without_ms": spread(t_bare),
                  "yarns_and_max_ts_ms": round(float(np.median(t_with) - np.median(t_bare)), 3)}, a.out)
            del o
        del g
        torch.cuda.empty_cache()
    w.close()


if __name__ == "__main__":
    main()
