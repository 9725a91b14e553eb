"""Time the render stage (cw_render_lists / cw_render_maps) on the GPU.

    python scripts/render_bench.py --config 2 [--docs 10000] [--steps 3] [--out FILE]
    python scripts/render_bench.py --config 4 [--colls 1000000] [--steps 3] [--out FILE]

Config 2: gen.CONFIG2 (documents of 50,001 nodes, the bench's batch) woven in
device memory by cw_weave_lists_k32, then rendered with a 4-byte value column
(one code point a node).  Config 4: gen.CONFIG4's maps woven by cw_weave_maps,
then rendered with entry_key, entry_src and a 4-byte value column.  Reported,
in one JSON line (also written to --out):

* per kernel stat (render_lists or render_maps, render_offsets): the event
  time (cw_ctx_set_profiling, mean over --steps calls), the algorithmic bytes
  (DESIGN.md), GB/s on them and the fraction of the 8.0 TB/s HBM peak;
* variants: the main kernel's figures for the count-only call and for calls
  with some of the outputs, to tell the scan from the expansion and the gather;
* device_call_ms: the whole device-memory call, host clock, its one wait
  included; device_end_to_end_ms: that call plus the device-to-host copy of
  what it rendered (offsets, values; maps: keys too) -- the text of every
  document in host memory;
* host_path_ms: the same result the only way there was without this stage: a
  device-to-host copy of weave_perm and visible_bits (maps: seg_coll, seg_key,
  seg_active), then the compaction in numpy (copy_ms, numpy_ms).  Both results
  are compared before anything is reported.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=(2, 4), default=2)
    ap.add_argument("--docs", type=int, default=10_000)
    ap.add_argument("--colls", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import HBM_TBS, emit, list_outs, map_outs, med, timed, up
    from _common import z as empty
    from cause_amd import abi, gen

    torch.cuda.init()
    z = lambda n, dt: empty(max(n, 1), dt)
    host = lambda t, dt: t.cpu().numpy().view(dt)

    def kernels(w, fn, names):
        w.reset_kernel_stats()
        w.set_profiling(True)
        for _ in range(a.steps):
            fn()
        w.set_profiling(False)
        out = {}
        for name in names:
            launches, ms, by = w.kernel_stats()[name]
            ms, by = ms / launches, by / launches
            out[name] = {"ms": round(ms, 4), "bytes_alg": by, "gb_per_s": round(by / (ms / 1e3) / 1e9, 1),
                         "frac_of_hbm_peak": round(by / (ms / 1e3) / 1e12 / HBM_TBS, 3)}
        w.reset_kernel_stats()
        return out

    note = lambda what: print(f"[render_bench] {what}", file=sys.stderr, flush=True)
    w = abi.Weaver(0)
    note("generating and weaving the input")
    line = {"steps": a.steps, "build": abi.build_id(), "value_size": 4}
    if a.config == 2:
        spec = gen.CONFIG2
        lay = spec.layout()
        off, idk, ck, kd = gen.generate(spec, 0, a.docs, nthreads=16, k32=True)
        N, D = len(idk), a.docs
        val = (np.arange(N, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(11)  # "code points"
        g = [up(x) for x in (idk, ck, kd)]
        del idk, ck, kd
        gval = up(val)
        outs, ptrs = list_outs(N, (N + 31) // 32, D)
        perm, bits = outs["weave_perm"], outs["visible_bits"]
        torch.cuda.synchronize()
        w.weave_lists_k32_device(off, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), lay, ptrs)
        torch.cuda.synchronize()
        assert int(outs["status"].max().item()) == 0
        del g
        osrc, oval = z(N, torch.int32), z(N, torch.int32)
        call = lambda: w.render_lists_device(off, perm.data_ptr(), bits.data_ptr(), osrc.data_ptr(),
                                             gval.data_ptr(), 4, oval.data_ptr())

        def device_path():
            ro = call()
            return ro, host(oval[:int(ro[-1])], np.uint32)

        def host_path():
            t0 = time.perf_counter()
            p, b = host(perm, np.uint32), host(bits, np.uint32)
            t1 = time.perf_counter()
            on = np.unpackbits(b.view(np.uint8), bitorder="little")[:N].view(bool)
            n = spec.doc_size
            ro = np.zeros(D + 1, np.uint64)
            ro[1:] = np.cumsum(on.reshape(D, n).sum(axis=1))
            idx = np.flatnonzero(on)
            v = val[idx - idx % n + p[idx]]
            return ro, v, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        line.update({"what": "render of a config-2 batch: causal-list->edn of every document",
                     "docs": D, "nodes": N, "weave_perm": "u32"})
        names = ("render_lists", "render_offsets")
        variants = {"count_only": lambda: w.render_lists_device(off, perm.data_ptr(), bits.data_ptr()),
                    "src_only": lambda: w.render_lists_device(off, perm.data_ptr(), bits.data_ptr(),
                                                              osrc.data_ptr()),
                    "value_only": lambda: w.render_lists_device(off, perm.data_ptr(), bits.data_ptr(), None,
                                                                gval.data_ptr(), 4, oval.data_ptr())}
    else:
        spec = gen.CONFIG4
        lay, tb = spec.layout()
        off, idk, ck, ci, kd = gen.generate_maps(spec, 0, a.colls, nthreads=16)
        N, D = len(idk), a.colls
        val = (np.arange(N, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(11)
        g = [up(x) for x in (idk, ck, ci, kd)]
        del idk, ck, ci, kd
        gval = up(val)
        o, ptrs = map_outs(N, N, D)
        torch.cuda.synchronize()
        S = w.weave_maps_device(off, [x.data_ptr() for x in g], tb, lay.key_bits, ptrs, N)
        torch.cuda.synchronize()
        del g
        okey, osrc, oval = z(S, torch.int64), z(S, torch.int32), z(S, torch.int32)
        call = lambda: w.render_maps_device(D, S, o["seg_coll"].data_ptr(), o["seg_key"].data_ptr(),
                                            o["seg_active"].data_ptr(), okey.data_ptr(), osrc.data_ptr(), off,
                                            gval.data_ptr(), 4, oval.data_ptr())

        def device_path():
            eo = call()
            R = int(eo[-1])
            return eo, host(oval[:R], np.uint32), host(okey[:R], np.uint64)

        def host_path():
            t0 = time.perf_counter()
            coll = host(o["seg_coll"][:S], np.uint32)
            key = host(o["seg_key"][:S], np.uint64)
            act = host(o["seg_active"][:S], np.int64)
            t1 = time.perf_counter()
            on = act >= 0
            eo = np.zeros(D + 1, np.uint64)
            eo[1:] = np.cumsum(np.bincount(coll[on], minlength=D))
            v = val[off[coll[on]].astype(np.int64) + act[on]]
            return eo, v, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, key[on]

        line.update({"what": "render of config 4's maps: causal-map->edn of every collection",
                     "colls": D, "nodes": N, "key_weaves": S})
        names = ("render_maps", "render_offsets")
        variants = {"count_only": lambda: w.render_maps_device(D, S, o["seg_coll"].data_ptr(),
                                                               o["seg_key"].data_ptr(),
                                                               o["seg_active"].data_ptr()),
                    "key_and_src": lambda: w.render_maps_device(D, S, o["seg_coll"].data_ptr(),
                                                                o["seg_key"].data_ptr(),
                                                                o["seg_active"].data_ptr(), okey.data_ptr(),
                                                                osrc.data_ptr())}

    note("rendering")
    call()  # warm-up: scratch, the layout upload, code objects
    dres = device_path()
    note("the host path")
    hres = host_path()
    assert np.array_equal(dres[0], hres[0]) and np.array_equal(dres[1], hres[1]), "device and host paths differ"
    if a.config == 4:
        assert np.array_equal(dres[2], hres[4])
    note("timing")
    line["rendered"] = int(dres[0][-1])
    line["device_call_ms"] = med([timed(call)[0] for _ in range(a.steps)])
    line["device_end_to_end_ms"] = med([timed(device_path)[0] for _ in range(a.steps)])
    hp = [(timed(host_path)) for _ in range(a.steps)]
    line["host_path_ms"] = med([t for t, _ in hp])
    line["host_path_copy_ms"] = med([r[2] for _, r in hp])
    line["host_path_numpy_ms"] = med([r[3] for _, r in hp])
    line["kernels"] = kernels(w, call, names)
    # the same kernel with fewer outputs: what the scan alone and each output cost
    line["variants"] = {k: kernels(w, fn, names[:1])[names[0]] for k, fn in variants.items()}
    w.close()
    emit(line, a.out, mode="w")


if __name__ == "__main__":
    main()
