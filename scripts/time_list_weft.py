"""Time the list weft on the GPU: the host call, the device call and its routes.

    python scripts/time_list_weft.py [--docs 1000] [--steps 5] [--out FILE]

Config 2's generator (gen.CONFIG2: documents of 50,001 nodes), --docs
documents, every document cut consistently at its median timestamp (each
site's last id with ts <= the median: causally closed, about half the nodes
kept, no [id] node).  Reported, in one JSON line (appended to --out when
given):

* host_ms: the whole cw_weft_lists call in host memory (host clock), uploads
  and copies out included.  This is the one figure a build from before
  cw_weft_lists_dev can give (CW_LIB names such a build): its select kernels
  were launched without profiling records;
* list_weft: the fused select kernel's event time (cw_get_kernel_stats, timed
  alone with cw_ctx_set_profile_only) and its algorithmic bytes over that time,
  against 8.0 TB/s;
* dev_ms: the whole cw_weft_lists_dev call, everything resident in device
  memory, the same cuts every call; dev_fresh_cuts_ms: two cut tables (median
  and third-quartile ts) alternating;
* weave_ms: cw_weave_lists of the uncut input in device memory in the same
  process (a context of its own), alternating with the weft: what the select
  stage adds over a plain weave (it also halves the nodes the weave sees);
* general_ms: the whole device call through the general route
  (list_weft_fused = 0) with its weft_count / weft_write event times -- the
  unchanged k_weft_select, so these are also the kernel times of a build from
  before the fused route.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import emit, hbm, kernel_ms, list_outs, med, quantile_cuts, timed, up, z
    from cause_amd import abi, gen

    torch.cuda.init()
    spec = gen.CONFIG2
    lay = spec.layout()
    off, idk, ck, kd = gen.generate(spec, 0, a.docs, nthreads=16)
    N, D, sb = len(idk), a.docs, lay.site_bits
    cuts = lambda q: quantile_cuts(idk, D, spec.doc_size, lay.ts_shift, lay.site_shift, sb, q)
    cut = cuts(0.5)
    has_dev = hasattr(abi.lib(), "cw_weft_lists_dev")

    line = {"what": "list weft, config-2 documents cut at their median ts",
            "docs": D, "nodes": N, "site_bits": sb, "steps": a.steps, "build": abi.build_id()}

    with abi.Weaver(0) as wh:
        host = lambda: wh.weft_lists(off, idk, ck, kd, lay, cut)
        res = host()  # warm-up: scratch, tables, code objects
        line["kept"] = int(res.offsets[-1])
        line["status_or"] = int(np.bitwise_or.reduce(res.weave.status))
        line["host_ms"] = med([timed(host)[0] for _ in range(a.steps)])
        if has_dev:
            wh.set_profile_only("list_weft")
            wh.reset_kernel_stats()
            wh.set_profiling(True)
            host()
            wh.set_profiling(False)
            line["host_list_weft_ms"] = round(wh.kernel_stats()["list_weft"][1], 4)
    if has_dev:
        g = [up(x) for x in (idk, ck, kd)]
        gcut, gcut2 = up(cut), up(cuts(0.75))
        cap = N + (D << sb)
        o, outs = list_outs(cap, (cap + 31) // 32, D, yarns=True)
        src = z(cap, torch.int32)
        ptrs = [x.data_ptr() for x in g]
        torch.cuda.synchronize()

        # a context each: both calls cache the document tables by layout, and
        # the kept layout is not the input's
        w, w2 = abi.Weaver(0), abi.Weaver(0)
        weft = lambda ww=w, c=gcut: ww.weft_lists_device(off, ptrs, lay, c.data_ptr(), src.data_ptr(), outs)
        weave = lambda: w2.weave_lists_device(off, ptrs[0], ptrs[1], ptrs[2], lay, outs)
        for _ in range(2):
            ko = weft()
            weave()
        assert np.array_equal(ko, res.offsets)
        t_weft, t_weave = [], []
        for _ in range(a.steps):
            t_weft.append(timed(weft)[0])
            t_weave.append(timed(weave)[0])
        k_ms, k_by = kernel_ms(w, "list_weft", weft, a.steps)
        t_fresh = [timed(lambda: weft(w, (gcut2, gcut)[k % 2]))[0] for k in range(a.steps)]
        w.close()
        w2.close()
        with abi.Weaver(0, options={"list_weft_fused": 0}) as wg:
            for _ in range(2):
                kg = weft(wg)
            assert np.array_equal(kg, ko)
            t_general = [timed(lambda: weft(wg))[0] for _ in range(a.steps)]
            c_ms, _ = kernel_ms(wg, "weft_count", lambda: weft(wg), a.steps)
            r_ms, _ = kernel_ms(wg, "weft_write", lambda: weft(wg), a.steps)
        line.update({
            "list_weft": hbm(k_ms, k_by),
            "dev_ms": med(t_weft),
            "dev_fresh_cuts_ms": med(t_fresh),
            "weave_ms": med(t_weave),
            "general_ms": med(t_general),
            "general_kernels_ms": {"weft_count": round(c_ms, 4), "weft_write": round(r_ms, 4),
                                   "sum": round(c_ms + r_ms, 4)},
        })
    emit(line, a.out)


if __name__ == "__main__":
    main()
