"""Time cw_weft_maps on the GPU against the plain map weave of the uncut input.

    python scripts/time_map_weft.py [--colls 1000000] [--steps 7] [--out FILE]

Config 4's generator (gen.CONFIG4), --colls collections, every collection cut
consistently at its median timestamp (each site's last id with ts <= the
median: causally closed, about half the nodes kept, no [id] node), everything
resident in device memory, the cut table included.  Reported, in one JSON line
(appended to --out when given):

* map_weft: the select kernel's event time (cw_get_kernel_stats, timed alone
  with cw_ctx_set_profile_only) and its algorithmic bytes over that time,
  against 8.0 TB/s;
* weft_m_pack_ms: the event time of the k_map_pack that follows it, on the kept
  collections;
* weft_ms: the whole cw_weft_maps call (host clock around a synchronised call),
  the same cuts every call, so the weave's pack table of the kept layout is the
  cached one; weft_fresh_cuts_ms: two cut tables (median and third-quartile ts)
  alternating, so every call builds that table anew;
* weave_ms / weave_m_pack_ms: cw_weave_maps of the uncut input in the same
  process (a context of its own), the two calls alternating -- the only way to
  weave these collections without cw_weft_maps; the difference is what the
  select stage adds over a plain weave (it also halves the nodes the weave sees);
* general_ms: the whole call through the general route (map_weft_fused = 0),
  with its mw_count / mw_write event times.
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
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import emit, hbm, kernel_ms, map_outs, med, quantile_cuts, timed, up, z
    from cause_amd import abi, gen

    torch.cuda.init()
    spec = gen.CONFIG4
    lay, tb = spec.layout()
    off, idk, ck, ci, kd = gen.generate_maps(spec, 0, a.colls, nthreads=16)
    N, D, sb = len(idk), a.colls, lay.site_bits
    # a map id is ts << site_bits | site rank
    cuts = lambda q: quantile_cuts(idk, D, spec.nodes_per_coll, sb, 0, sb, q)
    g = [up(x) for x in (idk, ck, ci, kd)]
    gcut, gcut2 = up(cuts(0.5)), up(cuts(0.75))
    cap = N + (D << sb)
    o, outs = map_outs(cap, cap, D)
    src = z(cap, torch.int32)
    ptrs = [x.data_ptr() for x in g]
    torch.cuda.synchronize()

    # a context each: both calls cache cw_weave_maps' pack table by layout, and
    # the kept layout is not the input's
    w, w2 = abi.Weaver(0), abi.Weaver(0)
    weft = lambda ww=w, c=gcut: ww.weft_maps_device(off, ptrs, tb, lay.key_bits, lay.site_shift, sb,
                                                    c.data_ptr(), src.data_ptr(), outs, cap)
    weave = lambda: w2.weave_maps_device(off, ptrs, tb, lay.key_bits, outs, cap)
    for _ in range(2):  # warm-up: scratch, pack tables, code objects
        (ko, S), S0 = weft(), weave()
    assert int(o["status"].max().item()) == 0
    t_weft, t_weave = [], []
    for _ in range(a.steps):
        t_weft.append(timed(weft)[0])
        t_weave.append(timed(weave)[0])
    k_ms, k_by = kernel_ms(w, "map_weft", weft, a.steps)
    p_ms, _ = kernel_ms(w, "m_pack", weft, a.steps)
    q_ms, _ = kernel_ms(w2, "m_pack", weave, a.steps)
    # other cuts every call: the kept layout changes, so the weave's pack table is rebuilt
    t_fresh = [timed(lambda: weft(w, (gcut2, gcut)[k % 2]))[0] for k in range(a.steps)]
    w.close()
    w2.close()
    with abi.Weaver(0, options={"map_weft_fused": 0}) as wg:
        for _ in range(2):
            kg, Sg = weft(wg)
        assert np.array_equal(kg, ko) and Sg == S
        t_general = [timed(lambda: weft(wg))[0] for _ in range(a.steps)]
        c_ms, _ = kernel_ms(wg, "mw_count", lambda: weft(wg), a.steps)
        r_ms, _ = kernel_ms(wg, "mw_write", lambda: weft(wg), a.steps)
    line = {
        "what": "cw_weft_maps, config-4 collections cut at their median ts, device memory",
        "colls": D, "nodes": N, "site_bits": sb, "kept": int(ko[-1]), "key_weaves": S,
        "key_weaves_uncut": S0, "steps": a.steps, "build": abi.build_id(),
        "map_weft": hbm(k_ms, k_by),
        "weft_m_pack_ms": round(p_ms, 4),
        "weft_ms": med(t_weft),
        "weft_fresh_cuts_ms": med(t_fresh),
        "weave_m_pack_ms": round(q_ms, 4),
        "weave_ms": med(t_weave),
        "general_ms": med(t_general),
        "general_kernels_ms": {"mw_count": round(c_ms, 4), "mw_write": round(r_ms, 4)},
    }
    emit(line, a.out)


if __name__ == "__main__":
    main()
