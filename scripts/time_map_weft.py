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
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0


def quantile_cuts(idk, D, n, site_bits, q=0.5):
    """cut u64[D << site_bits]: per collection and site the largest id whose ts
    is <= the collection's q-quantile ts (0: the site has none)."""
    ids = idk.reshape(D, n)
    ts = ids >> np.uint64(site_bits)
    T = np.sort(ts, axis=1)[:, min(int(q * n), n - 1)]
    older = np.where(ts <= T[:, None], ids, np.uint64(0))
    site = ids & np.uint64((1 << site_bits) - 1)
    cut = np.zeros((D, 1 << site_bits), np.uint64)
    for r in range(1 << site_bits):
        cut[:, r] = np.where(site == np.uint64(r), older, np.uint64(0)).max(axis=1)
    return cut.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--colls", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from cause_amd import abi, gen

    dev = torch.device("cuda", 0)
    torch.cuda.init()
    spec = gen.CONFIG4
    lay, tb = spec.layout()
    off, idk, ck, ci, kd = gen.generate_maps(spec, 0, a.colls, nthreads=16)
    N, D, sb = len(idk), a.colls, lay.site_bits
    cut = quantile_cuts(idk, D, spec.nodes_per_coll, sb)
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    g = [up(x) for x in (idk, ck, ci, kd)]
    gcut = up(cut)
    gcut2 = up(quantile_cuts(idk, D, spec.nodes_per_coll, sb, 0.75))
    z = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    cap = N + (D << sb)
    o = {"seg_offsets": z(cap + 1, torch.int64), "seg_coll": z(cap, torch.int32),
         "seg_key": z(cap, torch.int64), "seg_active": z(cap, torch.int64),
         "seg_perm": z(2 * cap, torch.int32), "status": z(D, torch.int32)}
    src = z(cap, torch.int32)
    outs = {k: v.data_ptr() for k, v in o.items()}
    ptrs = [x.data_ptr() for x in g]
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def kernel_ms(w, name, fn):
        """Mean event time and algorithmic bytes of one kernel stat over --steps calls."""
        w.set_profile_only(name)
        w.reset_kernel_stats()
        w.set_profiling(True)
        for _ in range(a.steps):
            fn()
        w.set_profiling(False)
        launches, ms, by = w.kernel_stats()[name]
        return ms / launches, by / launches

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
    k_ms, k_by = kernel_ms(w, "map_weft", weft)
    p_ms, _ = kernel_ms(w, "m_pack", weft)
    q_ms, _ = kernel_ms(w2, "m_pack", weave)
    # other cuts every call: the kept layout changes, so the weave's pack table is rebuilt
    t_fresh = [timed(lambda: weft(w, (gcut2, gcut)[k % 2]))[0] for k in range(a.steps)]
    w.close()
    w2.close()
    with abi.Weaver(0, options={"map_weft_fused": 0}) as wg:
        for _ in range(2):
            kg, Sg = weft(wg)
        assert np.array_equal(kg, ko) and Sg == S
        t_general = [timed(lambda: weft(wg))[0] for _ in range(a.steps)]
        c_ms, _ = kernel_ms(wg, "mw_count", lambda: weft(wg))
        r_ms, _ = kernel_ms(wg, "mw_write", lambda: weft(wg))
    med = lambda t: {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                     "all": [round(x, 3) for x in t]}
    line = {
        "what": "cw_weft_maps, config-4 collections cut at their median ts, device memory",
        "colls": D, "nodes": N, "site_bits": sb, "kept": int(ko[-1]), "key_weaves": S,
        "key_weaves_uncut": S0, "steps": a.steps, "build": abi.build_id(),
        "map_weft": {"ms": round(k_ms, 4), "bytes_alg": k_by,
                     "tb_per_s": round(k_by / (k_ms / 1e3) / 1e12, 3),
                     "frac_of_hbm_peak": round(k_by / (k_ms / 1e3) / 1e12 / HBM_TBS, 3)},
        "weft_m_pack_ms": round(p_ms, 4),
        "weft_ms": med(t_weft),
        "weft_fresh_cuts_ms": med(t_fresh),
        "weave_m_pack_ms": round(q_ms, 4),
        "weave_ms": med(t_weave),
        "general_ms": med(t_general),
        "general_kernels_ms": {"mw_count": round(c_ms, 4), "mw_write": round(r_ms, 4)},
    }
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
