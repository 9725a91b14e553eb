"""What the timing scripts share (time_list_merge, time_map_merge,
time_list_weft, time_map_weft, render_bench): the host clock around a
synchronised call, one kernel stat's event time, the summary of a list of
times, uploads, output tensors with their pointer dicts, and the JSON line."""
import json
import os
import time

import numpy as np
import torch

HBM_TBS = 8.0
LIST_OUT = {"weave_perm": torch.int32, "visible_bits": torch.int32, "visible_count": torch.int32,
            "max_ts": torch.int64, "status": torch.int32, "yarn_perm": torch.int32}


def timed(fn):
    """(milliseconds on the host clock, fn()) with the device idle before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms(w, name, fn, steps):
    """Mean event time and algorithmic bytes of one kernel stat over `steps` calls."""
    w.set_profile_only(name)
    w.reset_kernel_stats()
    w.set_profiling(True)
    for _ in range(steps):
        fn()
    w.set_profiling(False)
    launches, ms, by = w.kernel_stats()[name]
    return ms / launches, by / launches


def med(t):
    return {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
            "all": [round(x, 3) for x in t]}


def hbm(ms, by):
    """A kernel's time, algorithmic bytes and rate against the HBM peak."""
    return {"ms": round(ms, 4), "bytes_alg": by, "tb_per_s": round(by / (ms / 1e3) / 1e12, 3),
            "frac_of_hbm_peak": round(by / (ms / 1e3) / 1e12 / HBM_TBS, 3)}


def up(x, dev=None):
    """A numpy array on the device (unsigned words as the signed torch dtype)."""
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(x.dtype)
    return torch.from_numpy(x.view(signed) if signed else x).to(dev or torch.device("cuda", 0))


def z(n, dt, dev=None):
    return torch.empty(n, dtype=dt, device=dev or torch.device("cuda", 0))


def list_outs(nodes, words, D, yarns=False):
    """The device tensors of a list result and their pointer dict."""
    sizes = {"weave_perm": nodes, "visible_bits": words, "yarn_perm": nodes}
    o = {k: z(sizes.get(k, D), dt) for k, dt in LIST_OUT.items() if yarns or k != "yarn_perm"}
    return o, {k: v.data_ptr() for k, v in o.items()}


def map_outs(cap, nodes, D):
    """The device tensors of a map result (cap key weaves over `nodes` nodes)
    and their pointer dict."""
    o = {"seg_offsets": z(cap + 1, torch.int64), "seg_coll": z(cap, torch.int32),
         "seg_key": z(cap, torch.int64), "seg_active": z(cap, torch.int64),
         "seg_perm": z(nodes + cap, torch.int32), "status": z(D, torch.int32)}
    return o, {k: v.data_ptr() for k, v in o.items()}


def quantile_cuts(ids, D, n, ts_shift, site_shift, site_bits, q=0.5):
    """cut u64[D << site_bits]: per document (collection) and site rank the
    largest id whose ts is <= its q-quantile ts (0: the site has none)."""
    S = 1 << site_bits
    ids = ids.reshape(D, n)
    ts = ids >> np.uint64(ts_shift)
    T = np.sort(ts, axis=1)[:, min(int(q * n), n - 1)]
    older = np.where(ts <= T[:, None], ids, np.uint64(0))
    site = (ids >> np.uint64(site_shift)) & np.uint64(S - 1)
    cut = np.zeros((D, S), np.uint64)
    for r in range(S):
        cut[:, r] = np.where(site == np.uint64(r), older, np.uint64(0)).max(axis=1)
    return cut.reshape(-1)


def emit(line, out=None, mode="a"):
    """Print the JSON line; with `out`, also append it to (mode "w": write) that file."""
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, mode) as f:
            f.write(text + "\n")
