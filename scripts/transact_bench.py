"""Time cw_transact on the GPU: the nodes of a batch of transactions from their token streams.

    python scripts/transact_bench.py [--bases 10000] [--paste 100000000] [--deep 1000000] [--steps 20]
                                     [--out profiles/transact_bench.txt]

Three shapes in device memory, one JSON line each (also appended to --out):
  bases  --bases bases, each a root list of 9 lists of 9 maps of 9 lists of 11
         scalars and a string of 3: 10,388 tokens nested four deep, 820 new
         collections and 11,764 nodes (739 of them list roots) a base.
  paste  one base: one STR of --paste characters in a new root list.
  deep   one base: --deep lists nested in one another around one scalar.
Reported: the median, min, max and interquartile spread of --steps timed calls
after one warm-up call (host clock, the call's wait included); per kernel stat
the event time of a further run (cw_ctx_set_profiling), the algorithmic bytes
and GB/s on them; measured in the same run, a device-to-device copy whose
traffic (bytes read + bytes written) equals the token bytes the call must read
(15 B a token) plus the node and collection bytes it must write (31 B a node, 5 B
a collection); and, for `bases`, base.transact_ on 64 of the bases, extrapolated
linearly to all of them.  The counts of the first call are checked before
anything is timed.  Nothing is gated: the figures are recorded.
"""
import argparse
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEAF, STR, OPEN_LIST, OPEN_MAP, CLOSE, PART, ROOT_LIST, ROOT_MAP = range(8)


def spread(t):
    q = np.percentile(t, [25, 50, 75])
    return {"median": round(float(q[1]), 3), "min": round(float(np.min(t)), 3), "max": round(float(np.max(t)), 3),
            "iqr": round(float(q[2] - q[0]), 3)}


def one_base():
    """The token kinds, arguments, causes and cause_is_id of one base of `bases`,
    and the value it stands for."""
    toks = [(ROOT_LIST, 0, 0, 1)]
    for _ in range(9):
        toks.append((OPEN_LIST, 0, 0, 1))
        for b in range(9):
            toks.append((OPEN_MAP, 0, 0, 1))
            for c in range(9):
                toks.append((OPEN_LIST, 0, c, 0))
                toks += [(LEAF, 0, 0, 1)] * 11 + [(STR, 3, 0, 1), (CLOSE, 0, 0, 0)]
            toks.append((CLOSE, 0, 0, 0))
        toks.append((CLOSE, 0, 0, 0))
    toks.append((CLOSE, 0, 0, 0))
    value = [[{f"k{c}": [1] * 11 + ["abc"] for c in range(9)} for _ in range(9)] for _ in range(9)]
    return toks, value


def columns(toks, G=1):
    col = lambda k, dt: np.tile(np.array([t[k] for t in toks], dt), G)
    return col(0, np.uint8), col(1, np.uint32), col(2, np.uint64), col(3, np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=10_000)
    ap.add_argument("--paste", type=int, default=100_000_000)
    ap.add_argument("--deep", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import emit, timed, up, z
    from cause_amd import abi, abi_transact as TX, base as B, pack

    note = lambda what: print(f"[transact_bench] {what}", file=sys.stderr, flush=True)
    torch.cuda.init()
    w = abi.Weaver(0)
    lay = pack.KeyLayout(20, 10, 30)
    base_toks, value = one_base()
    n = len(base_toks)

    def bases():
        return a.bases, n, columns(base_toks, a.bases), a.bases * 820, a.bases * 11764

    def paste():
        return 1, 3, columns([(ROOT_LIST, 0, 0, 1), (STR, a.paste, 0, 1), (CLOSE, 0, 0, 0)]), 1, a.paste + 1

    def deep():
        toks = [(ROOT_LIST, 0, 0, 1)] + [(OPEN_LIST, 0, 0, 1)] * a.deep + [(LEAF, 0, 0, 1)] + [(CLOSE, 0, 0, 0)] * (a.deep + 1)
        return 1, len(toks), columns(toks), a.deep + 1, 2 * a.deep + 2

    shapes = (("bases", f"{a.bases} bases of {n} tokens nested four deep", bases),
              ("paste", f"one base, one STR of {a.paste} characters in a list", paste),
              ("deep", f"one base nested {a.deep} deep", deep))
    for name, what, make in shapes:
        note(f"{name}: building the token streams")
        G, per, cols, C, M = make()
        T = G * per
        doff, toff = np.zeros(G + 1, np.uint64), np.arange(G + 1, dtype=np.uint64) * np.uint64(per)
        ntx = np.array([lay.pack(5, g % 1024, 0) for g in range(G)], np.uint64)
        g_cols, g_ntx = [up(x) for x in cols], up(ntx)
        o = {f: z(M, getattr(torch, {"uint8": "uint8", "uint32": "int32", "uint64": "int64"}[np.dtype(dt).name]))
             for f, dt in TX.NODE_COLUMNS}
        o.update(new_is_map=z(C, torch.uint8), new_open=z(C, torch.int32), root_doc=z(G, torch.int32),
                 base_status=z(G, torch.int32))
        ptrs = {k: v.data_ptr() for k, v in o.items()}
        tok_ptrs = [x.data_ptr() for x in g_cols] + [None]
        torch.cuda.synchronize()
        call = lambda: TX.transact_device(w, doff, None, lay, g_ntx.data_ptr(), toff, tok_ptrs, C, M, ptrs)
        note("warm-up and the counts")
        bn, bm, no = call()
        torch.cuda.synchronize()
        assert int(bn[-1]) == C and int(bm[-1]) == M and not o["base_status"].cpu().numpy().any(), (bn[-1], bm[-1])
        host_ms = None
        if name == "bases":
            few = min(G, 64)
            cbs = [B.new_cb(random.Random(g)) for g in range(few)]
            t0 = time.perf_counter()
            done = [B.transact_(cb, [[None, None, value]]) for cb in cbs]
            host_ms = (time.perf_counter() - t0) * 1e3
            assert all(len(cb["collections"]) == 820 and len(cb["history"]) == 11764 - 739 for cb in done)
        note("timing")
        times = [timed(call)[0] for _ in range(a.steps)]
        w.reset_kernel_stats()
        w.set_profiling(True)
        for _ in range(a.steps):
            call()
        w.set_profiling(False)
        kernels, total = {}, 0.0
        for kname, (launches, ms, by) in sorted(w.kernel_stats().items()):
            total += ms / a.steps
            ms, by = ms / launches, by / launches
            kernels[kname] = {"launches_a_call": launches / a.steps, "ms": round(ms, 4), "bytes_alg": by,
                              "gb_per_s": round(by / (ms / 1e3) / 1e9, 1)}
        w.reset_kernel_stats()
        nbytes = (15 * T + 31 * M + 5 * C) // 2
        src_, dst_ = z(nbytes, torch.uint8), z(nbytes, torch.uint8)
        dst_.copy_(src_)
        copies = [timed(lambda: dst_.copy_(src_))[0] for _ in range(a.steps)]
        del src_, dst_
        line = {"what": f"cw_transact, {name}: {what}, device memory", "bases": G, "tokens": T, "new_collections": C,
                "nodes": M, "steps": a.steps, "build": abi.build_id(), "call_ms": spread(times),
                "kernels_ms_a_call": round(total, 4), "kernels": kernels, "token_and_node_bytes": 2 * nbytes,
                "d2d_copy_of_those_bytes_ms": spread(copies)}
        if host_ms is not None:
            line["python_transact_ms"] = {"bases": few, "measured": round(host_ms, 1),
                                          "extrapolated_to_all_bases": round(host_ms * G / few, 1)}
        emit(line, a.out)
        del g_cols, g_ntx, o
        torch.cuda.empty_cache()
    w.close()


if __name__ == "__main__":
    main()
