"""Time cw_render_bases on the GPU: cb->edn of a batch of bases from its entry table.

    python scripts/render_bases_bench.py [--bases 10000] [--steps 20] [--out profiles/render_bases_bench.txt]

Two shapes in device memory, one JSON line each (also appended to --out):
  bases  invert_bench.py's shape: --bases bases of 100 collections of 100
         entries.  A base is a tree 4 deep: the root holds 9 collections, each
         of those 9 more, and 9 of the third level one more each; the refs sit
         among scalar entries.  Every collection is reached, no base is flagged.
  chain  one base that is a chain of 10^6 single-entry documents, numbered
         children first: the longest tour there is, it shows the jumping rounds.
Reported: the median, min, max and interquartile spread of --steps timed calls
after one warm-up call (host clock, the call's wait included); per kernel stat
the event time of a further run (cw_ctx_set_profiling), the algorithmic bytes
and GB/s on them; measured in the same run, a device-to-device copy whose
traffic (bytes read + bytes written) equals the entry bytes the three entry
passes read plus the token bytes written; and the Python recursion over the
same entry table on the first 64 bases, extrapolated linearly to all of them.
The first 64 bases' tokens of the first call are compared with that recursion
before anything is timed.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PER_BASE, ENTRIES = 100, 100
NONE = 0xFFFFFFFF


def spread(t):
    q = np.percentile(t, [25, 50, 75])
    return {"median": round(float(q[1]), 3), "min": round(float(np.min(t)), 3), "max": round(float(np.max(t)), 3),
            "iqr": round(float(q[2] - q[0]), 3)}


def tree_bases(G):
    """(ent_offsets, ent_ref, root_doc) of G bases: local document 0 is the root,
    1..9 its children (at its entries 5, 15, ..), 10..90 theirs, 91..99 one more
    level under 10..18."""
    parent = np.zeros(PER_BASE, np.int64)
    slot = np.zeros(PER_BASE, np.int64)
    for c in range(1, PER_BASE):
        if c < 10:
            parent[c], slot[c] = 0, 10 * (c - 1) + 5
        elif c < 91:
            parent[c], slot[c] = 1 + (c - 10) // 9, 10 * ((c - 10) % 9) + 5
        else:
            parent[c], slot[c] = 10 + (c - 91), 50
    D = G * PER_BASE
    ref = np.full((G, PER_BASE, ENTRIES), NONE, np.uint32)
    first = (np.arange(G, dtype=np.uint32) * np.uint32(PER_BASE))[:, None]
    c = np.arange(1, PER_BASE)
    ref[:, parent[c], slot[c]] = first + c.astype(np.uint32)
    off = np.arange(D + 1, dtype=np.uint64) * np.uint64(ENTRIES)
    return off, ref.reshape(-1), first[:, 0].copy()


def chain(n):
    off = np.arange(n + 1, dtype=np.uint64)
    ref = np.concatenate([[NONE], np.arange(n - 1)]).astype(np.uint32)      # document d holds a ref to d - 1
    return off, ref, np.array([n - 1], np.uint32)


def recurse(off, ref, D, roots):
    """cb->edn's recursion over the entry table, one Python step a value: the
    nested lists of entry indices (None for a ref to nothing)."""
    sys.setrecursionlimit(10_000)

    def go(d):
        out = []
        for e in range(off[d], off[d + 1]):
            t = ref[e]
            out.append(e if t == NONE else None if t >= D else go(t))
        return out
    return [go(r) for r in roots]


def from_tokens(kind, ent, lo, hi):
    """The same nested lists from a base's token stream [lo, hi): one stack pass."""
    stack, value = [], None
    for k, e in zip(kind[lo:hi], ent[lo:hi]):
        if k == 0:
            stack.append([])
        elif k == 1:
            value = stack.pop()
            if stack:
                stack[-1].append(value)
        else:
            stack[-1].append(e if k == 2 else None)
    return value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=10_000)
    ap.add_argument("--chain", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from _common import emit, timed, up, z
    from cause_amd import abi, abi_render_bases as RB

    note = lambda what: print(f"[render_bases_bench] {what}", file=sys.stderr, flush=True)
    torch.cuda.init()
    w = abi.Weaver(0)
    shapes = (("bases", f"{a.bases} bases of {PER_BASE} collections of {ENTRIES} entries, nested 4 deep",
               lambda: tree_bases(a.bases)),
              ("chain", f"one base, a chain of {a.chain} single-entry documents", lambda: chain(a.chain)))
    for name, what, make in shapes:
        note(f"{name}: building the entry table")
        off, ref, root = make()
        D, G, E = len(off) - 1, len(root), len(ref)
        cap = E + 2 * D
        g_ref, g_root = up(ref), up(root)
        o = {"tok_kind": z(cap, torch.uint8), "tok_doc": z(cap, torch.int32), "tok_entry": z(cap, torch.int32),
             "base_status": z(G, torch.int32), "doc_base": z(D, torch.int32), "doc_open": z(D, torch.int32)}
        ptrs = {k: v.data_ptr() for k, v in o.items()}
        torch.cuda.synchronize()
        call = lambda: RB.render_bases_device(w, off, g_ref.data_ptr(), G, g_root.data_ptr(), ptrs)
        note("warm-up and the comparison")
        bo = call()
        torch.cuda.synchronize()
        T = int(bo[-1])
        assert not o["base_status"].cpu().numpy().any() and T == E + 2 * D - (D - G)
        few = min(G, 64)
        lim = int(bo[few])
        kind, ent = o["tok_kind"][:lim].cpu().numpy().tolist(), o["tok_entry"][:lim].cpu().numpy().view(np.uint32).tolist()
        if name == "bases":
            offl, refl = off.tolist()[:few * PER_BASE + 1], ref[:int(off[few * PER_BASE])].tolist()
            t0 = time.perf_counter()
            want = recurse(offl, refl, D, root[:few].tolist())
            host_ms = (time.perf_counter() - t0) * 1e3
            assert [from_tokens(kind, ent, int(bo[g]), int(bo[g + 1])) for g in range(few)] == want
        else:                                     # (the recursion would be 10^6 frames deep)
            host_ms = None
            assert kind == [0] * D + [2] + [1] * D and ent[D] == 0
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
        nbytes = (3 * 4 * E + 9 * T) // 2
        src_, dst_ = z(nbytes, torch.uint8), z(nbytes, torch.uint8)
        dst_.copy_(src_)
        copies = [timed(lambda: dst_.copy_(src_))[0] for _ in range(a.steps)]
        del src_, dst_
        line = {"what": f"cw_render_bases, {name}: {what}, device memory", "bases": G, "docs": D, "entries": E,
                "tokens": T, "jump_rounds": int(kernels["k_rb_jump"]["launches_a_call"]), "steps": a.steps,
                "build": abi.build_id(), "call_ms": spread(times), "kernels_ms_a_call": round(total, 4),
                "kernels": kernels, "entry_and_token_bytes": 2 * nbytes, "d2d_copy_of_those_bytes_ms": spread(copies)}
        if host_ms is not None:
            line["python_recursion_ms"] = {"bases": few, "measured": round(host_ms, 1),
                                           "extrapolated_to_all_bases": round(host_ms * G / few, 1)}
        emit(line, a.out)
        del g_ref, g_root, o
    w.close()


if __name__ == "__main__":
    main()
