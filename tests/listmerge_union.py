"""Host reading of cw_merge_lists' union stage, shared by the GPU tests
(test_gpu_list_merge.py) and the CPU test that pins it to the restatement
(test_list_merge_ref.py).

A side is ``(offsets, id_key, cause_key, kind, value_token)``.  Per document the
two node bags are united by id: merged nodes in ascending id order, of equal
ids the copy with the smallest source index kept (a's before b's; source index
s = a's doc-local s, or na_d + b's doc-local s), and a repeated id whose body
(cause, kind, value token) differs sets CW_STATUS_DUP.
"""
import numpy as np

STATUS_DUP = 1 << 1


def host_union(a, b):
    """-> (src, bits): src[d] = the merged source indices of document d in id
    order (uint32), bits = uint32[D] with CW_STATUS_DUP where bodies differ."""
    D = len(a[0]) - 1
    bits = np.zeros(D, np.uint32)
    src = []
    for d in range(D):
        a0, a1, b0, b1 = int(a[0][d]), int(a[0][d + 1]), int(b[0][d]), int(b[0][d + 1])
        cat = lambda k: np.concatenate([a[k][a0:a1], b[k][b0:b1]])
        ids, body = cat(1), (cat(2), cat(3), cat(4))
        order = np.argsort(ids, kind="stable")  # equal ids: ascending source index
        sid = ids[order]
        keep = np.ones(len(sid), bool)
        keep[1:] = sid[1:] != sid[:-1]
        rep = np.flatnonzero(~keep)  # a repeat has the body of the copy before it, or DUP
        if len(rep) and any(np.any(f[order[rep]] != f[order[rep - 1]]) for f in body):
            bits[d] |= STATUS_DUP
        src.append(order[keep].astype(np.uint32))
    return src, bits


def merged_offsets(src):
    return np.concatenate([[0], np.cumsum([len(s) for s in src])]).astype(np.uint64)


def sides_of(src, a, b):
    """The (side, doc-local index) list of every document: side 0 = a, 1 = b."""
    out = []
    for d, s in enumerate(src):
        na = int(a[0][d + 1]) - int(a[0][d])
        out.append([(0, int(x)) if x < na else (1, int(x) - na) for x in s])
    return out


def union_arrays(src, a, b):
    """The merged documents as a list batch: (offsets, id_key, cause_key, kind)."""
    cols = [[], [], []]
    for d, s in enumerate(src):
        a0, b0 = int(a[0][d]), int(b[0][d])
        na = int(a[0][d + 1]) - a0
        s = s.astype(np.int64)
        fa = s < na
        ia, ib = a0 + s[fa], b0 + s[~fa] - na
        for k in range(3):
            col = np.empty(len(s), a[k + 1].dtype)
            col[fa], col[~fa] = a[k + 1][ia], b[k + 1][ib]
            cols[k].append(col)
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
    return (merged_offsets(src), cat(cols[0], np.uint64), cat(cols[1], np.uint64),
            cat(cols[2], np.uint8))
