"""ctypes binding of include/causeweave.h (libcauseweave.so).

This is the Python side of the drop-in boundary: the same C entry points a JVM
shim binds through Panama/JNA.  There is no fallback: if the
HIP library is missing or fails, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CW_LIB: another build of the same library, for A/B timing runs on one box)
LIB_PATH = os.environ.get("CW_LIB") or os.path.join(_HERE, "libcauseweave.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "causeweave.h")

CW_MEM_HOST, CW_MEM_DEVICE = 0, 1
STATUS_ROOT, STATUS_DUP, STATUS_ORPHAN, STATUS_NON_LAMPORT, STATUS_INTERNAL = 1, 2, 4, 8, 32
STATUS_MAP_KEY = 16
STATUS_WEFT = 64
STATUS_KEY_RANGE = 128
STATUS_UNWOVEN = 256  # reserved: never set since round 4 (include/causeweave.h)
NIL32 = 0xFFFFFFFF
K32_RESERVED = 0xFFFFFFF0     # K32 words from here up = the top 16 K64 values (CW_NIL, ...)


def narrow_k32(id_key, cause_key):
    """K64 packed keys -> the K32 words of cw_weave_lists_k32.  The top 16 K64
    values (nil, the non-id cause) map to the top 16 K32 words; every other key
    must be below K32_RESERVED (ValueError otherwise)."""
    out = []
    for a in (id_key, cause_key):
        a = np.ascontiguousarray(a, np.uint64)
        top = a >= np.uint64((1 << 64) - 16)
        rest = np.where(top, np.uint64(0), a)
        if rest.size and int(rest.max()) >= K32_RESERVED:
            raise ValueError("keys do not fit K32 (every id and cause below 2^32 - 16)")
        out.append(a.astype(np.uint32))     # the top 16 keep their low 32 bits
    return out[0], out[1]


_U64P = C.POINTER(C.c_uint64)
# the fields every list batch starts with, and the key layout of the K64 / K32 ones
_NODES = [("n_docs", C.c_uint64), ("doc_offsets", _U64P), ("id_key", C.c_void_p),
          ("cause_key", C.c_void_p), ("kind", C.c_void_p)]
_LAYOUT = [("key_bits", C.c_uint32), ("ts_shift", C.c_uint32), ("site_shift", C.c_uint32),
           ("site_bits", C.c_uint32)]


class CwListBatch(C.Structure):
    _fields_ = _NODES + _LAYOUT


class CwListBatchK32(C.Structure):
    _fields_ = _NODES + _LAYOUT + [("perm16", C.c_uint32)]


class CwListBatchK128(C.Structure):
    _fields_ = _NODES


class CwListResult(C.Structure):
    _fields_ = [("weave_perm", C.c_void_p), ("visible_bits", C.c_void_p),
                ("visible_count", C.c_void_p), ("max_ts", C.c_void_p), ("status", C.c_void_p),
                ("yarn_perm", C.c_void_p)]


class CwMapBatch(C.Structure):
    _fields_ = [("n_colls", C.c_uint64), ("coll_offsets", _U64P),
                ("id_key", C.c_void_p), ("cause", C.c_void_p), ("cause_is_id", C.c_void_p),
                ("kind", C.c_void_p), ("key_bits", C.c_uint32), ("token_bits", C.c_uint32)]


class CwMapResult(C.Structure):
    _fields_ = [("cap_segs", C.c_uint64), ("n_segs", C.c_uint64), ("seg_offsets", C.c_void_p),
                ("seg_coll", C.c_void_p), ("seg_key", C.c_void_p), ("seg_active", C.c_void_p),
                ("seg_perm", C.c_void_p), ("status", C.c_void_p)]


class CwMergeBatch(C.Structure):
    _fields_ = [("a", CwListBatch), ("a_value", C.c_void_p), ("b", CwListBatch),
                ("b_value", C.c_void_p)]


class CwMergeResult(C.Structure):
    _fields_ = [("merged_offsets", _U64P), ("merged_src", C.c_void_p), ("weave", CwListResult)]


class CwMapMergeBatch(C.Structure):
    _fields_ = [("a", CwMapBatch), ("a_value", C.c_void_p), ("b", CwMapBatch),
                ("b_value", C.c_void_p)]


class CwMapMergeResult(C.Structure):
    _fields_ = [("merged_offsets", _U64P), ("merged_src", C.c_void_p), ("maps", CwMapResult)]


class CwWeftBatch(C.Structure):
    _fields_ = [("nodes", CwListBatch), ("cut", _U64P)]


class CwWeftResult(C.Structure):
    _fields_ = [("kept_offsets", _U64P), ("kept_src", C.c_void_p), ("weave", CwListResult)]


class CwMapWeftBatch(C.Structure):
    _fields_ = [("nodes", CwMapBatch), ("site_shift", C.c_uint32), ("site_bits", C.c_uint32),
                ("cut", C.c_void_p)]


class CwMapWeftResult(C.Structure):
    _fields_ = [("kept_offsets", _U64P), ("kept_src", C.c_void_p), ("maps", CwMapResult)]


class CwRenderBatch(C.Structure):
    _fields_ = [("n_docs", C.c_uint64), ("doc_offsets", _U64P),
                ("weave_perm", C.c_void_p), ("visible_bits", C.c_void_p), ("perm16", C.c_uint32),
                ("value_size", C.c_uint32), ("value", C.c_void_p)]


class CwRenderResult(C.Structure):
    _fields_ = [("rendered_offsets", _U64P), ("rendered_src", C.c_void_p),
                ("rendered_value", C.c_void_p)]


class CwMapRenderBatch(C.Structure):
    _fields_ = [("n_colls", C.c_uint64), ("n_segs", C.c_uint64), ("seg_coll", C.c_void_p),
                ("seg_key", C.c_void_p), ("seg_active", C.c_void_p),
                ("coll_offsets", _U64P), ("value_size", C.c_uint32),
                ("value", C.c_void_p)]


class CwMapRenderResult(C.Structure):
    _fields_ = [("entry_offsets", _U64P), ("entry_key", C.c_void_p),
                ("entry_src", C.c_void_p), ("entry_value", C.c_void_p)]


class CwRankedList(C.Structure):
    _fields_ = [("n", C.c_uint64), ("par", C.c_void_p), ("kind", C.c_void_p), ("val", C.c_void_p)]


class CwLinkedList(C.Structure):
    _fields_ = [("n", C.c_uint64), ("succ", C.c_void_p), ("thr", C.c_void_p), ("val", C.c_void_p)]


class CwKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double),
                ("bytes_alg", C.c_double)]


_KINDS = {"P": C.c_void_p, "U64": C.c_uint64, "U32": C.c_uint32, "I": C.c_int, "S": C.c_char_p,
          "void": None}


def _sig(restype, *args):
    """(restype, argtypes) from kind words (P = a pointer, S = char *, I = int)
    and struct classes, which stand for a pointer to that struct."""
    types = []
    for a in args:
        types += [_KINDS[k] for k in a.split()] if isinstance(a, str) else [C.POINTER(a)]
    return _KINDS[restype], types


def _batch_call(batch, result, memspace="I"):
    return _sig("I", "P", batch, result, memspace)


# every function include/causeweave.h declares -> (restype, argtypes); the
# context comes first wherever there is one
SIGNATURES = {
    "cw_abi_version": _sig("I"),
    "cw_build_id": _sig("S"),
    "cw_ctx_create": _sig("I", "I", C.c_void_p),
    "cw_ctx_destroy": _sig("void", "P"),
    "cw_last_error": _sig("S", "P"),
    "cw_ctx_set_stream": _sig("I", "P P"),
    "cw_ctx_set_async": _sig("I", "P I"),
    "cw_ctx_set_profiling": _sig("I", "P I"),
    "cw_ctx_set_profile_only": _sig("I", "P S"),
    "cw_ctx_set_option": _sig("I", "P S U32"),
    "cw_get_kernel_stats": _sig("I", "P", CwKernelStat, "I"),
    "cw_reset_kernel_stats": _sig("I", "P"),
    "cw_get_counter": _sig("I", "P S", C.c_uint64),
    "cw_weave_lists": _batch_call(CwListBatch, CwListResult),
    "cw_weave_lists_k32": _batch_call(CwListBatchK32, CwListResult),
    "cw_weave_lists_k128": _batch_call(CwListBatchK128, CwListResult),
    "cw_weave_maps": _batch_call(CwMapBatch, CwMapResult),
    "cw_merge_lists": _batch_call(CwMergeBatch, CwMergeResult),
    "cw_merge_maps": _batch_call(CwMapMergeBatch, CwMapMergeResult),
    "cw_weft_lists": _batch_call(CwWeftBatch, CwWeftResult),
    "cw_weft_lists_dev": _batch_call(CwWeftBatch, CwWeftResult, ""),
    "cw_weft_maps": _batch_call(CwMapWeftBatch, CwMapWeftResult),
    "cw_render_lists": _batch_call(CwRenderBatch, CwRenderResult),
    "cw_render_maps": _batch_call(CwMapRenderBatch, CwMapRenderResult),
    "cw_weave_ranked": _batch_call(CwRankedList, CwListResult, ""),
    "cw_weave_linked": _batch_call(CwLinkedList, CwListResult, ""),
    "cw_sort_keys": _sig("I", "P P U64 U32 P P"),
    "cw_sort_keys32": _sig("I", "P P U64 U32 P P"),
    "cw_lookup_keys": _sig("I", "P P U64 P U64 U32 P P"),
    "cw_partition_keys": _sig("I", "P P U64 P U32 P P"),
    "cw_partition_keys_dev": _sig("I", "P P U64 P U32 P P"),
    "cw_gather": _sig("I", "P P P U64 U32 P"),
    "cw_scatter32": _sig("I", "P P P U64 P"),
    # the distributed tree's building blocks (dist.hip)
    "cw_dist_check": _sig("I", "P U64 U32 P P P"),
    "cw_dist_eff": _sig("I", "P U64 U32 P P P"),
    "cw_dist_climb": _sig("I", "P U64 U32 P P P U64 P"),
    "cw_dist_pending": _sig("I", "P P U64 P P"),
    "cw_dist_gkey": _sig("I", "P P P U64 P"),
    "cw_dist_runs": _sig("I", "P P P U64 U32 P P P P"),
    "cw_dist_rkey": _sig("I", "P P U64 P"),
    "cw_dist_link": _sig("I", "P P P U64 P U32 U64 P P P"),
    "cw_dist_put": _sig("I", "P P P U64 U32 U64 P"),
    "cw_dist_thr": _sig("I", "P P U64 U32 P"),
    "cw_dist_succ": _sig("I", "P P P P U64 U32 P"),
    "cw_dist_rs_rulers": _sig("I", "P P P U64 U32 U32 U32 P P P"),
    "cw_dist_rs_walk": _sig("I", "P P U64 P U32 P P U64 U32 P P P P P P"),
    "cw_dist_rs_top": _sig("I", "P P U64 U64 P P"),
    "cw_dist_rs_pos": _sig("I", "P P P P P U64 P P"),
    "cw_dist_rs_emit": _sig("I", "P P U64 U32 U64 P P P P"),
}


_LIB = None


class WeaveError(RuntimeError):
    pass


def header_functions():
    """Names of every function declared in include/causeweave.h."""
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(cw_\w+)\s*\(", src, re.M)))


def build_id() -> str:
    """The loaded library's build id (a hash of its sources, see Makefile)."""
    return lib().cw_build_id().decode()


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64
    (soname libamdhip64.so.7, NEEDED by torch as plain "libamdhip64.so"): when
    this library loaded /opt/rocm's copy first, a later `import torch` loads a
    second runtime, which then sees no GPU, and device pointers / streams could
    not be shared.  Loading torch's copy first (without importing torch) makes
    libcauseweave.so bind to it (same soname) and torch reuse it (same path).
    CW_HIP_RUNTIME=system keeps /opt/rocm's runtime."""
    if os.environ.get("CW_HIP_RUNTIME") == "system":
        return
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        C.CDLL(path, mode=C.RTLD_GLOBAL)


def lib():
    """Load libcauseweave.so (raises if it was not built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise WeaveError(f"{LIB_PATH} is missing: build it (python -c "
                             "'import __graft_entry__ as g; g.build()' or `make`)")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if hasattr(L, name):  # (an older build, named by CW_LIB for an A/B run, may lack it)
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


@dataclass
class ListResult:
    weave_perm: np.ndarray     # uint32[N] doc-local input index per weave position
    visible_bits: np.ndarray   # uint32[(N+31)//32]
    visible_count: np.ndarray  # uint32[D]
    max_ts: np.ndarray         # uint64[D]
    status: np.ndarray         # uint32[D]
    yarn_perm: np.ndarray | None

    def visible(self) -> np.ndarray:
        """uint8[N]: 1 where the global weave position renders."""
        n = len(self.weave_perm)
        b = np.unpackbits(self.visible_bits.view(np.uint8), bitorder="little")
        return b[:n]


@dataclass
class MergeResult:
    """Union of two node bags per document and its weave (cw_merge_lists)."""
    offsets: np.ndarray      # uint64[D+1] merged documents
    src: np.ndarray          # uint32[M] merged nodes in id order: < na_d -> a, else b (- na_d)
    weave: ListResult        # weave_perm holds doc-local merged indices (into src)

    def weave_src(self) -> np.ndarray:
        """uint32[M]: source index (as in src) of every weave position."""
        out = np.empty_like(self.weave.weave_perm)
        for d in range(len(self.offsets) - 1):
            lo, hi = int(self.offsets[d]), int(self.offsets[d + 1])
            out[lo:hi] = self.src[lo:hi][self.weave.weave_perm[lo:hi]]
        return out


@dataclass
class MapResult:
    """Key weaves of a batch of maps, per collection in ascending key-token order."""
    seg_offsets: np.ndarray  # uint64[S+1] into seg_perm
    seg_coll: np.ndarray     # uint32[S]
    seg_key: np.ndarray      # uint64[S] key token
    seg_active: np.ndarray   # int64[S] collection-local input index, -1 = ::blank
    seg_perm: np.ndarray     # uint32[N+S] root (UINT32_MAX) then input indices, weave order
    status: np.ndarray       # uint32[n_colls]

    def key_weave(self, s):
        return self.seg_perm[int(self.seg_offsets[s]):int(self.seg_offsets[s + 1])]


@dataclass
class MapMergeResult:
    """Union of two node bags per collection and its map weave (cw_merge_maps)."""
    offsets: np.ndarray      # uint64[D+1] merged collections
    src: np.ndarray          # uint32[M] merged nodes in id order: < na_d -> a, else b (- na_d)
    maps: MapResult          # every index is collection-local into src


@dataclass
class MapWeftResult:
    """Kept nodes per collection and their map weave (cw_weft_maps)."""
    offsets: np.ndarray      # uint64[D+1] kept collections
    src: np.ndarray          # uint32[M] kept nodes in input order, then UINT32_MAX per [id] node
    maps: MapResult          # every index is collection-local into src


@dataclass
class RenderResult:
    """Rendered nodes per document (cw_render_lists)."""
    offsets: np.ndarray        # uint64[D+1] rendered documents; their differences are `count`
    src: np.ndarray            # uint32[R] doc-local index of each rendered node, weave order
    value: np.ndarray | None   # [R] its value word (the dtype of the value column)


@dataclass
class MapRenderResult:
    """Non-blank key weaves per collection (cw_render_maps)."""
    offsets: np.ndarray        # uint64[D+1]; their differences are `count-`
    key: np.ndarray            # uint64[R] seg_key of each entry, ascending in a collection
    src: np.ndarray            # uint32[R] collection-local index of its active node
    value: np.ndarray | None   # [R] the active node's value word


_VALUE_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _value_column(value):
    """A value column as an unsigned array of its item size (1, 2, 4 or 8 bytes)."""
    if value is None:
        return None
    v = np.ascontiguousarray(value)
    if v.dtype.itemsize not in _VALUE_DTYPES:
        raise ValueError("value words of 1, 2, 4 or 8 bytes")
    return v.view(_VALUE_DTYPES[v.dtype.itemsize])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _u64p(a):
    return a.ctypes.data_as(_U64P) if a is not None else None


def _vp(p):
    """A raw device pointer (an int; None or 0 = NULL) as a struct field."""
    return C.c_void_p(p) if p else None


def _u64(a):
    return np.ascontiguousarray(a, np.uint64)


_LIST_DT = (np.uint64, np.uint64, np.uint8)           # id_key, cause_key, kind
_MAP_DT = (np.uint64, np.uint64, np.uint8, np.uint8)  # id_key, cause, cause_is_id, kind


def _host_nodes(offsets, columns, dtypes, what, every=True):
    """Host offsets and node columns as contiguous arrays of their dtypes.
    ValueError(what) unless the first column (every: each one) has offsets[-1]
    elements."""
    off = _u64(offsets)
    cols = [np.ascontiguousarray(x, dt) for x, dt in zip(columns, dtypes)]
    n = int(off[-1])
    if any(len(x) != n for x in (cols if every else cols[:1])):
        raise ValueError(what)
    return off, cols


# A ctypes struct keeps no numpy array alive: whoever builds one holds the
# arrays it points into in locals until the C call has returned.  The builders
# below return those arrays next to the struct.

def _list_result(out_ptrs, null=()):
    """CwListResult from a dict of device pointers (absent, None or 0 = NULL)."""
    return CwListResult(*[None if f in null else _vp(out_ptrs.get(f))
                          for f, _ in CwListResult._fields_])


def _map_result(out_ptrs, cap_segs):
    """CwMapResult from a dict of device pointers and the key-weave capacity."""
    return CwMapResult(cap_segs, 0, *[_vp(out_ptrs.get(f)) for f, _ in CwMapResult._fields_[2:]])


def _new_list_result(n, words, D, yarns):
    """Zeroed host arrays of a list result (n per node, `words` of bitmap, D
    per document) and the CwListResult that points at them."""
    out = ListResult(np.zeros(n, np.uint32), np.zeros(words, np.uint32), np.zeros(D, np.uint32),
                     np.zeros(D, np.uint64), np.zeros(D, np.uint32),
                     np.zeros(n, np.uint32) if yarns else None)
    return out, CwListResult(*[_ptr(getattr(out, f)) for f, _ in CwListResult._fields_])


def _trim_list_result(w, M, D):
    return ListResult(w.weave_perm[:M], w.visible_bits[:(M + 31) // 32], w.visible_count[:D],
                      w.max_ts[:D], w.status[:D], None if w.yarn_perm is None else w.yarn_perm[:M])


def _new_map_result(cap, nodes, D):
    """Zeroed host arrays of a map result (cap key weaves over `nodes` nodes in
    D collections) and the CwMapResult that points at them."""
    out = MapResult(np.zeros(cap + 1, np.uint64), np.zeros(cap, np.uint32),
                    np.zeros(cap, np.uint64), np.zeros(cap, np.int64),
                    np.zeros(nodes + cap, np.uint32), np.zeros(max(D, 1), np.uint32))
    return out, CwMapResult(cap, 0, *[_ptr(getattr(out, f)) for f, _ in CwMapResult._fields_[2:]])


def _trim_map_result(out, S, M, D):
    return MapResult(out.seg_offsets[:S + 1], out.seg_coll[:S], out.seg_key[:S],
                     out.seg_active[:S], out.seg_perm[:M + S], out.status[:D])


class Weaver:
    """A weave context on one HIP device (cw_ctx)."""

    def __init__(self, device: int = 0, options: dict[str, int] | None = None):
        """options: name -> value for cw_ctx_set_option (INTEGRATION.md lists them)."""
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.cw_ctx_create(device, C.byref(h))
        if rc != 0 or not h:
            raise WeaveError(f"cw_ctx_create(device={device}) failed: no usable HIP device")
        self._h = h
        self.device = device
        for name, value in (options or {}).items():
            self.set_option(name, value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.cw_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise WeaveError(f"{what}: {self._L.cw_last_error(self._h).decode()}")

    def set_stream(self, stream_ptr):
        self._check(self._L.cw_ctx_set_stream(self._h, C.c_void_p(stream_ptr)), "set_stream")

    def set_async(self, on: bool):
        self._check(self._L.cw_ctx_set_async(self._h, int(on)), "set_async")

    def set_profiling(self, on: bool):
        self._check(self._L.cw_ctx_set_profiling(self._h, int(on)), "set_profiling")

    def set_profile_only(self, kernel: str | None):
        """Per-kernel events for this kernel stat name only (None: every kernel)."""
        self._check(self._L.cw_ctx_set_profile_only(self._h, kernel.encode() if kernel else None),
                    "set_profile_only")

    def set_option(self, name: str, value: int):
        """A path or geometry option, from the next call on (cw_ctx_set_option)."""
        self._check(self._L.cw_ctx_set_option(self._h, name.encode(), int(value)), "set_option")

    def kernel_stats(self):
        n = self._L.cw_get_kernel_stats(self._h, None, 0)
        arr = (CwKernelStat * max(n, 1))()
        self._L.cw_get_kernel_stats(self._h, arr, n)
        return {a.name.decode(): (a.launches, a.total_ms, a.bytes_alg) for a in arr[:n]}

    def reset_kernel_stats(self):
        self._L.cw_reset_kernel_stats(self._h)

    def counter(self, name: str) -> int:
        """A diagnostic counter of the last call (cw_get_counter; waits for the
        stream): "continued_sublists" = walk-slot overflows of the last HBM walk."""
        v = C.c_uint64(0)
        self._check(self._L.cw_get_counter(self._h, name.encode(), C.byref(v)), "get_counter")
        return int(v.value)

    @staticmethod
    def _list_batch(cls, offsets, id_ptr, cause_ptr, kind_ptr, layout=None, key_bits=None, **more):
        """A CwListBatch / K32 / K128 and the offsets array it points into."""
        off = _u64(offsets)
        b = cls(len(off) - 1, _u64p(off), id_ptr, cause_ptr, kind_ptr, **more)
        if layout is not None:
            b.key_bits = layout.key_bits if key_bits is None else key_bits
            b.ts_shift, b.site_shift, b.site_bits = layout.ts_shift, layout.site_shift, layout.site_bits
        return b, off

    @staticmethod
    def _batch(offsets, id_ptr, cause_ptr, kind_ptr, layout, key_bits=None):
        return Weaver._list_batch(CwListBatch, offsets, id_ptr, cause_ptr, kind_ptr, layout, key_bits)

    def _weave_host(self, fn, b, N, D, yarns) -> ListResult:
        out, r = _new_list_result(N, (N + 31) // 32, D, yarns)
        self._check(getattr(self._L, fn)(self._h, C.byref(b), C.byref(r), CW_MEM_HOST), fn)
        return out

    def _weave_device(self, fn, b, out_ptrs):
        r = _list_result(out_ptrs)
        self._check(getattr(self._L, fn)(self._h, C.byref(b), C.byref(r), CW_MEM_DEVICE), fn)

    def weave_lists(self, offsets, id_key, cause_key, kind, layout, yarns=True,
                    key_bits=None) -> ListResult:
        """Host-memory call: numpy in, numpy out."""
        off, cols = _host_nodes(offsets, (id_key, cause_key, kind), _LIST_DT,
                                "offsets[-1] != number of nodes", every=False)
        b, off = self._batch(off, *map(_ptr, cols), layout, key_bits)
        return self._weave_host("cw_weave_lists", b, len(cols[0]), len(off) - 1,
                                yarns and layout.site_bits)

    def weave_lists_device(self, offsets, id_ptr, cause_ptr, kind_ptr, layout, out_ptrs,
                           key_bits=None):
        """Device-memory call: raw device pointers (e.g. torch tensor data_ptr()).
        out_ptrs: dict with weave_perm, visible_bits, visible_count, max_ts,
        status, yarn_perm (None allowed where the header allows NULL)."""
        b, off = self._batch(offsets, _vp(id_ptr), _vp(cause_ptr), _vp(kind_ptr), layout, key_bits)
        self._weave_device("cw_weave_lists", b, out_ptrs)

    def weave_lists_k32(self, offsets, id_key, cause_key, kind, layout, yarns=True,
                        key_bits=None) -> ListResult:
        """Host-memory call of cw_weave_lists_k32: id_key / cause_key are uint32
        (nil = NIL32, see narrow_k32)."""
        off, cols = _host_nodes(offsets, (id_key, cause_key, kind), (np.uint32, np.uint32, np.uint8),
                                "offsets[-1] / id_key / cause_key / kind sizes differ")
        b, off = self._list_batch(CwListBatchK32, off, *map(_ptr, cols), layout, key_bits, perm16=0)
        return self._weave_host("cw_weave_lists_k32", b, len(cols[0]), len(off) - 1,
                                yarns and layout.site_bits)

    def weave_lists_k32_device(self, offsets, id_ptr, cause_ptr, kind_ptr, layout, out_ptrs,
                               key_bits=None, perm16=False):
        """Device-memory call of cw_weave_lists_k32 (u32 keys; out_ptrs as
        weave_lists_device; perm16: weave_perm is uint16 per node)."""
        b, off = self._list_batch(CwListBatchK32, offsets, _vp(id_ptr), _vp(cause_ptr),
                                  _vp(kind_ptr), layout, key_bits, perm16=int(perm16))
        self._weave_device("cw_weave_lists_k32", b, out_ptrs)

    def weave_lists_k128(self, offsets, id_key, cause_key, kind, yarns=True) -> ListResult:
        """Host-memory call of cw_weave_lists_k128: id_key / cause_key are
        uint64[N, 2] (hi = ts, lo = site_rank << 32 | tx; nil = (NIL, NIL))."""
        i, c = (_u64(x).reshape(-1, 2) for x in (id_key, cause_key))
        off, cols = _host_nodes(offsets, (i, c, kind), _LIST_DT,
                                "offsets[-1] / id_key / cause_key / kind sizes differ")
        b, off = self._list_batch(CwListBatchK128, off, *map(_ptr, cols))
        return self._weave_host("cw_weave_lists_k128", b, len(cols[2]), len(off) - 1, yarns)

    def weave_lists_k128_device(self, offsets, id_ptr, cause_ptr, kind_ptr, out_ptrs):
        """Device-memory call of cw_weave_lists_k128 (out_ptrs as weave_lists_device)."""
        b, off = self._list_batch(CwListBatchK128, offsets, _vp(id_ptr), _vp(cause_ptr),
                                  _vp(kind_ptr))
        self._weave_device("cw_weave_lists_k128", b, out_ptrs)

    # --- building blocks of the distributed giant list (device pointers) ---------
    def sort_keys_device(self, keys_ptr, n, key_bits, keys_out_ptr, idx_out_ptr):
        self._check(self._L.cw_sort_keys(self._h, keys_ptr, n, key_bits, keys_out_ptr, idx_out_ptr),
                    "cw_sort_keys")

    def sort_keys(self, keys, key_bits=0):
        """Host arrays: (sorted keys, input index of each) through cw_sort_keys
        (device buffers from torch; the call is synchronous)."""
        import torch

        k = np.ascontiguousarray(keys, np.uint64)
        n = len(k)
        if n == 0:
            return k.copy(), np.zeros(0, np.uint32)
        dev = torch.device("cuda", self.device)
        kin = torch.from_numpy(k.view(np.int64)).to(dev)
        kout = torch.empty_like(kin)
        iout = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.sort_keys_device(kin.data_ptr(), n, key_bits, kout.data_ptr(), iout.data_ptr())
        return kout.cpu().numpy().view(np.uint64), iout.cpu().numpy().view(np.uint32)

    def lookup_keys_device(self, sorted_ptr, n, q_ptr, m, base, out_ptr, status_ptr=None):
        self._check(self._L.cw_lookup_keys(self._h, sorted_ptr, n, q_ptr, m, base, out_ptr,
                                           status_ptr), "cw_lookup_keys")

    def partition_keys_device(self, keys_ptr, m, split_ptr, n_split, perm_ptr) -> np.ndarray:
        counts = np.zeros(n_split + 1, np.uint64)
        self._check(self._L.cw_partition_keys(self._h, keys_ptr, m, split_ptr, n_split, perm_ptr,
                                              counts.ctypes.data), "cw_partition_keys")
        return counts

    def partition_keys_dev(self, keys_ptr, m, split_ptr, n_split, perm_ptr, counts_ptr):
        """cw_partition_keys with the n_split + 1 counts (u64) left in device memory."""
        self._check(self._L.cw_partition_keys_dev(self._h, keys_ptr, m, split_ptr, n_split, perm_ptr,
                                                  counts_ptr), "cw_partition_keys_dev")

    def gather_device(self, src_ptr, idx_ptr, m, elem_size, dst_ptr):
        self._check(self._L.cw_gather(self._h, src_ptr, idx_ptr, m, elem_size, dst_ptr), "cw_gather")

    def scatter32_device(self, src_ptr, idx_ptr, m, dst_ptr):
        self._check(self._L.cw_scatter32(self._h, src_ptr, idx_ptr, m, dst_ptr), "cw_scatter32")

    def weave_ranked_device(self, n, par_ptr, kind_ptr, val_ptr, out_ptrs):
        """out_ptrs: weave_perm, visible_bits (or None), visible_count, status."""
        lst = CwRankedList(n, par_ptr, kind_ptr, val_ptr)
        r = _list_result(out_ptrs, null=("max_ts", "yarn_perm"))
        self._check(self._L.cw_weave_ranked(self._h, C.byref(lst), C.byref(r)), "cw_weave_ranked")

    def sort_keys32_device(self, keys_ptr, n, key_bits, keys_out_ptr, idx_out_ptr):
        self._check(self._L.cw_sort_keys32(self._h, keys_ptr, n, key_bits, keys_out_ptr,
                                           idx_out_ptr), "cw_sort_keys32")

    def dist(self, name, *args):
        """cw_dist_<name>(ctx, *args): a building block of the distributed tree
        (device pointers as ints, sizes, bases)."""
        self._check(getattr(self._L, "cw_dist_" + name)(self._h, *args), "cw_dist_" + name)

    def weave_linked_device(self, n, succ_ptr, thr_ptr, val_ptr, out_ptrs):
        """cw_weave_linked: out_ptrs as weave_ranked_device."""
        lst = CwLinkedList(n, succ_ptr, thr_ptr, val_ptr)
        r = _list_result(out_ptrs, null=("max_ts", "yarn_perm"))
        self._check(self._L.cw_weave_linked(self._h, C.byref(lst), C.byref(r)), "cw_weave_linked")

    # --- merge and weft: a node selection per document, then its weave --------------
    def _kept_lists_host(self, fn, batch, result, nodes, words, D, yarns) -> MergeResult:
        """The host call of a list merge or weft: room for `nodes` in every
        per-node array, the result trimmed to the offsets the library returns."""
        offs, src = np.zeros(D + 1, np.uint64), np.zeros(nodes, np.uint32)
        w, wr = _new_list_result(nodes, words, max(D, 1), yarns)
        r = result(_u64p(offs), _ptr(src), wr)
        self._check(getattr(self._L, fn)(self._h, C.byref(batch), C.byref(r), CW_MEM_HOST), fn)
        M = int(offs[-1])
        return MergeResult(offs, src[:M], _trim_list_result(w, M, D))

    def _kept_lists_device(self, fn, batch, result, D, src_ptr, out_ptrs, *memspace):
        offs = np.zeros(D + 1, np.uint64)
        r = result(_u64p(offs), _vp(src_ptr), _list_result(out_ptrs))
        self._check(getattr(self._L, fn)(self._h, C.byref(batch), C.byref(r), *memspace), fn)
        return offs

    def _kept_maps_host(self, fn, batch, result, nodes, D):
        """As _kept_lists_host for maps: (offsets, src, MapResult), every node a
        possible key weave."""
        cap = max(nodes, 1)
        offs, src = np.zeros(D + 1, np.uint64), np.zeros(cap, np.uint32)
        out, mr = _new_map_result(cap, nodes, D)
        r = result(_u64p(offs), _ptr(src), mr)
        self._check(getattr(self._L, fn)(self._h, C.byref(batch), C.byref(r), CW_MEM_HOST), fn)
        S, M = int(r.maps.n_segs), int(offs[-1])
        return offs, src[:M], _trim_map_result(out, S, M, D)

    def _kept_maps_device(self, fn, batch, result, D, src_ptr, out_ptrs, cap_segs):
        offs = np.zeros(D + 1, np.uint64)
        r = result(_u64p(offs), _vp(src_ptr), _map_result(out_ptrs, cap_segs))
        self._check(getattr(self._L, fn)(self._h, C.byref(batch), C.byref(r), CW_MEM_DEVICE), fn)
        return offs, int(r.maps.n_segs)

    def merge_lists(self, a, b, layout, yarns=True) -> MergeResult:
        """Host-memory call of cw_merge_lists.  a, b: (offsets, id_key, cause_key,
        kind, value_token) per side, with the same number of documents."""
        what = "offsets[-1] != number of nodes"
        ao, ac = _host_nodes(a[0], a[1:], _LIST_DT + (np.uint64,), what, every=False)
        bo, bc = _host_nodes(b[0], b[1:], _LIST_DT + (np.uint64,), what, every=False)
        if len(ao) != len(bo):
            raise ValueError("a and b must have the same number of documents")
        D, NC = len(ao) - 1, len(ac[0]) + len(bc[0])
        # (ao and bo are uint64 arrays already, so the batches point into them)
        mb = CwMergeBatch(self._batch(ao, *map(_ptr, ac[:3]), layout)[0], _ptr(ac[3]),
                          self._batch(bo, *map(_ptr, bc[:3]), layout)[0], _ptr(bc[3]))
        return self._kept_lists_host("cw_merge_lists", mb, CwMergeResult, max(NC, 1),
                                     (NC + 31) // 32 + 1, D, yarns and layout.site_bits)

    def merge_lists_device(self, a_offsets, a_ptrs, b_offsets, b_ptrs, layout, src_ptr, out_ptrs):
        """Device-memory call of cw_merge_lists.  a_ptrs / b_ptrs = (id_key,
        cause_key, kind, value) device pointers; src_ptr: merged_src (uint32
        [Na+Nb]); out_ptrs as weave_lists_device, every array sized for Na+Nb.
        Returns the merged offsets (uint64[D+1])."""
        ao, bo = _u64(a_offsets), _u64(b_offsets)
        if len(ao) != len(bo):
            raise ValueError("a and b must have the same number of documents")
        mb = CwMergeBatch(self._batch(ao, *map(_vp, a_ptrs[:3]), layout)[0], _vp(a_ptrs[3]),
                          self._batch(bo, *map(_vp, b_ptrs[:3]), layout)[0], _vp(b_ptrs[3]))
        return self._kept_lists_device("cw_merge_lists", mb, CwMergeResult, len(ao) - 1, src_ptr,
                                       out_ptrs, CW_MEM_DEVICE)

    def weft_lists(self, offsets, id_key, cause_key, kind, layout, cut, yarns=True) -> MergeResult:
        """Host-memory call of cw_weft_lists.  cut: uint64[D << site_bits] packed
        cut id per (document, site rank), 0 = site not named.  Returns the kept
        nodes (src = doc-local input index, input order) and their weave."""
        cut = _u64(cut)
        off, cols = _host_nodes(offsets, (id_key, cause_key, kind), _LIST_DT,
                                "offsets / cut sizes", every=False)
        D, N = len(off) - 1, len(cols[0])
        if len(cut) != D << layout.site_bits:
            raise ValueError("offsets / cut sizes")
        b, off = self._batch(off, *map(_ptr, cols), layout)
        cap = max(N + (D << layout.site_bits), 1)  # + one [id] node per named site
        return self._kept_lists_host("cw_weft_lists", CwWeftBatch(b, _u64p(cut)), CwWeftResult,
                                     cap, (cap + 31) // 32 + 1, D, yarns and layout.site_bits)

    def weft_lists_device(self, offsets, ptrs, layout, cut_ptr, src_ptr, out_ptrs):
        """Device-memory call (cw_weft_lists_dev).  ptrs = (id_key, cause_key,
        kind) device pointers; cut_ptr: uint64[D << site_bits] in device memory;
        src_ptr: kept_src (uint32); out_ptrs as weave_lists_device; src and
        every per-node array sized for N + (D << site_bits).  Returns the kept
        offsets (uint64[D+1])."""
        b, off = self._batch(offsets, *map(_vp, ptrs[:3]), layout)
        wb = CwWeftBatch(b, C.cast(_vp(cut_ptr), _U64P))
        return self._kept_lists_device("cw_weft_lists_dev", wb, CwWeftResult, len(off) - 1,
                                       src_ptr, out_ptrs)

    # --- maps ---------------------------------------------------------------------
    @staticmethod
    def _map_batch(off, ptrs, key_bits, token_bits):
        """A CwMapBatch over `off`, a uint64 array the caller keeps alive."""
        b = CwMapBatch(len(off) - 1, _u64p(off), key_bits=key_bits, token_bits=token_bits)
        b.id_key, b.cause, b.cause_is_id, b.kind = ptrs
        return b

    def weave_maps_device(self, offsets, ptrs, token_bits, key_bits, out_ptrs, cap_segs) -> int:
        """Device-memory call of cw_weave_maps: ptrs = (id_key, cause, cause_is_id,
        kind) device pointers; out_ptrs: seg_offsets, seg_coll, seg_key,
        seg_active, seg_perm, status device pointers.  Returns n_segs."""
        off = _u64(offsets)
        b = self._map_batch(off, [_vp(p) for p in ptrs], key_bits, token_bits)
        r = _map_result(out_ptrs, cap_segs)
        self._check(self._L.cw_weave_maps(self._h, C.byref(b), C.byref(r), CW_MEM_DEVICE),
                    "cw_weave_maps")
        return int(r.n_segs)

    def weave_maps(self, offsets, id_key, cause, cause_is_id, kind, token_bits,
                   key_bits=0) -> MapResult:
        """Host-memory call of cw_weave_maps."""
        off, cols = _host_nodes(offsets, (id_key, cause, cause_is_id, kind), _MAP_DT,
                                "offsets[-1] != number of nodes", every=False)
        D, N = len(off) - 1, len(cols[0])
        b = self._map_batch(off, [_ptr(x) for x in cols], key_bits, token_bits)
        out, r = _new_map_result(max(N, 1), N, D)
        self._check(self._L.cw_weave_maps(self._h, C.byref(b), C.byref(r), CW_MEM_HOST),
                    "cw_weave_maps")
        return _trim_map_result(out, int(r.n_segs), N, D)

    def merge_maps_device(self, a_offsets, a_ptrs, b_offsets, b_ptrs, token_bits, key_bits,
                          src_ptr, out_ptrs, cap_segs):
        """Device-memory call of cw_merge_maps.  a_ptrs / b_ptrs = (id_key, cause,
        cause_is_id, kind, value) device pointers; src_ptr: merged_src (uint32
        [Na+Nb]); out_ptrs as weave_maps_device (seg_perm sized Na+Nb+cap_segs).
        Returns (merged offsets uint64[D+1], n_segs)."""
        ao, bo = _u64(a_offsets), _u64(b_offsets)
        if len(ao) != len(bo):
            raise ValueError("a and b must have the same number of collections")
        ba = self._map_batch(ao, [_vp(p) for p in a_ptrs[:4]], key_bits, token_bits)
        bb = self._map_batch(bo, [_vp(p) for p in b_ptrs[:4]], key_bits, token_bits)
        mb = CwMapMergeBatch(ba, _vp(a_ptrs[4]), bb, _vp(b_ptrs[4]))
        return self._kept_maps_device("cw_merge_maps", mb, CwMapMergeResult, len(ao) - 1, src_ptr,
                                      out_ptrs, cap_segs)

    def merge_maps(self, a, b, token_bits, key_bits=0) -> MapMergeResult:
        """Host-memory call of cw_merge_maps.  a, b: (offsets, id_key, cause,
        cause_is_id, kind, value_token) per side, with the same number of
        collections."""
        what = "offsets[-1] != number of nodes"
        ao, aa = _host_nodes(a[0], a[1:], _MAP_DT + (np.uint64,), what)
        bo, ab = _host_nodes(b[0], b[1:], _MAP_DT + (np.uint64,), what)
        if len(ao) != len(bo):
            raise ValueError("a and b must have the same number of collections")
        ba = self._map_batch(ao, [_ptr(x) for x in aa[:4]], key_bits, token_bits)
        bb = self._map_batch(bo, [_ptr(x) for x in ab[:4]], key_bits, token_bits)
        mb = CwMapMergeBatch(ba, _ptr(aa[4]), bb, _ptr(ab[4]))
        return MapMergeResult(*self._kept_maps_host("cw_merge_maps", mb, CwMapMergeResult,
                                                    len(aa[0]) + len(ab[0]), len(ao) - 1))

    def weft_maps_device(self, offsets, ptrs, token_bits, key_bits, site_shift, site_bits, cut_ptr,
                         src_ptr, out_ptrs, cap_segs):
        """Device-memory call of cw_weft_maps.  ptrs = (id_key, cause, cause_is_id,
        kind) device pointers; cut_ptr: the cut table (uint64[D << site_bits]) in
        device memory; src_ptr: kept_src (uint32[N + (D << site_bits)]); out_ptrs
        as weave_maps_device (seg_perm sized N + (D << site_bits) + cap_segs).
        Returns (kept offsets uint64[D+1], n_segs)."""
        off = _u64(offsets)
        wb = CwMapWeftBatch(self._map_batch(off, [_vp(p) for p in ptrs], key_bits, token_bits),
                            site_shift, site_bits, _vp(cut_ptr))
        return self._kept_maps_device("cw_weft_maps", wb, CwMapWeftResult, len(off) - 1, src_ptr,
                                      out_ptrs, cap_segs)

    def weft_maps(self, offsets, id_key, cause, cause_is_id, kind, token_bits, site_shift,
                  site_bits, cut, key_bits=0) -> MapWeftResult:
        """Host-memory call of cw_weft_maps.  cut: uint64[D << site_bits] packed
        cut id per (collection, site rank), 0 = site not named.  Returns the kept
        nodes (src = collection-local input index, input order, then UINT32_MAX
        per [id] node) and their map weave."""
        cut = _u64(cut)
        off, cols = _host_nodes(offsets, (id_key, cause, cause_is_id, kind), _MAP_DT,
                                "offsets[-1] != number of nodes")
        D, N = len(off) - 1, len(cols[0])
        if 1 <= site_bits <= 10 and len(cut) != D << site_bits:  # (else: the library's error)
            raise ValueError("cut size != collections << site_bits")
        wb = CwMapWeftBatch(self._map_batch(off, [_ptr(x) for x in cols], key_bits, token_bits),
                            site_shift, site_bits, _ptr(cut))
        # + one [id] node per named site
        return MapWeftResult(*self._kept_maps_host("cw_weft_maps", wb, CwMapWeftResult,
                                                   N + (D << site_bits), D))

    # --- render: causal->edn / count of woven lists and maps -----------------------
    def render_lists_device(self, offsets, perm_ptr, bits_ptr, src_ptr=None, value_ptr=None,
                            value_size=0, out_value_ptr=None, perm16=False) -> np.ndarray:
        """Device-memory call of cw_render_lists: raw device pointers to
        weave_perm (uint32, or uint16 with perm16), visible_bits, the value
        column and the outputs rendered_src / rendered_value (None = NULL).
        Returns the rendered offsets (uint64[D+1])."""
        off = _u64(offsets)
        b = CwRenderBatch(len(off) - 1, _u64p(off), _vp(perm_ptr), _vp(bits_ptr), int(perm16),
                          value_size, _vp(value_ptr))
        ro = np.zeros(len(off), np.uint64)
        r = CwRenderResult(_u64p(ro), _vp(src_ptr), _vp(out_value_ptr))
        self._check(self._L.cw_render_lists(self._h, C.byref(b), C.byref(r), CW_MEM_DEVICE),
                    "cw_render_lists")
        return ro

    def render_lists(self, offsets, weave_perm, visible_bits, value=None) -> RenderResult:
        """Host-memory call of cw_render_lists: the rendered nodes of every
        document from a weave's weave_perm (uint32, or uint16: perm16) and
        visible_bits; value: one word of 1, 2, 4 or 8 bytes per node."""
        off = _u64(offsets)
        perm = np.ascontiguousarray(weave_perm)
        if perm.dtype != np.uint16:
            perm = np.ascontiguousarray(perm, np.uint32)
        bits = np.ascontiguousarray(visible_bits, np.uint32)
        N = len(perm)
        val = _value_column(value)
        if int(off[-1]) != N or len(bits) < (N + 31) // 32 or (val is not None and len(val) != N):
            raise ValueError("offsets[-1] / weave_perm / visible_bits / value sizes differ")
        ro = np.zeros(len(off), np.uint64)
        src = np.zeros(max(N, 1), np.uint32)
        oval = None if val is None else np.zeros(max(N, 1), val.dtype)
        b = CwRenderBatch(len(off) - 1, _u64p(off), _ptr(perm), _ptr(bits),
                          int(perm.dtype == np.uint16), 0 if val is None else val.dtype.itemsize,
                          _ptr(val))
        r = CwRenderResult(_u64p(ro), _ptr(src), _ptr(oval))
        self._check(self._L.cw_render_lists(self._h, C.byref(b), C.byref(r), CW_MEM_HOST),
                    "cw_render_lists")
        R = int(ro[-1])
        return RenderResult(ro, src[:R], None if oval is None else oval[:R])

    def render_maps_device(self, n_colls, n_segs, coll_ptr, key_ptr, active_ptr, key_out_ptr=None,
                           src_ptr=None, coll_offsets=None, value_ptr=None, value_size=0,
                           out_value_ptr=None) -> np.ndarray:
        """Device-memory call of cw_render_maps: raw device pointers to seg_coll,
        seg_key, seg_active (cw_weave_maps' result), the value column and the
        outputs entry_key / entry_src / entry_value (None = NULL); coll_offsets
        (host) only with a value column.  Returns the entry offsets
        (uint64[n_colls+1])."""
        co = None if coll_offsets is None else _u64(coll_offsets)
        b = CwMapRenderBatch(n_colls, n_segs, _vp(coll_ptr), _vp(key_ptr), _vp(active_ptr),
                             _u64p(co), value_size, _vp(value_ptr))
        eo = np.zeros(n_colls + 1, np.uint64)
        r = CwMapRenderResult(_u64p(eo), _vp(key_out_ptr), _vp(src_ptr), _vp(out_value_ptr))
        self._check(self._L.cw_render_maps(self._h, C.byref(b), C.byref(r), CW_MEM_DEVICE),
                    "cw_render_maps")
        return eo

    def render_maps(self, n_colls, seg_coll, seg_key, seg_active, coll_offsets=None,
                    value=None) -> MapRenderResult:
        """Host-memory call of cw_render_maps on the seg_coll / seg_key /
        seg_active of a MapResult; value (with coll_offsets): one word of 1, 2,
        4 or 8 bytes per node, collection-local order."""
        sc = np.ascontiguousarray(seg_coll, np.uint32)
        sk = np.ascontiguousarray(seg_key, np.uint64)
        sa = np.ascontiguousarray(seg_active, np.int64)
        S = len(sc)
        if len(sk) != S or len(sa) != S:
            raise ValueError("seg_coll / seg_key / seg_active sizes differ")
        val = _value_column(value)
        co = None
        if val is not None:
            co = _u64(coll_offsets)
            if len(co) != n_colls + 1 or int(co[-1]) != len(val):
                raise ValueError("coll_offsets / value sizes")
        eo = np.zeros(n_colls + 1, np.uint64)
        key, src = np.zeros(max(S, 1), np.uint64), np.zeros(max(S, 1), np.uint32)
        oval = None if val is None else np.zeros(max(S, 1), val.dtype)
        b = CwMapRenderBatch(n_colls, S, _ptr(sc), _ptr(sk), _ptr(sa), _u64p(co),
                             0 if val is None else val.dtype.itemsize, _ptr(val))
        r = CwMapRenderResult(_u64p(eo), _ptr(key), _ptr(src), _ptr(oval))
        self._check(self._L.cw_render_maps(self._h, C.byref(b), C.byref(r), CW_MEM_HOST),
                    "cw_render_maps")
        R = int(eo[-1])
        return MapRenderResult(eo, key[:R], src[:R], None if oval is None else oval[:R])
