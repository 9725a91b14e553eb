"""cause_amd/abi.py against include/causeweave.h, read as text (no GPU).

The Cw* classes and abi.SIGNATURES are hand copies of the header.  check_abi
compares them with what tests/jvm_twins.py parses out of it: for every struct
the field names, order, offsets, sizes and kinds; for every function the
restype and argtypes against the return and parameter kinds (pointer, u64,
u32, int, char *), a struct pointer against the class that mirrors the typedef.
It returns the list of problems; the tests feed it the committed header and
deliberately drifted copies.
"""
import ctypes as C

import pytest

from cause_amd import abi
from tests import jvm_twins as J

SCALARS = {"JAVA_LONG": (C.c_uint64, C.c_int64), "JAVA_INT": (C.c_uint32, C.c_int32, C.c_int),
           "JAVA_BYTE": (C.c_uint8, C.c_char), "JAVA_DOUBLE": (C.c_double,)}
C_KINDS = {"void": "void", "int": "int", "uint32_t": "u32", "uint64_t": "u64", "char *": "char *"}
CT_KINDS = {None: "void", C.c_int: "int", C.c_uint32: "u32", C.c_uint64: "u64",
            C.c_char_p: "char *", C.c_void_p: "pointer"}


def mirror(typedef):
    """cw_list_batch_k32 -> abi.CwListBatchK32 (None when abi.py has no such class)."""
    return getattr(abi, "".join(w.capitalize() for w in typedef.split("_")), None)


def is_pointer(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def field_fits(carrier, ctype):
    """Does a ctypes field type mirror a header member of this carrier?"""
    base, _, count = carrier.partition("[")
    if count:
        return (issubclass(ctype, C.Array) and ctype._length_ == int(count[:-1])
                and ctype._type_ in SCALARS[base])
    if base == "ADDRESS":
        return is_pointer(ctype)
    if base in SCALARS:
        return ctype in SCALARS[base]
    return ctype is mirror(base)  # a nested struct


def c_kind(text, layouts):
    if text in C_KINDS:
        return C_KINDS[text]
    base = text.split()[0]
    if text == base + " *" and base in layouts:
        return mirror(base) or "no class for " + base
    return "pointer" if text.endswith("*") else "?" + text


def ct_kind(t):
    if t in CT_KINDS:
        return CT_KINDS[t]
    if is_pointer(t):
        return t._type_ if issubclass(t._type_, C.Structure) else "pointer"
    return "?" + repr(t)


def check_abi(header_src):
    problems = []
    layouts = J.header_layouts(header_src)
    for typedef, (fields, size, _) in layouts.items():
        cls = mirror(typedef)
        if cls is None:
            problems.append(f"abi.py has no class for {typedef}")
            continue
        want = [(f, off, sz) for f, _, sz, off in fields]
        got = [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
        if got != want or C.sizeof(cls) != size:
            problems.append(f"{cls.__name__} = {got} ({C.sizeof(cls)} bytes) but {typedef} = {want} "
                            f"({size} bytes)")
            continue
        for (f, car, _, _), (_, ctype) in zip(fields, cls._fields_):
            if not field_fits(car, ctype):
                problems.append(f"{cls.__name__}.{f} is {ctype.__name__}, {typedef}'s is {car}")
    protos = J.header_prototypes(header_src)
    for name in sorted(set(abi.SIGNATURES) - set(protos)):
        problems.append(f"abi.SIGNATURES has {name}, which the header does not declare")
    for name, (ret, params) in protos.items():
        if name not in abi.SIGNATURES:
            problems.append(f"abi.SIGNATURES lacks {name}")
            continue
        restype, argtypes = abi.SIGNATURES[name]
        want = (c_kind(ret, layouts), [c_kind(p, layouts) for p in params])
        got = (ct_kind(restype), [ct_kind(t) for t in argtypes])
        if got != want:
            problems.append(f"{name}: abi.SIGNATURES {got}, header {want}")
    return problems


HEADER = open(abi.HEADER).read()


def test_abi_py_mirrors_the_header():
    assert check_abi(HEADER) == []


def test_the_parsers_see_every_struct_and_function():
    layouts, protos = J.header_layouts(HEADER), J.header_prototypes(HEADER)
    assert len(layouts) == 21 and len(protos) == 49
    assert set(protos) == set(abi.header_functions()) == set(abi.SIGNATURES)
    classes = {n for n in dir(abi) if n.startswith("Cw") and issubclass(getattr(abi, n), C.Structure)}
    assert {mirror(t).__name__ for t in layouts} == classes
    # the three kinds header_structs used to skip
    assert layouts["cw_kernel_stat"][0][0] == ("name", "JAVA_BYTE[48]", 48, 0)
    assert layouts["cw_merge_batch"][0][2] == ("b", "cw_list_batch", 56, 64)
    assert [f for f, *_ in layouts["cw_map_render_batch"][0]][:2] == ["n_colls", "n_segs"]
    assert [layouts[t][1] for t in ("cw_kernel_stat", "cw_map_weft_batch", "cw_map_render_batch")] \
        == [72, 72, 64]
    assert protos["cw_ctx_create"] == ("int", ["int", "cw_ctx * *"])
    assert protos["cw_last_error"] == ("char *", ["cw_ctx *"])
    assert protos["cw_ctx_destroy"][0] == "void"
    # every function has an explicit restype, None only for void
    assert [n for n, (r, _) in abi.SIGNATURES.items() if r is None] == ["cw_ctx_destroy"]


def test_lib_applies_the_table():
    L = abi.lib()
    for name, (restype, argtypes) in abi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


@pytest.mark.parametrize("old,new,what", [
    # a field moved
    ("uint32_t ts_shift;           /* lamport-ts = id_key >> ts_shift                       */\n"
     "  uint32_t site_shift;", "uint32_t site_shift;\n  uint32_t ts_shift;", "CwListBatch"),
    ("  uint32_t site_shift;     /* site rank = (id_key >> site_shift) & (2^site_bits - 1)  */\n"
     "  uint32_t site_bits;      /* 1..10",
     "  uint32_t site_bits;\n  uint32_t site_shift;      /* 1..10", "CwMapWeftBatch"),
    # a field that changes kind, inside a struct other structs nest
    ("uint64_t cap_segs;", "uint32_t cap_segs;", "CwMapResult"),
    ("  int64_t *seg_active;", "  int64_t seg_active;", "CwMapResult.seg_active"),
    ("char name[48];", "char name[40];", "CwKernelStat"),
    # a parameter dropped, one retyped, a struct swapped, a return type changed
    ("uint64_t m, uint32_t elem_size,\n", "uint64_t m,\n", "cw_gather"),
    ("uint64_t m, uint32_t base, uint32_t *out, uint32_t *status);",
     "uint64_t m, uint64_t base, uint32_t *out, uint32_t *status);", "cw_lookup_keys"),
    ("int cw_weft_maps(cw_ctx *ctx, const cw_map_weft_batch *batch",
     "int cw_weft_maps(cw_ctx *ctx, const cw_weft_batch *batch", "cw_weft_maps"),
    ("int cw_reset_kernel_stats(", "void cw_reset_kernel_stats(", "cw_reset_kernel_stats"),
    # a function abi.py does not know, and one it knows that is gone
    ("int cw_abi_version(void);", "int cw_abi_version(void);\nint cw_abi_minor(void);",
     "lacks cw_abi_minor"),
    ("int cw_scatter32(", "int cw_scatter(", "cw_scatter32"),
])
def test_a_drifted_header_is_reported(old, new, what):
    assert HEADER.count(old) == 1, old
    problems = check_abi(HEADER.replace(old, new))
    assert problems and any(what in p for p in problems), problems
