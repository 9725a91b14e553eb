"""cause_amd/abi_map_insert.py against include/causeweave_map_insert.h (no GPU).

The two structs and the signature are compared with what tests/jvm_twins.py
parses out of the header (fed the main header's text first, so that the nested
typedefs resolve); drifted copies must be reported; the built library exports
the symbol; insert_maps and insert_maps_device run against the stub library of
tests/test_abi_calls.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cause_amd import abi, abi_map_insert
from tests import jvm_twins as J
from tests import test_abi_calls as S
from tests import test_abi_header as H

MAIN = open(abi.HEADER).read()
SRC = open(abi_map_insert.HEADER).read()
NEW_STRUCTS = {"cw_map_insert_batch": abi_map_insert.CwMapInsertBatch,
               "cw_map_insert_result": abi_map_insert.CwMapInsertResult}
U8, U32, U64, I64 = np.uint8, np.uint32, np.uint64, np.int64


def c_kind(text, layouts):
    base = text.split()[0]
    if text == base + " *" and base in NEW_STRUCTS:
        return NEW_STRUCTS[base]
    return H.c_kind(text, layouts)


def check_abi(src):
    """Problems between abi_map_insert.py and the header text (empty = in line)."""
    problems = []
    layouts = J.header_layouts(MAIN + "\n" + src)
    new = {t: v for t, v in layouts.items() if t not in J.header_layouts(MAIN)}
    if set(new) != set(NEW_STRUCTS):
        problems.append(f"the header defines {sorted(new)}, abi_map_insert.py mirrors {sorted(NEW_STRUCTS)}")
    for typedef, (fields, size, _) in new.items():
        cls = NEW_STRUCTS.get(typedef)
        if cls is None:
            continue
        want = [(f, off, sz) for f, _, sz, off in fields]
        got = [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
        if got != want or C.sizeof(cls) != size:
            problems.append(f"{cls.__name__} = {got} ({C.sizeof(cls)} bytes) but {typedef} = {want} "
                            f"({size} bytes)")
            continue
        for (f, car, _, _), (_, ctype) in zip(fields, cls._fields_):
            if not H.field_fits(car, ctype):
                problems.append(f"{cls.__name__}.{f} is {ctype.__name__}, {typedef}'s is {car}")
    protos = J.header_prototypes(src)
    for name in sorted(set(abi_map_insert.SIGNATURES) - set(protos)):
        problems.append(f"abi_map_insert.SIGNATURES has {name}, which the header does not declare")
    for name, (ret, params) in protos.items():
        if name not in abi_map_insert.SIGNATURES:
            problems.append(f"abi_map_insert.SIGNATURES lacks {name}")
            continue
        restype, argtypes = abi_map_insert.SIGNATURES[name]
        want = (c_kind(ret, layouts), [c_kind(p, layouts) for p in params])
        got = (H.ct_kind(restype), [H.ct_kind(t) for t in argtypes])
        if got != want:
            problems.append(f"{name}: abi_map_insert.SIGNATURES {got}, header {want}")
    return problems


def test_abi_map_insert_mirrors_the_header():
    assert check_abi(SRC) == []
    layouts = J.header_layouts(MAIN + "\n" + SRC)
    assert [f for f, *_ in layouts["cw_map_insert_batch"][0]] == [
        "colls", "n_segs", "seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm", "coll_value",
        "tx_offsets", "tx_id", "tx_cause", "tx_cause_is_id", "tx_kind", "tx_value"]
    assert [f for f, *_ in layouts["cw_map_insert_result"][0]] == [
        "new_offsets", "tx_seg", "tx_pos", "maps", "id_key", "cause", "cause_is_id", "kind", "value"]
    assert layouts["cw_map_insert_batch"][0][0][:2] == ("colls", "cw_map_batch")
    assert layouts["cw_map_insert_result"][0][3][:2] == ("maps", "cw_map_result")
    assert J.header_prototypes(SRC) == {
        "cw_insert_maps": ("int", ["cw_ctx *", "cw_map_insert_batch *", "cw_map_insert_result *", "int"])}


def test_the_other_headers_are_as_they_were():
    assert len(J.header_layouts(MAIN)) == 21 and len(J.header_prototypes(MAIN)) == 49
    assert "cw_insert_maps" not in abi.SIGNATURES and "cw_insert_maps" not in J.header_prototypes(MAIN)
    assert not [t for t in J.header_layouts(MAIN) if t.startswith("cw_map_insert")]


@pytest.mark.parametrize("old,new,what", [
    ("  const uint64_t *seg_key;       /* [n_segs] */\n  const int64_t  *seg_active;    /* [n_segs] */\n",
     "  const int64_t  *seg_active;    /* [n_segs] */\n  const uint64_t *seg_key;       /* [n_segs] */\n",
     "CwMapInsertBatch"),
    ("  uint64_t n_segs;  ", "  uint32_t n_segs;  ", "CwMapInsertBatch"),
    ("  uint32_t *tx_pos; ", "  uint64_t tx_pos[2]; ", "CwMapInsertResult"),
    ("  cw_map_result maps; ", "  cw_map_result *maps; ", "CwMapInsertResult"),
    ("  cw_map_batch colls; ", "  cw_list_batch colls; ", "CwMapInsertBatch"),
    ("cw_map_insert_result *result, int memspace);", "cw_map_insert_result *result);", "cw_insert_maps"),
    ("int cw_insert_maps(", "int cw_insert_map(", "cw_insert_maps"),
    ("#ifdef __cplusplus\n}\n", "int cw_insert_sets(cw_ctx *ctx);\n#ifdef __cplusplus\n}\n",
     "lacks cw_insert_sets"),
])
def test_a_drifted_header_is_reported(old, new, what):
    assert SRC.count(old) == 1, old
    problems = check_abi(SRC.replace(old, new))
    assert problems and any(what in p for p in problems), problems


def test_the_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    assert any(line.split()[-1] == "cw_insert_maps" and line.split()[-2] == "T"
               for line in out.splitlines() if line.strip())
    L = abi_map_insert.lib()
    restype, argtypes = abi_map_insert.SIGNATURES["cw_insert_maps"]
    assert L.cw_insert_maps.restype is restype and list(L.cw_insert_maps.argtypes) == argtypes
    assert os.path.basename(abi_map_insert.HEADER) == "causeweave_map_insert.h"


# ------------------------------------------------------------- against the stub
OFF, TOFF = [0, 4, 4, 6], [0, 2, 3, 3]
N, T, D, NSEG = 6, 3, 3, 2
NEW = np.array([0, 6, 6, 8], U64)
weaver = S.weaver


def inputs():
    cols = (np.arange(N, dtype=U64) + U64(10), np.arange(N, dtype=U64), np.zeros(N, U8), np.zeros(N, U8))
    segs = (np.array([0, 5, 8], U64), np.array([0, 2], U32), np.array([1, 3], U64), np.array([0, 1], I64),
            np.arange(N + NSEG, dtype=U32))
    tx = (np.arange(T, dtype=U64) + U64(90), np.arange(T, dtype=U64), np.zeros(T, U8), np.ones(T, U8))
    return cols, segs, tx


def play(call):
    b, r = call.snaps
    if call.plain == [abi.CW_MEM_HOST]:
        call.seen = {"off": S.rd(b["colls"]["coll_offsets"], U64, D + 1), "toff": S.rd(b["tx_offsets"], U64, D + 1),
                     "seg_key": S.rd(b["seg_key"], U64, NSEG), "seg_perm": S.rd(b["seg_perm"], U32, N + NSEG),
                     "tx_kind": S.rd(b["tx_kind"], U8, T)}
        S.wr(r["tx_seg"], np.array([0, 1, 0xFFFFFFFF], U32))
        S.wr(r["maps"]["seg_key"], np.array([1, 2, 3], U64))
    S.wr(r["new_offsets"], NEW)


@pytest.mark.parametrize("values,columns", [(True, True), (False, True), (True, False)])
def test_insert_maps_host(weaver, values, columns):
    cols, segs, tx = inputs()
    val, tval = (np.arange(N, dtype=U64), np.arange(T, dtype=U64)) if values else (None, None)
    weaver._L.play = play
    res = abi_map_insert.insert_maps(weaver, (OFF,) + cols, segs, (TOFF,) + tx + (tval,), coll_value=val,
                                     columns=columns)
    call = S.one_call(weaver, "cw_insert_maps", abi.CW_MEM_HOST)
    assert call.types == [abi_map_insert.CwMapInsertBatch, abi_map_insert.CwMapInsertResult]
    b, r = call.snaps
    assert b["colls"]["n_colls"] == D and b["n_segs"] == NSEG and r["maps"]["cap_segs"] == NSEG + T
    assert S.nulls(b) == (set() if values else {"coll_value", "tx_value"})
    S.same(call.seen["off"], np.array(OFF, U64)), S.same(call.seen["toff"], np.array(TOFF, U64))
    S.same(call.seen["seg_key"], segs[2]), S.same(call.seen["seg_perm"], segs[4])
    S.same(call.seen["tx_kind"], tx[3])
    want_null = set() if columns else {"id_key", "cause", "cause_is_id", "kind"}
    if not (columns and values):
        want_null |= {"value"}
    assert S.nulls(r) == want_null and S.nulls(r["maps"]) == set()
    assert isinstance(res, abi_map_insert.MapInsertResult)
    S.same(res.offsets, NEW)
    S.same(res.tx_seg, np.array([0, 1, 0xFFFFFFFF], U32))
    assert (res.id_key is None) == (not columns) and (res.value is None) == (not (columns and values))
    if columns:
        assert len(res.id_key) == 8 and len(res.cause_is_id) == 8


def test_insert_maps_host_checks_sizes(weaver):
    cols, segs, tx = inputs()
    ok = dict(w=weaver, colls=(OFF,) + cols, segs=segs, tx=(TOFF,) + tx)
    for bad in (dict(colls=(OFF, cols[0][:3]) + cols[1:]), dict(tx=(TOFF, tx[0], tx[1][:1]) + tx[2:]),
                dict(tx=(TOFF[:3],) + tx), dict(segs=(segs[0][:2],) + segs[1:]),
                dict(segs=segs[:4] + (segs[4][:5],)), dict(segs=segs[:2] + (segs[2][:1],) + segs[3:]),
                dict(coll_value=np.zeros(N, U64)), dict(tx=(TOFF,) + tx + (np.zeros(T, U64),)),
                dict(coll_value=np.zeros(2, U64), tx=(TOFF,) + tx + (np.zeros(T, U64),))):
        with pytest.raises(ValueError):
            abi_map_insert.insert_maps(**{**ok, **bad})
    assert weaver._L.calls == []


@pytest.mark.parametrize("full", [True, False])
def test_insert_maps_device(weaver, full):
    weaver._L.play = play
    outs = {"seg_offsets": 0x1000, "seg_coll": 0x2000, "seg_key": 0x3000, "seg_active": 0x4000,
            "seg_perm": 0x5000, "status": 0x6000}
    more = dict(tx_seg_ptr=0x7000, tx_pos_ptr=0x7100, value_ptr=0x9000,
                col_ptrs=(0xA000, 0xB000, 0xC000, 0xD000, 0xE000)) if full else {}
    tx_ptrs = (0x10, 0x20, 0x30, 0x40, 0x50) if full else (0x10, 0x20, 0x30, 0x40)
    offs, ns = abi_map_insert.insert_maps_device(weaver, OFF, (0x100, 0x200, 0x300, 0x400), NSEG,
                                                 (0x510, 0x520, 0x530, 0x540, 0x550), TOFF, tx_ptrs, outs, 9, **more)
    call = S.one_call(weaver, "cw_insert_maps", abi.CW_MEM_DEVICE)
    b, r = call.snaps
    assert (b["colls"]["id_key"], b["colls"]["cause"], b["colls"]["cause_is_id"], b["colls"]["kind"]) == \
        (0x100, 0x200, 0x300, 0x400)
    assert [b[f] for f in ("seg_offsets", "seg_coll", "seg_key", "seg_active", "seg_perm")] == \
        [0x510, 0x520, 0x530, 0x540, 0x550]
    assert [b[f] for f in ("tx_id", "tx_cause", "tx_cause_is_id", "tx_kind")] == [0x10, 0x20, 0x30, 0x40]
    assert (b["coll_value"], b["tx_value"]) == ((0x9000, 0x50) if full else (None, None))
    assert b["n_segs"] == NSEG and r["maps"]["cap_segs"] == 9
    assert {f: r["maps"][f] for f in outs} == outs
    assert [r[f] for f in ("tx_seg", "tx_pos", "id_key", "cause", "cause_is_id", "kind", "value")] == \
        ([0x7000, 0x7100, 0xA000, 0xB000, 0xC000, 0xD000, 0xE000] if full else [None] * 7)
    S.same(offs, NEW)
    with pytest.raises(ValueError):
        abi_map_insert.insert_maps_device(weaver, OFF, (1, 2, 3, 4), 0, (1, 2, 3, 4, 5), TOFF[:3], (1, 2, 3, 4),
                                          outs, 9)


def test_an_error_return_raises_with_the_library_text(weaver):
    weaver._L.play = lambda call: -1 if call.name == "cw_insert_maps" else b"tx_offsets not monotone"
    cols, segs, tx = inputs()
    with pytest.raises(abi.WeaveError, match="cw_insert_maps: tx_offsets not monotone"):
        abi_map_insert.insert_maps(weaver, (OFF,) + cols, segs, (TOFF,) + tx)
