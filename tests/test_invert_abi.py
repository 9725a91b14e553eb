"""cause_amd/abi_invert.py against include/causeweave_invert.h (no GPU).

The two structs and the signature are compared with what tests/jvm_twins.py
parses out of the header (fed the main header's text first, so that its
typedefs resolve); drifted copies must be reported; the built library exports
the symbol; invert and invert_device run against the stub library of
tests/test_abi_calls.py.
"""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest

from cause_amd import abi, abi_invert
from tests import jvm_twins as J
from tests import test_abi_calls as S
from tests import test_abi_header as H

MAIN = open(abi.HEADER).read()
SRC = open(abi_invert.HEADER).read()
NEW_STRUCTS = {"cw_invert_batch": abi_invert.CwInvertBatch, "cw_invert_result": abi_invert.CwInvertResult}
U8, U32, U64 = np.uint8, np.uint32, np.uint64


def c_kind(text, layouts):
    base = text.split()[0]
    if text == base + " *" and base in NEW_STRUCTS:
        return NEW_STRUCTS[base]
    return H.c_kind(text, layouts)


def check_abi(src):
    """Problems between abi_invert.py and the header text (empty = in line)."""
    problems = []
    layouts = J.header_layouts(MAIN + "\n" + src)
    new = {t: v for t, v in layouts.items() if t not in J.header_layouts(MAIN)}
    if set(new) != set(NEW_STRUCTS):
        problems.append(f"the header defines {sorted(new)}, abi_invert.py mirrors {sorted(NEW_STRUCTS)}")
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
    for name in sorted(set(abi_invert.SIGNATURES) - set(protos)):
        problems.append(f"abi_invert.SIGNATURES has {name}, which the header does not declare")
    for name, (ret, params) in protos.items():
        if name not in abi_invert.SIGNATURES:
            problems.append(f"abi_invert.SIGNATURES lacks {name}")
            continue
        restype, argtypes = abi_invert.SIGNATURES[name]
        want = (c_kind(ret, layouts), [c_kind(p, layouts) for p in params])
        got = (H.ct_kind(restype), [H.ct_kind(t) for t in argtypes])
        if got != want:
            problems.append(f"{name}: abi_invert.SIGNATURES {got}, header {want}")
    return problems


def test_abi_invert_mirrors_the_header():
    assert check_abi(SRC) == []
    layouts = J.header_layouts(MAIN + "\n" + SRC)
    assert [f for f, *_ in layouts["cw_invert_batch"][0]] == [
        "n_docs", "doc_offsets", "id_key", "cause", "kind", "cause_is_id", "ref_doc", "ts_shift", "site_shift",
        "site_bits", "reserved", "n_bases", "base_offsets", "sel_lo", "sel_hi", "sel_sites", "new_tx"]
    assert [f for f, *_ in layouts["cw_invert_result"][0]] == [
        "part_offsets", "inv_id", "inv_cause", "inv_cause_is_id", "inv_kind", "inv_src", "base_parts", "status"]
    assert J.header_prototypes(SRC) == {
        "cw_invert": ("int", ["cw_ctx *", "cw_invert_batch *", "cw_invert_result *", "int"])}


def test_the_main_header_is_as_it_was():
    assert "cw_invert" not in abi.SIGNATURES and "cw_invert" not in J.header_prototypes(MAIN)
    assert not [t for t in J.header_layouts(MAIN) if t.startswith("cw_invert")]


@pytest.mark.parametrize("old,new,what", [
    ("  const uint64_t *sel_lo;        /* [n_bases] */\n  const uint64_t *sel_hi;        /* [n_bases] */\n",
     "  const uint64_t *sel_hi;        /* [n_bases] */\n  const uint64_t *sel_lo;        /* [n_bases] */\n",
     "CwInvertBatch"),
    ("  uint64_t n_bases;\n", "  uint32_t n_bases;\n", "CwInvertBatch"),
    ("  uint32_t reserved;  ", "  uint64_t reserved;  ", "CwInvertBatch"),
    ("  uint32_t *inv_src;  ", "  uint32_t inv_src[4];  ", "CwInvertResult"),
    ("  uint64_t *part_offsets;  ", "  uint32_t part_offsets;  ", "CwInvertResult"),
    ("cw_invert_result *result, int memspace);", "cw_invert_result *result);", "cw_invert"),
    ("int cw_invert(", "int cw_inverse(", "cw_invert"),
    ("#ifdef __cplusplus\n}\n", "int cw_undo(cw_ctx *ctx);\n#ifdef __cplusplus\n}\n", "lacks cw_undo"),
])
def test_a_drifted_header_is_reported(old, new, what):
    assert SRC.count(old) == 1, old
    problems = check_abi(SRC.replace(old, new))
    assert problems and any(what in p for p in problems), problems


def test_the_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    assert any(line.split()[-1] == "cw_invert" and line.split()[-2] == "T"
               for line in out.splitlines() if line.strip())
    L = abi_invert.lib()
    restype, argtypes = abi_invert.SIGNATURES["cw_invert"]
    assert L.cw_invert.restype is restype and list(L.cw_invert.argtypes) == argtypes
    assert os.path.basename(abi_invert.HEADER) == "causeweave_invert.h"


# ------------------------------------------------------------- against the stub
OFF, BOFF = [0, 4, 4, 6], [0, 2, 3]
N, D, G, P = 6, 3, 2, 3
LAY = NS(ts_shift=20, site_shift=18, site_bits=7)     # 128 site ranks: two mask words a base
PO = np.array([0, 2, 2, 3], U64)
weaver = S.weaver


def inputs():
    cols = (np.arange(N, dtype=U64) + U64(10), np.arange(N, dtype=U64), (np.arange(N) % 4).astype(U8))
    sel = (np.array([1, 2], U64), np.array([8, 9], U64), np.arange(4, dtype=U64) + U64(50),
           np.array([100, 200], U64))
    return cols, np.ones(N, U8), np.full(N, 0xFFFFFFFF, U32), sel


def play(call):
    b, r = call.snaps
    if call.plain == [abi.CW_MEM_HOST]:
        call.seen = {"off": S.rd(b["doc_offsets"], U64, D + 1), "boff": S.rd(b["base_offsets"], U64, G + 1),
                     "kind": S.rd(b["kind"], U8, N), "sites": S.rd(b["sel_sites"], U64, 4),
                     "new_tx": S.rd(b["new_tx"], U64, G)}
        S.wr(r["inv_id"], np.array([100, 101, 200], U64))
        S.wr(r["inv_kind"], np.array([2, 3, 2], U8))
        S.wr(r["inv_src"], np.array([3, 0, 1], U32))
        S.wr(r["base_parts"], np.array([2, 1], U32))
        S.wr(r["status"], np.array([0, 0, 128], U32))
    S.wr(r["part_offsets"], PO)


@pytest.mark.parametrize("maps,refs", [(True, True), (False, True), (True, False)])
def test_invert_host(weaver, maps, refs):
    cols, cii, ref, sel = inputs()
    weaver._L.play = play
    res = abi_invert.invert(weaver, OFF, *cols, cii if maps else None, ref if refs else None, LAY, BOFF, *sel)
    call = S.one_call(weaver, "cw_invert", abi.CW_MEM_HOST)
    assert call.types == [abi_invert.CwInvertBatch, abi_invert.CwInvertResult]
    b, r = call.snaps
    assert (b["n_docs"], b["n_bases"], b["ts_shift"], b["site_shift"], b["site_bits"], b["reserved"]) == \
        (D, G, 20, 18, 7, 0)
    assert S.nulls(b) == ({"cause_is_id"} if not maps else set()) | ({"ref_doc"} if not refs else set())
    assert S.nulls(r) == ({"inv_cause_is_id"} if not maps else set())
    S.same(call.seen["off"], np.array(OFF, U64)), S.same(call.seen["boff"], np.array(BOFF, U64))
    S.same(call.seen["kind"], cols[2]), S.same(call.seen["sites"], sel[2]), S.same(call.seen["new_tx"], sel[3])
    assert isinstance(res, abi_invert.InvertResult)
    S.same(res.part_offsets, PO)
    S.same(res.inv_id, np.array([100, 101, 200], U64)), S.same(res.inv_kind, np.array([2, 3, 2], U8))
    S.same(res.inv_src, np.array([3, 0, 1], U32)), S.same(res.base_parts, np.array([2, 1], U32))
    S.same(res.status, np.array([0, 0, 128], U32))
    assert (res.inv_cause_is_id is None) == (not maps) and len(res.inv_cause) == P
    assert S.cap(res.inv_id) == N and S.cap(res.inv_src) == N      # sized for N


def test_invert_host_checks_sizes(weaver):
    cols, cii, ref, sel = inputs()
    ok = [OFF, cols[0], cols[1], cols[2], cii, ref, LAY, BOFF, sel[0], sel[1], sel[2], sel[3]]
    for at, bad in ((1, cols[0][:3]), (3, cols[2][:5]), (4, cii[:2]), (5, ref[:1]), (8, sel[0][:1]),
                    (10, sel[2][:2]), (11, sel[3][:1]), (0, [0, 4, 4, 5]), (0, []), (7, [])):
        args = list(ok)
        args[at] = bad
        with pytest.raises(ValueError):
            abi_invert.invert(weaver, *args)
    assert weaver._L.calls == []


@pytest.mark.parametrize("full", [True, False])
def test_invert_device(weaver, full):
    weaver._L.play = play
    outs = {"inv_id": 0x1000, "inv_cause": 0x2000, "inv_kind": 0x3000, "status": 0x4000}
    more = {}
    if full:
        outs.update(inv_cause_is_id=0x5000, inv_src=0x6000, base_parts=0x7000)
        more = dict(cause_is_id_ptr=0x400, ref_doc_ptr=0x500)
    po = abi_invert.invert_device(weaver, OFF, (0x100, 0x200, 0x300), LAY, BOFF, (0x10, 0x20, 0x30, 0x40), outs,
                                  **more)
    call = S.one_call(weaver, "cw_invert", abi.CW_MEM_DEVICE)
    b, r = call.snaps
    assert (b["id_key"], b["cause"], b["kind"]) == (0x100, 0x200, 0x300)
    assert (b["cause_is_id"], b["ref_doc"]) == ((0x400, 0x500) if full else (None, None))
    assert [b[f] for f in ("sel_lo", "sel_hi", "sel_sites", "new_tx")] == [0x10, 0x20, 0x30, 0x40]
    assert (b["n_docs"], b["n_bases"], b["site_bits"]) == (D, G, 7)
    assert {f: r[f] for f in outs} == outs
    assert S.nulls(r) == (set() if full else {"inv_cause_is_id", "inv_src", "base_parts"})
    S.same(po, PO)
    with pytest.raises(ValueError):
        abi_invert.invert_device(weaver, [], (1, 2, 3), LAY, BOFF, (1, 2, 3, 4), outs)


def test_an_error_return_raises_with_the_library_text(weaver):
    weaver._L.play = lambda call: -1 if call.name == "cw_invert" else b"base_offsets not monotone"
    cols, cii, ref, sel = inputs()
    with pytest.raises(abi.WeaveError, match="cw_invert: base_offsets not monotone"):
        abi_invert.invert(weaver, OFF, *cols, cii, ref, LAY, BOFF, *sel)
