"""cause_amd/abi_insert.py against include/causeweave_insert.h (no GPU).

The two structs and the signature are compared with what tests/jvm_twins.py
parses out of the header (fed the main header's text first, so that the nested
typedefs resolve); drifted copies must be reported; the built library exports
the symbol; insert_lists and insert_lists_device run against a stub library in
the manner of tests/test_abi_calls.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cause_amd import abi, abi_insert
from tests import jvm_twins as J
from tests import test_abi_calls as S
from tests import test_abi_header as H

MAIN = open(abi.HEADER).read()
INSERT = open(abi_insert.HEADER).read()
NEW_STRUCTS = {"cw_insert_batch": abi_insert.CwInsertBatch, "cw_insert_result": abi_insert.CwInsertResult}
U8, U32, U64 = np.uint8, np.uint32, np.uint64


def mirror(typedef):
    return NEW_STRUCTS.get(typedef) or H.mirror(typedef)


def c_kind(text, layouts):
    base = text.split()[0]
    if text == base + " *" and base in NEW_STRUCTS:
        return NEW_STRUCTS[base]
    return H.c_kind(text, layouts)


def check_insert_abi(insert_src):
    """Problems between abi_insert.py and the header text (empty = in line)."""
    problems = []
    layouts = J.header_layouts(MAIN + "\n" + insert_src)
    new = {t: v for t, v in layouts.items() if t not in J.header_layouts(MAIN)}
    if set(new) != set(NEW_STRUCTS):
        problems.append(f"the header defines {sorted(new)}, abi_insert.py mirrors {sorted(NEW_STRUCTS)}")
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
    protos = J.header_prototypes(insert_src)
    for name in sorted(set(abi_insert.SIGNATURES) - set(protos)):
        problems.append(f"abi_insert.SIGNATURES has {name}, which the header does not declare")
    for name, (ret, params) in protos.items():
        if name not in abi_insert.SIGNATURES:
            problems.append(f"abi_insert.SIGNATURES lacks {name}")
            continue
        restype, argtypes = abi_insert.SIGNATURES[name]
        want = (c_kind(ret, layouts), [c_kind(p, layouts) for p in params])
        got = (H.ct_kind(restype), [H.ct_kind(t) for t in argtypes])
        if got != want:
            problems.append(f"{name}: abi_insert.SIGNATURES {got}, header {want}")
    return problems


def test_abi_insert_mirrors_the_header():
    assert check_insert_abi(INSERT) == []
    layouts = J.header_layouts(MAIN + "\n" + INSERT)
    assert [f for f, *_ in layouts["cw_insert_batch"][0]] == [
        "docs", "weave_perm", "visible_bits", "yarn_perm", "doc_value", "tx_offsets", "tx_id",
        "tx_cause", "tx_kind", "tx_value"]
    assert layouts["cw_insert_batch"][0][0] == ("docs", "cw_list_batch", 56, 0)
    assert layouts["cw_insert_result"][0][2] == ("weave", "cw_list_result", 48, 16)
    assert (layouts["cw_insert_batch"][1], layouts["cw_insert_result"][1]) == (128, 96)
    assert J.header_prototypes(INSERT) == {
        "cw_insert_lists": ("int", ["cw_ctx *", "cw_insert_batch *", "cw_insert_result *", "int"])}


def test_the_main_header_is_as_it_was():
    assert len(J.header_layouts(MAIN)) == 21 and len(J.header_prototypes(MAIN)) == 49
    assert "cw_insert_lists" not in abi.SIGNATURES and "cw_insert_lists" not in J.header_prototypes(MAIN)
    assert not [t for t in J.header_layouts(MAIN) if t.startswith("cw_insert")]
    assert not [n for n in dir(abi) if n.startswith("CwInsert")]


@pytest.mark.parametrize("old,new,what", [
    # a field moved, one retyped, one dropped
    ("  const uint32_t *weave_perm;   /* [N] their weave, as cw_list_result.weave_perm                     */\n"
     "  const uint32_t *visible_bits;", "  const uint32_t *visible_bits;\n  const uint32_t *weave_perm;",
     "CwInsertBatch"),
    ("const uint8_t *tx_kind; ", "uint8_t tx_kind; ", "CwInsertBatch"),
    ("  uint64_t *value;\n", "", "CwInsertResult"),
    ("  cw_list_result weave;", "  cw_list_result *weave;", "CwInsertResult"),
    # the nested batch swapped for another struct
    ("  cw_list_batch docs;", "  cw_list_batch_k128 docs;", "CwInsertBatch"),
    # a parameter dropped, a struct swapped, the function renamed, a new one
    ("cw_insert_result *result, int memspace);", "cw_insert_result *result);", "cw_insert_lists"),
    ("const cw_insert_batch *batch, cw_insert_result", "const cw_list_batch *batch, cw_insert_result",
     "cw_insert_lists"),
    ("int cw_insert_lists(", "int cw_insert_list(", "cw_insert_lists"),
    ("#ifdef __cplusplus\n}\n", "int cw_insert_maps(cw_ctx *ctx);\n#ifdef __cplusplus\n}\n",
     "lacks cw_insert_maps"),
])
def test_a_drifted_header_is_reported(old, new, what):
    assert INSERT.count(old) == 1, old
    problems = check_insert_abi(INSERT.replace(old, new))
    assert problems and any(what in p for p in problems), problems


def test_the_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    assert any(line.split()[-1] == "cw_insert_lists" and line.split()[-2] == "T"
               for line in out.splitlines() if line.strip())
    L = abi_insert.lib()
    restype, argtypes = abi_insert.SIGNATURES["cw_insert_lists"]
    assert L.cw_insert_lists.restype is restype and list(L.cw_insert_lists.argtypes) == argtypes
    assert os.path.basename(abi_insert.HEADER) == "causeweave_insert.h"


# ------------------------------------------------------------- against the stub
OFF, TOFF = [0, 20, 20, 32], [0, 2, 3, 3]  # three documents (the middle one empty); tx of 2, 1, 0
N, T, D = 32, 3, 3
NEW = np.array([0, 22, 22, 34], U64)     # what the stub answers: the second tx refused
COL_PAT = {"id_key": (U64, 500), "cause_key": (U64, 600), "kind": (U8, 7), "value": (U64, 700)}
weaver = S.weaver


def play_insert(call, m=34):
    b, r = call.snaps
    off = S.rd(b["docs"]["doc_offsets"], U64, b["docs"]["n_docs"] + 1)
    toff = S.rd(b["tx_offsets"], U64, b["docs"]["n_docs"] + 1)
    n, t = int(off[-1]), int(toff[-1])
    if call.plain == [abi.CW_MEM_HOST]:
        call.seen = {"off": off, "toff": toff, "id": S.rd(b["docs"]["id_key"], U64, n),
                     "kind": S.rd(b["docs"]["kind"], U8, n), "perm": S.rd(b["weave_perm"], U32, n),
                     "bits": S.rd(b["visible_bits"], U32, (n + 31) // 32),
                     "tx_id": S.rd(b["tx_id"], U64, t), "tx_cause": S.rd(b["tx_cause"], U64, t),
                     "tx_kind": S.rd(b["tx_kind"], U8, t)}
        for f, dt in (("yarn_perm", U32), ("doc_value", U64)):
            if b[f] is not None:
                call.seen[f] = S.rd(b[f], dt, n)
        if b["tx_value"] is not None:
            call.seen["tx_value"] = S.rd(b["tx_value"], U64, t)
        S.fill_list(r["weave"], m, (m + 31) // 32, D)
        S.wr(r["insert_pos"], np.array([5, 0xFFFFFFFF, 9], U32))
        for f in COL_PAT:
            if r[f] is not None:
                S.wr(r[f], S.pat(COL_PAT, f, m))
    S.wr(r["new_offsets"], NEW)


@pytest.mark.parametrize("yarns,values,columns", [(True, True, True), (False, False, True),
                                                   (True, False, False), (False, True, False)])
def test_insert_lists_host(weaver, yarns, values, columns):
    i, c, k = S.nodes(N)
    ti, tc, tk = (x[:T] + x.dtype.type(1) for x in S.nodes(T))
    perm = np.arange(N, dtype=U32)[::-1].copy()
    bits = np.array([0xF0F0F0F0], U32)
    yarn = np.arange(N, dtype=U32) if yarns else None
    val, tval = (np.arange(N, dtype=U64) + U64(40), np.arange(T, dtype=U64) + U64(90)) if values \
        else (None, None)
    weaver._L.play = play_insert
    res = abi_insert.insert_lists(weaver, (OFF, i, c, k), perm, bits, (TOFF, ti, tc, tk, tval), S.LAY2,
                                  yarn_perm=yarn, doc_value=val, columns=columns)
    call = S.one_call(weaver, "cw_insert_lists", abi.CW_MEM_HOST)
    assert call.types == [abi_insert.CwInsertBatch, abi_insert.CwInsertResult]
    b, r = call.snaps
    assert b["docs"]["n_docs"] == D and S.nulls(b["docs"]) == set()
    assert {f: b["docs"][f] for f in ("key_bits", "ts_shift", "site_shift", "site_bits")} == \
        {"key_bits": 40, "ts_shift": 20, "site_shift": 18, "site_bits": 2}
    assert S.nulls(b) == ({"yarn_perm"} if not yarns else set()) | \
        ({"doc_value", "tx_value"} if not values else set())
    seen = call.seen
    S.same(seen["off"], np.array(OFF, U64)), S.same(seen["toff"], np.array(TOFF, U64))
    S.same(seen["id"], i), S.same(seen["kind"], k), S.same(seen["perm"], perm), S.same(seen["bits"], bits)
    S.same(seen["tx_id"], ti), S.same(seen["tx_cause"], tc), S.same(seen["tx_kind"], tk)
    if yarns:
        S.same(seen["yarn_perm"], yarn)
    if values:
        S.same(seen["doc_value"], val), S.same(seen["tx_value"], tval)
    want_null = set() if columns else {"id_key", "cause_key", "kind"}
    if not (columns and values):
        want_null |= {"value"}
    assert S.nulls(r) == want_null
    assert S.nulls(r["weave"]) == (set() if yarns else {"yarn_perm"})
    assert isinstance(res, abi_insert.InsertResult)
    S.same(res.offsets, NEW)
    S.same(res.insert_pos, np.array([5, 0xFFFFFFFF, 9], U32))
    M = 34
    S.check_list(res.weave, M, 2, D, yarns, (N + T, 2, D))
    for f in COL_PAT:
        a = getattr(res, f)
        if f in want_null:
            assert a is None
        else:
            S.same(a, S.pat(COL_PAT, f, M))
            assert S.cap(a) == N + T


def test_insert_lists_host_checks_sizes(weaver):
    i, c, k = S.nodes(N)
    ti, tc, tk = S.nodes(T)
    perm, bits = np.arange(N, dtype=U32), np.zeros(1, U32)
    ok = dict(w=weaver, docs=(OFF, i, c, k), weave_perm=perm, visible_bits=bits, tx=(TOFF, ti, tc, tk),
              layout=S.LAY2)
    for bad in (dict(docs=(OFF, i[:5], c, k)), dict(tx=(TOFF, ti, tc[:1], tk)), dict(weave_perm=perm[:7]),
                dict(visible_bits=np.zeros(0, U32)), dict(tx=(TOFF[:3], ti, tc, tk)),
                dict(yarn_perm=perm[:3]), dict(doc_value=np.zeros(N, U64)),
                dict(tx=(TOFF, ti, tc, tk, np.zeros(T, U64))),
                dict(doc_value=np.zeros(3, U64), tx=(TOFF, ti, tc, tk, np.zeros(T, U64)))):
        with pytest.raises(ValueError):
            abi_insert.insert_lists(**{**ok, **bad})
    assert weaver._L.calls == []


@pytest.mark.parametrize("full", [True, False])
def test_insert_lists_device(weaver, full):
    weaver._L.play = play_insert
    outs = {"weave_perm": 0x1000, "visible_bits": 0x2000, "visible_count": 0x3000, "status": 0x5000}
    if full:
        outs.update(max_ts=0x4000, yarn_perm=0x6000)
    more = dict(pos_ptr=0x7000, yarn_ptr=0x8000, value_ptr=0x9000,
                col_ptrs=(0xA000, 0xB000, 0xC000, 0xD000)) if full else {}
    tx_ptrs = (0x10, 0x20, 0x30, 0x40) if full else (0x10, 0x20, 0x30)
    offs = abi_insert.insert_lists_device(weaver, OFF, (0x100, 0x200, 0x300), 0x400, 0x500, TOFF, tx_ptrs,
                                          S.LAY2, outs, **more)
    call = S.one_call(weaver, "cw_insert_lists", abi.CW_MEM_DEVICE)
    assert call.types == [abi_insert.CwInsertBatch, abi_insert.CwInsertResult]
    b, r = call.snaps
    assert (b["docs"]["id_key"], b["docs"]["cause_key"], b["docs"]["kind"]) == (0x100, 0x200, 0x300)
    assert (b["weave_perm"], b["visible_bits"]) == (0x400, 0x500)
    assert (b["tx_id"], b["tx_cause"], b["tx_kind"]) == (0x10, 0x20, 0x30)
    assert (b["yarn_perm"], b["doc_value"], b["tx_value"]) == ((0x8000, 0x9000, 0x40) if full
                                                               else (None, None, None))
    assert b["docs"]["n_docs"] == D and b["docs"]["site_bits"] == 2
    assert {f: r["weave"][f] for f in outs} == outs
    assert S.nulls(r["weave"]) == (set() if full else {"max_ts", "yarn_perm"})
    assert (r["insert_pos"], r["id_key"], r["cause_key"], r["kind"], r["value"]) == \
        ((0x7000, 0xA000, 0xB000, 0xC000, 0xD000) if full else (None,) * 5)
    S.same(offs, NEW)
    with pytest.raises(ValueError):
        abi_insert.insert_lists_device(weaver, OFF, (1, 2, 3), 4, 5, TOFF[:3], (1, 2, 3), S.LAY2, outs)


def test_an_error_return_raises_with_the_library_text(weaver):
    weaver._L.play = lambda call: -1 if call.name == "cw_insert_lists" else b"tx_offsets not monotone"
    i, c, k = S.nodes(N)
    ti, tc, tk = S.nodes(T)
    with pytest.raises(abi.WeaveError, match="cw_insert_lists: tx_offsets not monotone"):
        abi_insert.insert_lists(weaver, (OFF, i, c, k), np.arange(N, dtype=U32), np.zeros(1, U32),
                                (TOFF, ti, tc, tk), S.LAY2)


def test_ids_over_63_bits_are_refused_before_the_call():
    """cw_insert_lists has no K128 form: causal.insert_lists says so with a CauseError."""
    from cause_amd import causal as K

    site = "s" * 13
    ct = K.new_list_ct(site_id=site, uuid="u" * 21)
    with pytest.raises(K.CauseError) as e:
        K.insert_lists([(ct, ((1 << 62, site, 0), K.ROOT_ID, "a"), None)])
    assert "key-range" in e.value.causes and "63 bits" in str(e.value)
