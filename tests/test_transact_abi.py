"""cause_amd/abi_transact.py against include/causeweave_transact.h (no GPU).

The two structs and the signature are compared with what tests/jvm_twins.py
parses out of the header (fed the main header's text first, so that its
typedefs resolve); drifted copies must be reported; the main header is as it
was; the built library exports the symbol; transact and transact_device run
against the stub library of tests/test_abi_calls.py.
"""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest

from cause_amd import abi, abi_transact as A
from tests import jvm_twins as J
from tests import test_abi_calls as S
from tests import test_abi_header as H

MAIN = open(abi.HEADER).read()
SRC = open(A.HEADER).read()
NEW_STRUCTS = {"cw_transact_batch": A.CwTransactBatch, "cw_transact_result": A.CwTransactResult}
U8, U32, U64 = np.uint8, np.uint32, np.uint64


def c_kind(text, layouts):
    base = text.split()[0]
    if text == base + " *" and base in NEW_STRUCTS:
        return NEW_STRUCTS[base]
    return H.c_kind(text, layouts)


def check_abi(src):
    """Problems between abi_transact.py and the header text (empty = in line)."""
    problems = []
    layouts = J.header_layouts(MAIN + "\n" + src)
    new = {t: v for t, v in layouts.items() if t not in J.header_layouts(MAIN)}
    if set(new) != set(NEW_STRUCTS):
        problems.append(f"the header defines {sorted(new)}, abi_transact.py mirrors {sorted(NEW_STRUCTS)}")
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
    for name in sorted(set(A.SIGNATURES) - set(protos)):
        problems.append(f"abi_transact.SIGNATURES has {name}, which the header does not declare")
    for name, (ret, params) in protos.items():
        if name not in A.SIGNATURES:
            problems.append(f"abi_transact.SIGNATURES lacks {name}")
            continue
        restype, argtypes = A.SIGNATURES[name]
        want = (c_kind(ret, layouts), [c_kind(p, layouts) for p in params])
        got = (H.ct_kind(restype), [H.ct_kind(t) for t in argtypes])
        if got != want:
            problems.append(f"{name}: abi_transact.SIGNATURES {got}, header {want}")
    return problems


def test_abi_transact_mirrors_the_header():
    assert check_abi(SRC) == []
    layouts = J.header_layouts(MAIN + "\n" + SRC)
    assert [f for f, *_ in layouts["cw_transact_batch"][0]] == [f for f, _ in A.CwTransactBatch._fields_] == [
        "n_docs", "base_doc_offsets", "doc_is_map", "ts_shift", "site_shift", "site_bits", "reserved", "n_bases",
        "new_tx", "tok_offsets", "tok_kind", "tok_arg", "tok_cause", "tok_cause_is_id", "tok_vkind"]
    assert [f for f, *_ in layouts["cw_transact_result"][0]] == [
        "new_cap", "node_cap", "base_new_offsets", "base_node_offsets", "node_offsets", "node_id", "node_cause",
        "node_cause_is_id", "node_kind", "node_src", "node_sub", "node_ref", "node_run", "new_is_map", "new_open",
        "root_doc", "base_status"]
    assert J.header_prototypes(SRC) == {
        "cw_transact": ("int", ["cw_ctx *", "cw_transact_batch *", "cw_transact_result *", "int"])}
    # the column tables name the result's node and collection arrays, in its order
    assert [f for f, _ in A.NODE_COLUMNS + A.NEW_COLUMNS] == [f for f, _ in A.CwTransactResult._fields_[5:15]]


def test_the_constants_are_the_headers():
    consts = J.header_constants(SRC)
    assert consts["CW_STATUS_TX_MALFORMED"] == A.STATUS_TX_MALFORMED == 1 << 10
    names = ("CW_TX_LEAF", "CW_TX_STR", "CW_TX_OPEN_LIST", "CW_TX_OPEN_MAP", "CW_TX_CLOSE", "CW_TX_PART",
             "CW_TX_ROOT_LIST", "CW_TX_ROOT_MAP")
    assert [consts[n] for n in names] == list(range(8)) == [
        A.TX_LEAF, A.TX_STR, A.TX_OPEN_LIST, A.TX_OPEN_MAP, A.TX_CLOSE, A.TX_PART, A.TX_ROOT_LIST, A.TX_ROOT_MAP]
    main = J.header_constants(MAIN)
    assert A.STATUS_TX_MALFORMED not in [v for k, v in main.items() if k.startswith("CW_STATUS_")]
    assert main["CW_STATUS_KEY_RANGE"] == abi.STATUS_KEY_RANGE


def test_the_main_header_is_as_it_was():
    assert "cw_transact" not in abi.SIGNATURES and "cw_transact" not in J.header_prototypes(MAIN)
    assert not [t for t in J.header_layouts(MAIN) if t.startswith("cw_transact")]
    assert "TX_MALFORMED" not in MAIN and "CW_TX_" not in MAIN


@pytest.mark.parametrize("old,new,what", [
    ("  uint8_t  *node_kind;  ", "  uint32_t *node_src2;  ", "CwTransactResult"),
    ("  uint64_t n_bases;\n", "  uint32_t n_bases;\n", "CwTransactBatch"),
    ("  const uint32_t *tok_arg;  ", "  uint32_t tok_arg;  ", "CwTransactBatch"),
    ("  uint32_t *new_open;  ", "  uint32_t new_open[2];  ", "CwTransactResult"),
    ("  uint64_t *node_offsets;  ", "  uint32_t node_offsets;  ", "CwTransactResult"),
    ("  uint64_t node_cap;  ", "  uint32_t node_cap;  ", "CwTransactResult"),
    ("  uint32_t reserved;  ", "", "CwTransactBatch"),
    ("cw_transact_result *result, int memspace);", "cw_transact_result *result);", "cw_transact"),
    ("int cw_transact(", "int cw_transacts(", "cw_transact"),
    ("#ifdef __cplusplus\n}\n", "int cw_transact_apply(cw_ctx *ctx);\n#ifdef __cplusplus\n}\n", "lacks cw_transact_apply"),
])
def test_a_drifted_header_is_reported(old, new, what):
    assert SRC.count(old) == 1, old
    problems = check_abi(SRC.replace(old, new))
    assert problems and any(what in p for p in problems), problems


def test_the_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    assert any(line.split()[-1] == "cw_transact" and line.split()[-2] == "T"
               for line in out.splitlines() if line.strip())
    L = A.lib()
    restype, argtypes = A.SIGNATURES["cw_transact"]
    assert L.cw_transact.restype is restype and list(L.cw_transact.argtypes) == argtypes
    assert os.path.basename(A.HEADER) == "causeweave_transact.h"


# ------------------------------------------------------------- against the stub
LAY = NS(key_bits=40, ts_shift=20, site_shift=18, site_bits=2)
DOFF, ISM, NTX, TOFF = [0, 2, 3], [0, 1, 1], [1 << 20, 2 << 20], [0, 4, 6]
KIND, ARG = [6, 0, 1, 4, 5, 4], [0, 0, 3, 0, 2, 0]
CAUSE, CII, VK = [0, 0, 0, 0, 9, 0], [1, 1, 1, 0, 1, 0], [0, 2, 0, 0, 0, 0]
G, D, T, CN, MN = 2, 3, 6, 1, 5
BN, BM = np.array([0, 1, 1], U64), np.array([0, 5, 5], U64)
NO = np.array([0, 0, 0, 0, 5], U64)
weaver = S.weaver


def pattern(f, dt, n):
    return (np.arange(n) + 7 * len(f)).astype(dt)


def play(call):
    b, r = call.snaps
    if call.plain == [abi.CW_MEM_HOST]:
        call.seen = {"doff": S.rd(b["base_doc_offsets"], U64, G + 1), "toff": S.rd(b["tok_offsets"], U64, G + 1),
                     "ism": S.rd(b["doc_is_map"], U8, D), "ntx": S.rd(b["new_tx"], U64, G),
                     "kind": S.rd(b["tok_kind"], U8, T), "arg": S.rd(b["tok_arg"], U32, T),
                     "cause": S.rd(b["tok_cause"], U64, T), "cii": S.rd(b["tok_cause_is_id"], U8, T),
                     "vk": None if b["tok_vkind"] is None else S.rd(b["tok_vkind"], U8, T)}
        if r["node_id"] is not None:
            for f, dt in A.NODE_COLUMNS:
                S.wr(r[f], pattern(f, dt, MN))
            for f, dt in A.NEW_COLUMNS:
                S.wr(r[f], pattern(f, dt, CN))
        S.wr(r["root_doc"], np.array([3, 0xFFFFFFFF], U32))
        S.wr(r["base_status"], np.array([0, 1024], U32))
    S.wr(r["base_new_offsets"], BN)
    S.wr(r["base_node_offsets"], BM)
    S.wr(r["node_offsets"], NO[:D + min(CN, r["new_cap"]) + 1])


@pytest.mark.parametrize("nodes,vkind", [(True, True), (True, False), (False, True)])
def test_transact_host(weaver, nodes, vkind):
    weaver._L.play = play
    res = A.transact(weaver, DOFF, ISM, LAY, NTX, TOFF, KIND, ARG, CAUSE, CII, VK if vkind else None, new_cap=3,
                     node_cap=8, nodes=nodes)
    call = S.one_call(weaver, "cw_transact", abi.CW_MEM_HOST)
    assert call.types == [A.CwTransactBatch, A.CwTransactResult]
    b, r = call.snaps
    assert (b["n_docs"], b["n_bases"], b["ts_shift"], b["site_shift"], b["site_bits"], b["reserved"]) == (D, G, 20, 18, 2, 0)
    assert (r["new_cap"], r["node_cap"]) == (3, 8)
    assert S.nulls(b) == (set() if vkind else {"tok_vkind"})
    assert S.nulls(r) == (set() if nodes else {f for f, _ in A.NODE_COLUMNS + A.NEW_COLUMNS})
    for k, want, dt in (("doff", DOFF, U64), ("toff", TOFF, U64), ("ism", ISM, U8), ("ntx", NTX, U64), ("kind", KIND, U8),
                        ("arg", ARG, U32), ("cause", CAUSE, U64), ("cii", CII, U8)):
        S.same(call.seen[k], np.array(want, dt))
    assert (call.seen["vk"] is None) == (not vkind)
    assert isinstance(res, A.TransactResult)
    S.same(res.base_new_offsets, BN), S.same(res.base_node_offsets, BM), S.same(res.node_offsets, NO)
    S.same(res.root_doc, np.array([3, 0xFFFFFFFF], U32)), S.same(res.base_status, np.array([0, 1024], U32))
    assert S.cap(res.node_offsets) == D + 3 + 1
    for f, dt in A.NODE_COLUMNS:
        if nodes:
            S.same(getattr(res, f), pattern(f, dt, MN))
            assert S.cap(getattr(res, f)) == 8
        else:
            assert getattr(res, f) is None
    for f, dt in A.NEW_COLUMNS:
        if nodes:
            S.same(getattr(res, f), pattern(f, dt, CN))
            assert S.cap(getattr(res, f)) == 3
        else:
            assert getattr(res, f) is None


def test_transact_host_sizes_its_arrays_from_a_count_only_call(weaver):
    weaver._L.play = play
    res = A.transact(weaver, DOFF, ISM, LAY, NTX, TOFF, KIND, ARG, CAUSE, CII, VK)
    counts, full = weaver._L.calls
    assert counts.name == full.name == "cw_transact"
    assert S.nulls(counts.snaps[1]) == {f for f, _ in A.NODE_COLUMNS + A.NEW_COLUMNS} and S.nulls(full.snaps[1]) == set()
    assert (counts.snaps[1]["new_cap"], full.snaps[1]["new_cap"], full.snaps[1]["node_cap"]) == (T, CN, MN)
    S.same(res.node_id, pattern("node_id", U64, MN)), S.same(res.node_offsets, NO)


def test_transact_host_checks_sizes(weaver):
    for doff, toff, kind, ntx in (([0, 2, 4], TOFF, KIND, NTX), (DOFF, [0, 4, 7], KIND, NTX), ([], [], KIND, NTX),
                                  (DOFF, TOFF, KIND[:5], NTX), (DOFF, TOFF[:2], KIND, NTX), (DOFF, TOFF, KIND, NTX[:1])):
        with pytest.raises(ValueError):
            A.transact(weaver, doff, ISM, LAY, ntx, toff, kind, ARG, CAUSE, CII, VK, new_cap=3, node_cap=8)
    assert weaver._L.calls == []


@pytest.mark.parametrize("full", [True, False])
def test_transact_device(weaver, full):
    weaver._L.play = play
    outs = {"root_doc": 0x4000, "base_status": 0x5000}
    if full:
        outs.update({f: 0x10000 * (k + 1) for k, (f, _) in enumerate(A.NODE_COLUMNS + A.NEW_COLUMNS)})
    bn, bm, no = A.transact_device(weaver, DOFF, 0x100, LAY, 0x200, TOFF, (0x300, 0x400, 0x500, 0x600, None), 3, 8, outs)
    call = S.one_call(weaver, "cw_transact", abi.CW_MEM_DEVICE)
    b, r = call.snaps
    assert (b["doc_is_map"], b["new_tx"], b["tok_kind"], b["tok_arg"], b["tok_cause"], b["tok_cause_is_id"],
            b["tok_vkind"]) == (0x100, 0x200, 0x300, 0x400, 0x500, 0x600, None)
    assert (b["n_docs"], b["n_bases"], r["new_cap"], r["node_cap"]) == (D, G, 3, 8)
    assert {f: r[f] for f in outs} == outs
    assert S.nulls(r) == (set() if full else {f for f, _ in A.NODE_COLUMNS + A.NEW_COLUMNS})
    S.same(bn, BN), S.same(bm, BM), S.same(no[:D + CN + 1], NO)
    assert len(no) == D + 3 + 1
    with pytest.raises(ValueError):
        A.transact_device(weaver, [], 0x100, LAY, 0x200, [], (0x300, 0x400, 0x500, 0x600, None), 3, 8, outs)


def test_an_error_return_raises_with_the_library_text(weaver):
    weaver._L.play = lambda call: -1 if call.name == "cw_transact" else b"null token columns"
    with pytest.raises(abi.WeaveError, match="cw_transact: null token columns"):
        A.transact(weaver, DOFF, ISM, LAY, NTX, TOFF, KIND, ARG, CAUSE, CII, VK, new_cap=3, node_cap=8)
