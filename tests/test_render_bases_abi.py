"""cause_amd/abi_render_bases.py against include/causeweave_render_bases.h (no GPU).

The two structs and the signature are compared with what tests/jvm_twins.py
parses out of the header (fed the main header's text first, so that its
typedefs resolve); drifted copies must be reported; the main header is as it
was; the built library exports the symbol; render_bases and
render_bases_device run against the stub library of tests/test_abi_calls.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cause_amd import abi, abi_render_bases as A
from tests import jvm_twins as J
from tests import test_abi_calls as S
from tests import test_abi_header as H

MAIN = open(abi.HEADER).read()
SRC = open(A.HEADER).read()
NEW_STRUCTS = {"cw_render_bases_batch": A.CwRenderBasesBatch, "cw_render_bases_result": A.CwRenderBasesResult}
U8, U32, U64 = np.uint8, np.uint32, np.uint64


def c_kind(text, layouts):
    base = text.split()[0]
    if text == base + " *" and base in NEW_STRUCTS:
        return NEW_STRUCTS[base]
    return H.c_kind(text, layouts)


def check_abi(src):
    """Problems between abi_render_bases.py and the header text (empty = in line)."""
    problems = []
    layouts = J.header_layouts(MAIN + "\n" + src)
    new = {t: v for t, v in layouts.items() if t not in J.header_layouts(MAIN)}
    if set(new) != set(NEW_STRUCTS):
        problems.append(f"the header defines {sorted(new)}, abi_render_bases.py mirrors {sorted(NEW_STRUCTS)}")
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
        problems.append(f"abi_render_bases.SIGNATURES has {name}, which the header does not declare")
    for name, (ret, params) in protos.items():
        if name not in A.SIGNATURES:
            problems.append(f"abi_render_bases.SIGNATURES lacks {name}")
            continue
        restype, argtypes = A.SIGNATURES[name]
        want = (c_kind(ret, layouts), [c_kind(p, layouts) for p in params])
        got = (H.ct_kind(restype), [H.ct_kind(t) for t in argtypes])
        if got != want:
            problems.append(f"{name}: abi_render_bases.SIGNATURES {got}, header {want}")
    return problems


def test_abi_render_bases_mirrors_the_header():
    assert check_abi(SRC) == []
    layouts = J.header_layouts(MAIN + "\n" + SRC)
    assert [f for f, *_ in layouts["cw_render_bases_batch"][0]] == [
        "n_docs", "ent_offsets", "ent_ref", "n_bases", "root_doc"]
    assert [f for f, *_ in layouts["cw_render_bases_result"][0]] == [
        "base_tok_offsets", "tok_kind", "tok_doc", "tok_entry", "base_status", "doc_base", "doc_open"]
    assert J.header_prototypes(SRC) == {
        "cw_render_bases": ("int", ["cw_ctx *", "cw_render_bases_batch *", "cw_render_bases_result *", "int"])}


def test_the_constants_are_the_headers():
    consts = J.header_constants(SRC)
    assert consts["CW_STATUS_REF_SHARED"] == A.STATUS_REF_SHARED == 1 << 9
    assert [consts[n] for n in ("CW_TOK_OPEN", "CW_TOK_CLOSE", "CW_TOK_LEAF", "CW_TOK_NIL")] == \
        [A.TOK_OPEN, A.TOK_CLOSE, A.TOK_LEAF, A.TOK_NIL]
    assert A.STATUS_REF_SHARED not in J.header_constants(MAIN).values()


def test_the_main_header_is_as_it_was():
    assert "cw_render_bases" not in abi.SIGNATURES and "cw_render_bases" not in J.header_prototypes(MAIN)
    assert not [t for t in J.header_layouts(MAIN) if t.startswith("cw_render_bases")]
    assert "REF_SHARED" not in MAIN and "recursion into them is host work" in " ".join(MAIN.split()).replace("* ", "")


@pytest.mark.parametrize("old,new,what", [
    ("  uint8_t  *tok_kind;  ", "  uint32_t *tok_doc;  ", "CwRenderBasesResult"),
    ("  uint64_t n_bases;\n", "  uint32_t n_bases;\n", "CwRenderBasesBatch"),
    ("  const uint32_t *ent_ref;  ", "  uint32_t ent_ref;  ", "CwRenderBasesBatch"),
    ("  uint32_t *doc_open;  ", "  uint32_t doc_open[2];  ", "CwRenderBasesResult"),
    ("  uint64_t *base_tok_offsets;  ", "  uint32_t base_tok_offsets;  ", "CwRenderBasesResult"),
    ("cw_render_bases_result *result, int memspace);", "cw_render_bases_result *result);", "cw_render_bases"),
    ("int cw_render_bases(", "int cw_render_base(", "cw_render_bases"),
    ("#ifdef __cplusplus\n}\n", "int cw_render_dag(cw_ctx *ctx);\n#ifdef __cplusplus\n}\n", "lacks cw_render_dag"),
])
def test_a_drifted_header_is_reported(old, new, what):
    assert SRC.count(old) == 1, old
    problems = check_abi(SRC.replace(old, new))
    assert problems and any(what in p for p in problems), problems


def test_the_library_exports_the_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    assert any(line.split()[-1] == "cw_render_bases" and line.split()[-2] == "T"
               for line in out.splitlines() if line.strip())
    L = A.lib()
    restype, argtypes = A.SIGNATURES["cw_render_bases"]
    assert L.cw_render_bases.restype is restype and list(L.cw_render_bases.argtypes) == argtypes
    assert os.path.basename(A.HEADER) == "causeweave_render_bases.h"


# ------------------------------------------------------------- against the stub
OFF, REF, ROOT = [0, 3, 3, 4], [0xFFFFFFFF, 2, 9, 0xFFFFFFFF], [0, 5]
D, G, E, T = 3, 2, 4, 7
BO = np.array([0, 7, 7], U64)
KIND = np.array([0, 2, 0, 2, 1, 3, 1], U8)
weaver = S.weaver


def play(call):
    b, r = call.snaps
    if call.plain == [abi.CW_MEM_HOST]:
        call.seen = {"off": S.rd(b["ent_offsets"], U64, D + 1), "ref": S.rd(b["ent_ref"], U32, E),
                     "root": S.rd(b["root_doc"], U32, G)}
        if r["tok_kind"] is not None:
            S.wr(r["tok_kind"], KIND)
            S.wr(r["tok_doc"], np.arange(T, dtype=U32) + U32(10))
            S.wr(r["tok_entry"], np.arange(T, dtype=U32) + U32(20))
        S.wr(r["base_status"], np.array([0, 512], U32))
        S.wr(r["doc_base"], np.array([0, 0xFFFFFFFF, 0], U32))
        S.wr(r["doc_open"], np.array([0, 9, 2], U32))
    S.wr(r["base_tok_offsets"], BO)


@pytest.mark.parametrize("tokens", [True, False])
def test_render_bases_host(weaver, tokens):
    weaver._L.play = play
    res = A.render_bases(weaver, OFF, REF, ROOT, tokens=tokens)
    call = S.one_call(weaver, "cw_render_bases", abi.CW_MEM_HOST)
    assert call.types == [A.CwRenderBasesBatch, A.CwRenderBasesResult]
    b, r = call.snaps
    assert (b["n_docs"], b["n_bases"]) == (D, G) and S.nulls(b) == set()
    assert S.nulls(r) == (set() if tokens else {"tok_kind", "tok_doc", "tok_entry"})
    S.same(call.seen["off"], np.array(OFF, U64)), S.same(call.seen["ref"], np.array(REF, U32))
    S.same(call.seen["root"], np.array(ROOT, U32))
    assert isinstance(res, A.RenderBasesResult)
    S.same(res.base_tok_offsets, BO), S.same(res.base_status, np.array([0, 512], U32))
    S.same(res.doc_base, np.array([0, 0xFFFFFFFF, 0], U32)), S.same(res.doc_open, np.array([0, 9, 2], U32))
    if tokens:
        S.same(res.tok_kind, KIND), S.same(res.tok_doc, np.arange(T, dtype=U32) + U32(10))
        S.same(res.tok_entry, np.arange(T, dtype=U32) + U32(20))
        assert S.cap(res.tok_kind) == S.cap(res.tok_doc) == S.cap(res.tok_entry) == E + 2 * D
    else:
        assert res.tok_kind is None and res.tok_doc is None and res.tok_entry is None


def test_render_bases_host_checks_sizes(weaver):
    for off, ref in (([0, 3, 3, 5], REF), ([], REF), ([0, 3, 3, 4], REF[:2])):
        with pytest.raises(ValueError):
            A.render_bases(weaver, off, ref, ROOT)
    assert weaver._L.calls == []


@pytest.mark.parametrize("full", [True, False])
def test_render_bases_device(weaver, full):
    weaver._L.play = play
    outs = {"base_status": 0x4000}
    if full:
        outs.update(tok_kind=0x1000, tok_doc=0x2000, tok_entry=0x3000, doc_base=0x5000, doc_open=0x6000)
    bo = A.render_bases_device(weaver, OFF, 0x100, G, 0x200, outs)
    call = S.one_call(weaver, "cw_render_bases", abi.CW_MEM_DEVICE)
    b, r = call.snaps
    assert (b["ent_ref"], b["root_doc"], b["n_docs"], b["n_bases"]) == (0x100, 0x200, D, G)
    assert {f: r[f] for f in outs} == outs
    assert S.nulls(r) == (set() if full else {"tok_kind", "tok_doc", "tok_entry", "doc_base", "doc_open"})
    S.same(bo, BO)
    with pytest.raises(ValueError):
        A.render_bases_device(weaver, [], 0x100, G, 0x200, outs)


def test_an_error_return_raises_with_the_library_text(weaver):
    weaver._L.play = lambda call: -1 if call.name == "cw_render_bases" else b"null ent_ref"
    with pytest.raises(abi.WeaveError, match="cw_render_bases: null ent_ref"):
        A.render_bases(weaver, OFF, REF, ROOT)
