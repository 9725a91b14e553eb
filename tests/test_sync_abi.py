"""cause_amd/abi_sync.py against include/causeweave_sync.h (no GPU).

The three structs and the two signatures are compared with what
tests/jvm_twins.py parses out of the header (fed the main header's text first,
so that its typedefs resolve); drifted copies must be reported; the built
library exports both symbols; version, delta, version_device and delta_device
run against the stub library of tests/test_abi_calls.py.
"""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest

from cause_amd import abi, abi_sync
from tests import jvm_twins as J
from tests import test_abi_calls as S
from tests import test_abi_header as H

MAIN = open(abi.HEADER).read()
SRC = open(abi_sync.HEADER).read()
NEW_STRUCTS = {"cw_sync_batch": abi_sync.CwSyncBatch, "cw_version_result": abi_sync.CwVersionResult,
               "cw_delta_result": abi_sync.CwDeltaResult}
U8, U32, U64 = np.uint8, np.uint32, np.uint64


def c_kind(text, layouts):
    base = text.split()[0]
    if text == base + " *" and base in NEW_STRUCTS:
        return NEW_STRUCTS[base]
    return H.c_kind(text, layouts)


def check_abi(src):
    """Problems between abi_sync.py and the header text (empty = in line)."""
    problems = []
    layouts = J.header_layouts(MAIN + "\n" + src)
    new = {t: v for t, v in layouts.items() if t not in J.header_layouts(MAIN)}
    if set(new) != set(NEW_STRUCTS):
        problems.append(f"the header defines {sorted(new)}, abi_sync.py mirrors {sorted(NEW_STRUCTS)}")
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
    for name in sorted(set(abi_sync.SIGNATURES) - set(protos)):
        problems.append(f"abi_sync.SIGNATURES has {name}, which the header does not declare")
    for name, (ret, params) in protos.items():
        if name not in abi_sync.SIGNATURES:
            problems.append(f"abi_sync.SIGNATURES lacks {name}")
            continue
        restype, argtypes = abi_sync.SIGNATURES[name]
        want = (c_kind(ret, layouts), [c_kind(p, layouts) for p in params])
        got = (H.ct_kind(restype), [H.ct_kind(t) for t in argtypes])
        if got != want:
            problems.append(f"{name}: abi_sync.SIGNATURES {got}, header {want}")
    return problems


def test_abi_sync_mirrors_the_header():
    assert check_abi(SRC) == []
    layouts = J.header_layouts(MAIN + "\n" + SRC)
    assert [f for f, *_ in layouts["cw_sync_batch"][0]] == [
        "n_docs", "doc_offsets", "id_key", "cause", "kind", "cause_is_id", "ts_shift", "site_shift", "site_bits",
        "reserved"]
    assert [f for f, *_ in layouts["cw_version_result"][0]] == ["ver", "yarn_len", "max_ts"]
    assert [f for f, *_ in layouts["cw_delta_result"][0]] == [
        "delta_offsets", "delta_src", "delta_id", "delta_cause", "delta_kind", "delta_cause_is_id", "ahead"]
    assert J.header_prototypes(SRC) == {
        "cw_version": ("int", ["cw_ctx *", "cw_sync_batch *", "cw_version_result *", "int"]),
        "cw_delta": ("int", ["cw_ctx *", "cw_sync_batch *", "uint64_t *", "cw_delta_result *", "int"])}
    assert f"#define CW_SYNC_WAVE_CAP {abi_sync.WAVE_CAP}\n" in SRC


def test_the_main_header_is_as_it_was():
    for name in ("cw_version", "cw_delta"):
        assert name not in abi.SIGNATURES and name not in J.header_prototypes(MAIN)
    assert not [t for t in J.header_layouts(MAIN) if t in NEW_STRUCTS]


@pytest.mark.parametrize("old,new,what", [
    ("  const uint64_t *cause;  ", "  const uint64_t *kind_;  ", "CwSyncBatch"),
    ("  uint32_t reserved;  ", "  uint64_t reserved;  ", "CwSyncBatch"),
    ("  uint32_t ts_shift;\n  uint32_t site_shift;\n", "  uint32_t site_shift;\n  uint32_t ts_shift;\n", "CwSyncBatch"),
    ("  uint32_t *yarn_len;  ", "  uint32_t yarn_len;  ", "CwVersionResult"),
    ("  uint64_t *delta_offsets;  ", "  uint32_t delta_offsets;  ", "CwDeltaResult"),
    ("  uint32_t *ahead;  ", "  uint32_t ahead[2];  ", "CwDeltaResult"),
    ("const uint64_t *have, cw_delta_result *result, int memspace);", "cw_delta_result *result, int memspace);",
     "cw_delta"),
    ("int cw_version(", "int cw_versions(", "cw_version"),
    ("#ifdef __cplusplus\n}\n", "int cw_spin(cw_ctx *ctx);\n#ifdef __cplusplus\n}\n", "lacks cw_spin"),
])
def test_a_drifted_header_is_reported(old, new, what):
    assert SRC.count(old) == 1, old
    problems = check_abi(SRC.replace(old, new))
    assert problems and any(what in p for p in problems), problems


def test_the_library_exports_the_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    for name in ("cw_version", "cw_delta"):
        assert any(line.split()[-1] == name and line.split()[-2] == "T"
                   for line in out.splitlines() if line.strip()), name
    L = abi_sync.lib()
    for name, (restype, argtypes) in abi_sync.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert os.path.basename(abi_sync.HEADER) == "causeweave_sync.h"


# ------------------------------------------------------------- against the stub
OFF = [0, 4, 4, 6]
N, D, P = 6, 3, 3
LAY = NS(ts_shift=20, site_shift=18, site_bits=2)
WORDS = D << LAY.site_bits
DO = np.array([0, 2, 2, 3], U64)
VER = np.arange(WORDS, dtype=U64) + U64(500)
weaver = S.weaver


def inputs():
    return (np.arange(N, dtype=U64) + U64(10), np.arange(N, dtype=U64) * U64(3), (np.arange(N) % 4).astype(U8),
            np.ones(N, U8))


def play(call):
    if call.name == "cw_version":
        b, r = call.snaps
        if call.plain == [abi.CW_MEM_HOST]:
            call.seen = {"off": S.rd(b["doc_offsets"], U64, D + 1), "id": S.rd(b["id_key"], U64, N)}
            S.wr(r["ver"], VER)
            S.wr(r["yarn_len"], np.arange(WORDS, dtype=U32) + U32(7))
            S.wr(r["max_ts"], np.array([9, 0, 8], U64))
        return
    b, r = call.snaps
    if call.plain[-1] == abi.CW_MEM_HOST:
        call.seen = {"off": S.rd(b["doc_offsets"], U64, D + 1), "id": S.rd(b["id_key"], U64, N),
                     "have": S.rd(call.plain[0].value, U64, WORDS)}
        S.wr(r["delta_src"], np.array([1, 3, 0], U32))
        S.wr(r["delta_id"], np.array([11, 13, 14], U64))
        if r["delta_kind"] is not None:
            S.wr(r["delta_kind"], np.array([1, 3, 0], U8))
        S.wr(r["ahead"], np.array([0, 2, 0], U32))
    S.wr(r["delta_offsets"], DO)


def test_version_host(weaver):
    weaver._L.play = play
    res = abi_sync.version(weaver, OFF, inputs()[0], LAY)
    call = S.one_call(weaver, "cw_version", abi.CW_MEM_HOST)
    assert call.types == [abi_sync.CwSyncBatch, abi_sync.CwVersionResult]
    b, r = call.snaps
    assert (b["n_docs"], b["ts_shift"], b["site_shift"], b["site_bits"], b["reserved"]) == (D, 20, 18, 2, 0)
    assert S.nulls(b) == {"cause", "kind", "cause_is_id"} and S.nulls(r) == set()
    S.same(call.seen["off"], np.array(OFF, U64)), S.same(call.seen["id"], inputs()[0])
    assert isinstance(res, abi_sync.VersionResult)
    S.same(res.ver, VER), S.same(res.yarn_len, np.arange(WORDS, dtype=U32) + U32(7))
    S.same(res.max_ts, np.array([9, 0, 8], U64))
    with pytest.raises(ValueError):
        abi_sync.version(weaver, [0, 4, 4, 5], inputs()[0], LAY)
    with pytest.raises(ValueError):
        abi_sync.version(weaver, [], inputs()[0][:0], LAY)


@pytest.mark.parametrize("maps", [True, False])
def test_delta_host(weaver, maps):
    ids, ca, kd, cii = inputs()
    weaver._L.play = play
    res = abi_sync.delta(weaver, OFF, ids, ca, kd, cii if maps else None, LAY, VER)
    call = S.one_call(weaver, "cw_delta", ...)
    assert call.types == [abi_sync.CwSyncBatch, abi_sync.CwDeltaResult]
    assert len(call.plain) == 2 and call.plain[1] == abi.CW_MEM_HOST
    b, r = call.snaps
    assert (b["n_docs"], b["site_bits"], b["reserved"]) == (D, 2, 0)
    assert S.nulls(b) == (set() if maps else {"cause_is_id"})
    assert S.nulls(r) == (set() if maps else {"delta_cause_is_id"})
    S.same(call.seen["off"], np.array(OFF, U64)), S.same(call.seen["id"], ids), S.same(call.seen["have"], VER)
    assert isinstance(res, abi_sync.DeltaResult)
    S.same(res.delta_offsets, DO), S.same(res.delta_src, np.array([1, 3, 0], U32))
    S.same(res.delta_id, np.array([11, 13, 14], U64)), S.same(res.delta_kind, np.array([1, 3, 0], U8))
    S.same(res.ahead, np.array([0, 2, 0], U32))
    assert (res.delta_cause_is_id is None) == (not maps) and len(res.delta_cause) == P
    assert S.cap(res.delta_id) == N and S.cap(res.delta_src) == N      # sized for N


def test_delta_host_checks_sizes(weaver):
    ids, ca, kd, cii = inputs()
    ok = [OFF, ids, ca, kd, cii, LAY, VER]
    for at, bad in ((1, ids[:3]), (2, ca[:5]), (3, kd[:2]), (4, cii[:1]), (6, VER[:5]), (0, [0, 4, 4, 5]), (0, [])):
        args = list(ok)
        args[at] = bad
        with pytest.raises(ValueError):
            abi_sync.delta(weaver, *args)
    assert weaver._L.calls == []


def test_version_device(weaver):
    weaver._L.play = play
    assert abi_sync.version_device(weaver, OFF, 0x100, LAY, {"ver": 0x1000, "max_ts": 0x3000}) is None
    call = S.one_call(weaver, "cw_version", abi.CW_MEM_DEVICE)
    b, r = call.snaps
    assert b["id_key"] == 0x100 and S.nulls(b) == {"cause", "kind", "cause_is_id"}
    assert (b["n_docs"], b["ts_shift"], b["site_shift"], b["site_bits"]) == (D, 20, 18, 2)
    assert r == {"ver": 0x1000, "yarn_len": None, "max_ts": 0x3000}


@pytest.mark.parametrize("full", [True, False])
def test_delta_device(weaver, full):
    weaver._L.play = play
    outs = {"delta_src": 0x1000}
    ptrs = (0x100,)
    if full:
        outs.update(delta_id=0x2000, delta_cause=0x3000, delta_kind=0x4000, delta_cause_is_id=0x5000, ahead=0x6000)
        ptrs = (0x100, 0x200, 0x300, 0x400)
    do = abi_sync.delta_device(weaver, OFF, ptrs, LAY, 0x900, outs)
    call = S.one_call(weaver, "cw_delta", ...)
    assert call.plain[0].value == 0x900 and call.plain[1] == abi.CW_MEM_DEVICE
    b, r = call.snaps
    assert (b["id_key"], b["cause"], b["kind"], b["cause_is_id"]) == (ptrs + (None,) * 3)[:4]
    assert {f: r[f] for f in outs} == outs
    assert S.nulls(r) == (set() if full else {"delta_id", "delta_cause", "delta_kind", "delta_cause_is_id", "ahead"})
    S.same(do, DO)
    with pytest.raises(ValueError):
        abi_sync.delta_device(weaver, [], ptrs, LAY, 0x900, outs)


def test_an_error_return_raises_with_the_library_text(weaver):
    weaver._L.play = lambda call: -1 if call.name in ("cw_version", "cw_delta") else b"doc_offsets not monotone"
    ids, ca, kd, cii = inputs()
    with pytest.raises(abi.WeaveError, match="cw_delta: doc_offsets not monotone"):
        abi_sync.delta(weaver, OFF, ids, ca, kd, cii, LAY, VER)
    with pytest.raises(abi.WeaveError, match="cw_version: doc_offsets not monotone"):
        abi_sync.version(weaver, OFF, ids, LAY)
