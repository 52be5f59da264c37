"""CPU (-m "not gpu"): the C-ABI of zke_extract_captures_encoded and zke_utf8_lossy_batch without a GPU — the three symbols in the
header, the library, the ctypes mirror, the generated Rust, the C++ mirror and the safe Rust crate (same arguments in the same
order; no struct is new: the entry takes zke_capture_out and zke_encoded_out as they are), and every refusal that comes before
anything is staged: the checks run before the engine handle is looked at, so a handle that must not be dereferenced shows it."""
import ctypes as C
import os
import re
import sys

import numpy as np

from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_sys as g  # noqa: E402

HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zkemail_amd.h")).read(), flags=re.S)
NEW = ("zke_extract_captures_encoded", "zke_extract_captures_encoded_async", "zke_utf8_lossy_batch")
E_ARG, E_NOMEM = -1, -3
FAKE = C.c_void_p(1)             # an engine handle that must not be looked at: every check below comes first


def c_args(name):
    m = re.search(r"\bint %s\((.*?)\);" % name, HEADER, flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_symbols_and_signatures_in_every_mirror():
    build.build_engine()
    lib = C.CDLL(build.ENGINE_SO)
    rs = open(os.path.join(ROOT, "bindings", "zkemail-amd-sys", "src", "lib.rs")).read()
    assert rs == g.generate()
    loaded = engine.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in engine.EXPORTED_SYMBOLS
        args = c_args(name)
        assert len(getattr(loaded, name).argtypes) == len(args), name
        m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, rs)
        assert m and [a.split(":")[0].strip() for a in m.group(1).split(",")] == [a.split()[-1].lstrip("*") for a in args], name
    # the entry's signature is zke_extract_captures' plus the external-input table and the zke_encoded_out
    base = c_args("zke_extract_captures")
    assert c_args("zke_extract_captures_encoded") == base + ["const uint32_t* ext_off", "const uint32_t* ext_str_off", "const uint8_t* ext_blob",
                                                              "zke_encoded_out* enc"]
    assert c_args("zke_extract_captures_encoded_async") == c_args("zke_extract_captures_encoded") + ["uint64_t* ticket"]
    lib.zke_abi_version.restype = C.c_uint32
    assert lib.zke_abi_version() == 3                      # additive: no existing struct or entry changes
    assert A.UTF8_LOSSY_MAX_BYTES == int(re.search(r"#define ZKE_UTF8_LOSSY_MAX_BYTES (\d+)u", HEADER).group(1)) == (2 ** 32 - 1) // 3
    hpp = open(os.path.join(ROOT, "include", "zkemail_core.hpp")).read()
    assert "extract_captures_encoded(" in hpp and "zke_extract_captures_encoded(" in hpp and "utf8_lossy(" in hpp
    core = open(os.path.join(ROOT, "bindings", "zkemail-core-amd", "src", "lib.rs")).read()
    assert "pub fn extract_captures_encoded(" in core and "sys::zke_extract_captures_encoded(" in core and "sys::zke_utf8_lossy_batch(" in core


def test_utf8_lossy_batch_refuses_before_any_device_work():
    lib = engine.load_library()
    blob, out_off, flags, need = np.zeros(16, np.uint8), np.full(3, 7, np.uint32), np.zeros(2, np.uint8), C.c_size_t(9)
    off = np.array([0, 4, 8], np.uint64)
    call = lambda e=FAKE, b=blob.ctypes.data, o=off, n=2, oo=out_off.ctypes.data, ob=blob.ctypes.data, cap=16, nd=need, fl=flags.ctypes.data: \
        lib.zke_utf8_lossy_batch(e, b, o.ctypes.data if o is not None else None, n, oo, ob, cap, C.byref(nd) if nd is not None else None, fl)
    assert call(e=None) == E_ARG
    assert call(oo=None) == E_ARG and call(nd=None) == E_ARG and call(o=None) == E_ARG and call(fl=None) == E_ARG and call(ob=None) == E_ARG
    assert call(b=None) == E_ARG                                                     # bytes to read and no blob
    assert call(o=np.array([0, 9, 8], np.uint64)) == E_ARG and b"non-decreasing" in lib.zke_last_error(None)
    assert call(o=np.array([5, 5 + A.UTF8_LOSSY_MAX_BYTES + 1], np.uint64), n=1) == E_ARG and b"ZKE_UTF8_LOSSY_MAX_BYTES" in lib.zke_last_error(None)
    assert call(n=0) == 0 and out_off[0] == 0 and need.value == 0                     # nothing to run: the empty table is written here


def test_extract_captures_encoded_refuses_before_anything_is_staged():
    lib = engine.load_library()
    raw = b"From: a@example.com\r\n\r\nx\r\n"
    refs = (A.zke_email_ref * 2)()
    for r in refs:
        r.raw, r.raw_len = C.cast(C.c_char_p(raw), C.c_void_p).value, len(raw)
    out = np.zeros(2, A.RESULT_DTYPE)
    g1 = np.array([1, 2], np.uint32)
    parts = (A.zke_capture_part * 2)()
    for p in parts:
        p.dfa_id, p.prog_id, p.n_groups, p.groups = 0, 0, 2, g1.ctypes.data
    P, G = 2, 4
    spans, flags, cap_off, cap_str_off, blob = np.zeros(2 * G * 2, np.uint32), np.zeros(2 * G, np.uint8), np.zeros(2 * P + 1, np.uint32), np.zeros(2 * G + 1, np.uint32), np.zeros(64, np.uint8)
    caps = A.zke_capture_out()
    caps.spans, caps.spans_cap, caps.flags, caps.flags_cap = spans.ctypes.data, 2 * G * 2, flags.ctypes.data, 2 * G
    caps.cap_off, caps.cap_off_cap, caps.cap_str_off, caps.cap_str_off_cap = cap_off.ctypes.data, 2 * P + 1, cap_str_off.ctypes.data, 2 * G + 1
    caps.cap_blob, caps.cap_blob_cap = blob.ctypes.data, 64
    infos, data = np.zeros(2, A.ENCODED_INFO_DTYPE), np.zeros(4096, np.uint8)
    enc = A.zke_encoded_out(infos.ctypes.data, 2, data.ctypes.data, 4096, 0, 0)
    ext = A.StringTable([["n", "v"], ["name", "value"]])
    t = C.c_uint64()
    body = C.cast(C.byref(parts, C.sizeof(A.zke_capture_part)), C.POINTER(A.zke_capture_part))

    def call(e=FAKE, n=2, hp=parts, nh=1, bp=body, nb=1, o=out.ctypes.data, cp=caps, eo=ext.off.ctypes.data, es=ext.str_off.ctypes.data,
             eb=ext.blob.ctypes.data, en=enc, tk=t):
        return lib.zke_extract_captures_encoded_async(e, refs, n, hp, nh, bp, nb, o, C.byref(cp) if cp is not None else None, eo, es, eb,
                                                      C.byref(en) if en is not None else None, C.byref(tk) if tk is not None else None)
    assert call(e=None) == E_ARG and lib.zke_extract_captures_encoded(None, refs, 2, parts, 1, body, 1, out.ctypes.data, C.byref(caps), None, None, None,
                                                                      C.byref(enc)) == E_ARG
    assert call(en=None) == E_ARG and call(tk=None) == E_ARG and call(hp=None) == E_ARG and call(bp=None) == E_ARG and call(o=None) == E_ARG
    assert call(nh=0, nb=0) == E_ARG and call(nh=1, nb=A.CAP_MAX_PARTS) == E_ARG and b"ZKE_CAP_MAX_PARTS" in lib.zke_last_error(None)
    parts[1].n_groups = A.CAP_MAX_GROUPS + 1
    assert call() == E_ARG and b"ZKE_CAP_MAX_GROUPS" in lib.zke_last_error(None)
    parts[1].n_groups = 2
    # the refusal bound: n * G * 3 * ZKE_CAP_MAX_SPAN >= 2^32 (the e-mails are not read: the array holds two); one below passes this
    # check and is stopped by the next one (the caller's tables are too small for that many e-mails)
    n_bound = -(-2 ** 32 // (3 * A.CAP_MAX_SPAN * G))
    assert n_bound * G * 3 * A.CAP_MAX_SPAN >= 2 ** 32 > (n_bound - 1) * G * 3 * A.CAP_MAX_SPAN
    assert call(n=n_bound, cp=None) == E_ARG and b"3 * ZKE_CAP_MAX_SPAN" in lib.zke_last_error(None)
    assert call(n=n_bound) == E_ARG and b"3 * ZKE_CAP_MAX_SPAN" in lib.zke_last_error(None)
    assert call(n=n_bound - 1) == E_NOMEM and caps.spans_need == (n_bound - 1) * G * 2
    # a capture table that is too small, as zke_extract_captures reports it
    caps.cap_str_off_cap = 2 * G
    assert call() == E_NOMEM and caps.cap_str_off_need == 2 * G + 1
    caps.cap_str_off_cap = 2 * G + 1
    # the external-input table, as zke_encode_in's
    dmg = ext.off.copy(); dmg[1] = 9
    assert call(eo=dmg.ctypes.data) == E_ARG and b"decrease" in lib.zke_last_error(None)
    assert call(es=None) == E_ARG and b"non-zero tail" in lib.zke_last_error(None)
    assert call(eb=None) == E_ARG and b"non-zero tail" in lib.zke_last_error(None)
    # an encoding that could reach 2^32 bytes: external inputs whose offsets say 2^31 bytes twice (no byte of a blob is read)
    huge, two = np.array([0, 1 << 31, (1 << 32) - 1], np.uint32), np.array([0, 2, 2], np.uint32)
    assert call(eo=two.ctypes.data, es=huge.ctypes.data) == E_ARG and b"2^32" in lib.zke_last_error(None)
    # ... and one that only the largest matches the part lists can yield would take there
    near = np.array([0, (1 << 32) - 1024], np.uint32)
    assert call(eo=np.array([0, 1, 1], np.uint32).ctypes.data, es=near.ctypes.data) == E_ARG and b"2^32" in lib.zke_last_error(None)
    # zke_encoded_out: infos too small fails at once with infos_need set; null buffers
    few = A.zke_encoded_out(infos.ctypes.data, 1, data.ctypes.data, 4096, 7, 7)
    assert call(en=few) == E_NOMEM and (few.infos_need, few.bytes_need) == (2, 0)
    assert call(en=A.zke_encoded_out(None, 2, data.ctypes.data, 4096, 0, 0)) == E_ARG
    assert call(en=A.zke_encoded_out(infos.ctypes.data, 2, None, 4096, 0, 0)) == E_ARG
