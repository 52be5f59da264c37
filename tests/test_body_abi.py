"""CPU (-m "not gpu"): the C-ABI of the body extraction without a GPU — zke_extract_bodies refuses a null engine, null pointers,
unknown flag bits and an e-mail of 2^31 bytes before any device work; zke_body_info is 40 bytes in the header's field order; the
constants of the Python mirror and of the model agree with include/zkemail_amd.h; status 11 has a name that cites its site."""
import ctypes as C
import os
import re

import numpy as np

import body_model as M
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkemail_amd.h")).read()
E_ARG, E_NOMEM = -1, -3


def test_error_codes_are_the_headers():
    codes = dict(re.findall(r"#define\s+(ZKE_E_[A-Z]+)\s+\(?(-?\d+)\)?", HEADER))
    assert int(codes["ZKE_E_ARG"]) == E_ARG and int(codes["ZKE_E_NOMEM"]) == E_NOMEM


def test_arguments_are_refused_before_any_device_work():
    lib = engine.load_library()
    raw = b"From: a@example.com\r\n\r\nx\r\n"
    refs = (A.zke_email_ref * 2)()
    for r in refs:
        r.raw, r.raw_len = C.cast(C.c_char_p(raw), C.c_void_p).value, len(raw)
    infos = np.zeros(2, A.BODY_INFO_DTYPE)
    data = np.zeros(128, np.uint8)
    out = A.zke_body_out(infos.ctypes.data, 2, data.ctypes.data, 128, 0, 0)
    t = C.c_uint64()
    fake = C.c_void_p(1)            # an engine handle that must not be looked at: every check below comes first
    assert lib.zke_extract_bodies(None, refs, 2, 0, C.byref(out)) == E_ARG
    assert lib.zke_extract_bodies_async(None, refs, 2, 0, C.byref(out), C.byref(t)) == E_ARG
    assert lib.zke_extract_bodies(fake, None, 2, 0, C.byref(out)) == E_ARG
    assert lib.zke_extract_bodies(fake, refs, 2, 0, None) == E_ARG
    assert lib.zke_extract_bodies_async(fake, refs, 2, 0, C.byref(out), None) == E_ARG
    for flags in (2, 3, 0x80000000):
        assert lib.zke_extract_bodies(fake, refs, 2, flags, C.byref(out)) == E_ARG
        assert b"flag" in lib.zke_last_error(None)
    big = (A.zke_email_ref * 2)()
    big[0].raw, big[0].raw_len = refs[0].raw, len(raw)
    big[1].raw, big[1].raw_len = refs[0].raw, 1 << 31
    assert lib.zke_extract_bodies(fake, big, 2, 0, C.byref(out)) == E_ARG and b"2^31" in lib.zke_last_error(None)
    big[1].raw, big[1].raw_len = None, 5
    assert lib.zke_extract_bodies(fake, big, 2, 1, C.byref(out)) == E_ARG
    short = A.zke_body_out(infos.ctypes.data, 1, data.ctypes.data, 128, 77, 77)
    assert lib.zke_extract_bodies(fake, refs, 2, 0, C.byref(short)) == E_NOMEM and (short.infos_need, short.bytes_need) == (2, 0)
    assert lib.zke_extract_bodies(fake, refs, 2, 0, C.byref(A.zke_body_out(None, 2, data.ctypes.data, 128, 0, 0))) == E_ARG
    assert lib.zke_extract_bodies(fake, refs, 2, 0, C.byref(A.zke_body_out(infos.ctypes.data, 2, None, 128, 0, 0))) == E_ARG


def test_struct_layout_and_constants_match_the_header():
    assert C.sizeof(A.zke_body_info) == 40 == A.BODY_INFO_DTYPE.itemsize and C.sizeof(A.zke_body_out) == 48
    m = re.search(r"typedef struct zke_body_info \{(.*?)\} zke_body_info;", HEADER, flags=re.S)
    fields = re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f[0] for f in A.zke_body_info._fields_] == list(A.BODY_INFO_DTYPE.names)
    assert [A.zke_body_info.status.offset, A.zke_body_info.src_off.offset, A.zke_body_info.body_len.offset, A.zke_body_info.body_off.offset] == [0, 16, 24, 32]
    assert [A.BODY_INFO_DTYPE.fields[k][1] for k in ("status", "src_off", "body_len", "body_off")] == [0, 16, 24, 32]
    for cname, py in (("ZKE_BODYF_PART_KEEPS_EOL", A.BODYF_PART_KEEPS_EOL), ("ZKE_CTE_IDENTITY", A.CTE_IDENTITY), ("ZKE_CTE_BASE64", A.CTE_BASE64), ("ZKE_CTE_QP", A.CTE_QP)):
        assert int(re.search(r"#define\s+%s\s+(\d+)u" % cname, HEADER).group(1)) == py, cname
    enums = {k: int(v) for k, v in re.findall(r"\b(ZKE_(?:D_)?[A-Z0-9_]+)\s*=\s*(\d+)", HEADER)}
    assert enums["ZKE_BODY_DECODE_FAIL"] == 11 == A.ZKE_BODY_DECODE_FAIL and A.STATUS_NAMES[11] == "BODY_DECODE_FAIL"
    for name in ("D_BODY_B64_CHAR", "D_BODY_B64_LENGTH", "D_BODY_B64_TRAILING_BITS", "D_U_BODY_CTE"):
        assert enums["ZKE_" + name] == getattr(A, name) == getattr(M, name), name
    assert (enums["ZKE_D_BODY_B64_CHAR"], enums["ZKE_D_U_BODY_CTE"]) == (110, 113)
    assert (M.D_U_MIME_CTYPE, M.D_U_MIME_BOUNDARY, M.D_U_MIME_DEPTH) == (A.D_U_MIME_CTYPE, A.D_U_MIME_BOUNDARY, A.D_U_MIME_DEPTH)
    assert (M.CTE_IDENTITY, M.CTE_BASE64, M.CTE_QP, M.PART_HTML) == (A.CTE_IDENTITY, A.CTE_BASE64, A.CTE_QP, A.BODY_PART_HTML)


def test_new_entry_points_are_exported_and_named():
    lib = engine.load_library()
    assert {"zke_extract_bodies", "zke_extract_bodies_async"} <= set(engine.EXPORTED_SYMBOLS)
    assert hasattr(lib, "zke_extract_bodies") and hasattr(lib, "zke_extract_bodies_async")
    assert lib.zke_abi_version() == 3                       # new entry points change no layout
    assert b"core/src/email.rs:17-21" in lib.zke_status_name(A.ZKE_BODY_DECODE_FAIL) and A.STATUS_SITE[11] == "core/src/email.rs:17-21"
