"""CPU (-m "not gpu"): the C-ABI of the device-side output encoding (zke_verify_emails_encoded, zke_encode_outputs) without a GPU —
the three symbols, zke_encoded_info and zke_encode_in in the header, the ctypes mirror and the generated Rust (48 and 48 bytes, the
header's field order), the tables the Python packer builds from verifier outputs, the plan's places and lengths against
len(abi_encode(..)) for 500 seeded outputs (through the entry's own checks, which come before any device work), and every refusal
the header lists."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

import encode_cases as EC
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build, engine
from zkemail_rs_amd.abi_encode import abi_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_sys as g  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "zkemail_amd.h")).read()
E_ARG, E_NOMEM = -1, -3
FAKE = C.c_void_p(1)             # an engine handle that must not be looked at: every check below comes first


def encode_call(lib, tb, enc, n=None, **over):
    a = dict(records=tb.records.ctypes.data, kinds=tb.kinds.ctypes.data, ext_off=tb.ext.off.ctypes.data, ext_str_off=tb.ext.str_off.ctypes.data,
             ext_blob=tb.ext.blob.ctypes.data, match_off=tb.matches.off.ctypes.data, match_str_off=tb.matches.str_off.ctypes.data,
             match_blob=tb.matches.blob.ctypes.data)
    a.update(over)
    return lib.zke_encode_outputs(FAKE, a["records"], tb.n if n is None else n, a["kinds"], a["ext_off"], a["ext_str_off"], a["ext_blob"],
                                  a["match_off"], a["match_str_off"], a["match_blob"], C.byref(enc) if enc is not None else None)


def test_symbols_are_exported_and_abi_version_stays():
    build.build_engine()
    lib = C.CDLL(build.ENGINE_SO)
    for name in ("zke_verify_emails_encoded", "zke_verify_emails_encoded_async", "zke_encode_outputs"):
        assert hasattr(lib, name) and name in engine.EXPORTED_SYMBOLS
    lib.zke_abi_version.restype = C.c_uint32
    assert lib.zke_abi_version() == 3                      # additive, as the entries before these: no existing struct changes
    assert "not validated as UTF-8" in re.sub(r"\s+", " ", HEADER.replace("NOT", "not"))


def test_the_three_mirrors_of_the_new_structs_agree(tmp_path):
    """sizeof / offsetof as the C compiler lays the header out, against ctypes and numpy; field for field against the generated Rust."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkemail_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(zke_encoded_info), sizeof(zke_encoded_out), sizeof(zke_encode_in),\n'
                   '         offsetof(zke_encoded_info, len), offsetof(zke_encoded_info, kind), offsetof(zke_encoded_info, digest),\n'
                   '         offsetof(zke_encoded_out, bytes_need), offsetof(zke_encode_in, mixed), offsetof(zke_encode_in, ext_blob));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    b = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(A.zke_encoded_info), C.sizeof(A.zke_encoded_out), C.sizeof(A.zke_encode_in), A.zke_encoded_info.len.offset,
                   A.zke_encoded_info.kind.offset, A.zke_encoded_info.digest.offset, A.zke_encoded_out.bytes_need.offset,
                   A.zke_encode_in.mixed.offset, A.zke_encode_in.ext_blob.offset]
    assert out[:3] == [48, 48, 40] and out[3:6] == [8, 12, 16]
    assert A.ENCODED_INFO_DTYPE.itemsize == 48 and [A.ENCODED_INFO_DTYPE.fields[k][1] for k in ("off", "len", "kind", "digest")] == [0, 8, 12, 16]
    for name in ("zke_encoded_info", "zke_encoded_out", "zke_encode_in"):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S)
        fields = re.findall(r"\b([a-z_]+)(?:\[\d+\])?(?=[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert fields == [f[0] for f in getattr(A, name)._fields_], name
    assert list(A.ENCODED_INFO_DTYPE.names) == [f[0] for f in A.zke_encoded_info._fields_]
    rs = open(os.path.join(ROOT, "bindings", "zkemail-amd-sys", "src", "lib.rs")).read()
    assert rs == g.generate()
    structs = {m.group(1): re.findall(r"pub ([\w#]+): ([^,\n]+),", m.group(2))
               for m in re.finditer(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct (\w+) \{(.*?)\n\}", rs, flags=re.S)}
    width = {"u32": 4, "u64": 8, "usize": 8, "[u8; 32]": 32}
    for name in ("zke_encoded_info", "zke_encoded_out", "zke_encode_in"):
        py = getattr(A, name)._fields_
        assert [f for f, _ in structs[name]] == [f for f, _ in py], name
        for (_, rt), (_, pt) in zip(structs[name], py):
            assert (8 if rt.startswith("*") else width[rt]) == C.sizeof(pt), (name, rt)
    for fn in ("zke_verify_emails_encoded", "zke_verify_emails_encoded_async", "zke_encode_outputs"):
        assert re.search(r"pub fn %s\(" % fn, rs), fn


def test_the_packer_builds_the_tables_from_verifier_outputs():
    e0 = A.EmailVerifierOutput(bytes(range(32)), bytes(range(32, 64)), ["name", "välue"])
    e1 = A.EmailWithRegexVerifierOutput(A.EmailVerifierOutput(b"\x01" * 32, b"\x02" * 32, []), ["m0", "", "漢"])
    e2 = A.EmailWithRegexVerifierOutput(A.EmailVerifierOutput(b"\x03" * 32, b"\x04" * 32, ["a", "b", "c", "d"]), [])
    tb = A.EncodeTables([e0, e1, e2], [A.ZKE_OK, A.ZKE_DKIM_NOT_PASS, A.ZKE_OK])
    assert tb.n == 3 and list(tb.kinds) == [0, 1, 1]
    assert list(tb.ext.off) == [0, 2, 2, 6] and list(tb.ext.str_off) == [0, 4, 10, 11, 12, 13, 14]
    assert tb.ext.blob[:14].tobytes() == "namevälueabcd".encode()
    assert list(tb.matches.off) == [0, 0, 3, 3] and list(tb.matches.str_off) == [0, 2, 2, 5] and tb.matches.blob[:5].tobytes() == "m0漢".encode()
    assert [int(s) for s in tb.records["status"][:3]] == [0, 4, 0]
    assert tb.records[0]["from_domain_hash"].tobytes() == bytes(range(32)) and tb.records[2]["public_key_hash"].tobytes() == b"\x04" * 32
    x = [A.ExternalInput("n1", "v1"), A.ExternalInput("n2", None), A.ExternalInput("", "v3")]
    assert A.flat_external_inputs(x) == ["n1", "v1", "n2", "", "", "v3"]
    assert A.encoded_len(0, [4, 6]) == len(abi_encode(e0)) and A.encoded_len(1, [], [2, 0, 3]) == len(abi_encode(e1.email, e1.regex_matches))


def test_the_plan_places_500_seeded_outputs_where_abi_encode_says():
    """len: a batch of one per output (bytes_need of a call that fails with ZKE_E_NOMEM at once); enc_off: bytes_need of every prefix
    of the batch, i.e. the place the next e-mail gets — whatever the statuses, which the plan does not read."""
    lib = engine.load_library()
    outs = EC.plan_outputs()
    assert len(outs) == 500
    refs = [EC.ref_bytes(o) for o in outs]
    sizes = {len(o.email.external_inputs if isinstance(o, A.EmailWithRegexVerifierOutput) else o.external_inputs) for o in outs}
    assert {0, 130} <= sizes and any(isinstance(o, A.EmailWithRegexVerifierOutput) and len(o.regex_matches) == 130 for o in outs)
    for i, o in enumerate(outs):
        tb = A.EncodeTables([o], [i % 12])
        enc = A.zke_encoded_out()
        assert encode_call(lib, tb, enc) == E_NOMEM and (enc.infos_need, enc.bytes_need) == (1, len(refs[i])), i
        assert A.encoded_len(int(tb.kinds[0]), np.diff(tb.ext.str_off), np.diff(tb.matches.str_off)) == len(refs[i])
    tb = A.EncodeTables(outs)
    off = 0
    for k in range(1, len(outs) + 1):
        enc = A.zke_encoded_out()
        off += len(refs[k - 1])
        assert encode_call(lib, tb, enc, n=k) == E_NOMEM and (enc.infos_need, enc.bytes_need) == (k, off), k
    # exact-size buffers pass the size check (the next thing the call does is look at the engine, which this test must not reach:
    # so one byte short is the last thing that can be shown here)
    infos, data = np.zeros(500, A.ENCODED_INFO_DTYPE), np.zeros(off, np.uint8)
    short = A.zke_encoded_out(infos.ctypes.data, 500, data.ctypes.data, off - 1, 0, 0)
    assert encode_call(lib, tb, short) == E_NOMEM and short.bytes_need == off
    short = A.zke_encoded_out(infos.ctypes.data, 499, data.ctypes.data, off, 0, 0)
    assert encode_call(lib, tb, short) == E_NOMEM and short.infos_need == 500


def test_arguments_are_refused_before_any_device_work():
    lib = engine.load_library()
    outs = EC.random_outputs(3, 4)
    tb = A.EncodeTables(outs)
    _, total = EC.expected(outs)
    infos, data = np.zeros(4, A.ENCODED_INFO_DTYPE), np.zeros(total, np.uint8)
    ok = lambda: A.zke_encoded_out(infos.ctypes.data, 4, data.ctypes.data, total, 0, 0)
    assert lib.zke_encode_outputs(None, None, 0, None, None, None, None, None, None, None, None) == E_ARG
    assert encode_call(lib, tb, None) == E_ARG
    assert encode_call(lib, tb, ok(), records=None) == E_ARG and encode_call(lib, tb, ok(), kinds=None) == E_ARG
    bad = np.array([0, 1, 2, 0], np.uint32)
    assert encode_call(lib, tb, ok(), kinds=bad.ctypes.data) == E_ARG and b"kind" in lib.zke_last_error(None)
    # offsets that decrease, in each of the four arrays
    for field, arr in (("ext_off", tb.ext.off), ("ext_str_off", tb.ext.str_off), ("match_off", tb.matches.off), ("match_str_off", tb.matches.str_off)):
        if len(arr) < 3 or arr[-1] == 0:
            continue
        dmg = arr.copy()
        dmg[len(dmg) // 2] = dmg[-1] + 5
        assert encode_call(lib, tb, ok(), **{field: dmg.ctypes.data}) == E_ARG and b"decrease" in lib.zke_last_error(None), field
    # a null table with a non-zero tail
    assert tb.ext.off[-1] and tb.matches.off[-1]
    for field in ("ext_str_off", "ext_blob", "match_str_off", "match_blob"):
        assert encode_call(lib, tb, ok(), **{field: None}) == E_ARG and b"non-zero tail" in lib.zke_last_error(None), field
    # ... while null tables altogether are "no strings anywhere": the sizes are those of empty lists
    enc = A.zke_encoded_out()
    assert encode_call(lib, tb, enc, ext_off=None, ext_str_off=None, ext_blob=None, match_off=None, match_str_off=None, match_blob=None) == E_NOMEM
    assert enc.bytes_need == sum(A.encoded_len(int(k), [], []) for k in tb.kinds[:4])
    # an encoding of 2^32 bytes: two strings whose offsets say 2^31 bytes each (no byte of a blob is read by the plan)
    one = A.EncodeTables([outs[0]])
    huge = np.array([0, 1 << 31, (1 << 32) - 1], np.uint32)
    two = np.array([0, 2], np.uint32)
    assert encode_call(lib, one, ok(), ext_off=two.ctypes.data, ext_str_off=huge.ctypes.data) == E_ARG and b"2^32" in lib.zke_last_error(None)
    # null buffers in enc
    assert encode_call(lib, tb, A.zke_encoded_out(None, 4, data.ctypes.data, total, 0, 0)) == E_ARG
    assert encode_call(lib, tb, A.zke_encoded_out(infos.ctypes.data, 4, None, total, 0, 0)) == E_ARG


def test_the_verify_entry_checks_its_arguments_first():
    lib = engine.load_library()
    raw = b"From: a@example.com\r\n\r\nx\r\n"
    refs = (A.zke_email_ref * 2)()
    for r in refs:
        r.raw, r.raw_len = C.cast(C.c_char_p(raw), C.c_void_p).value, len(raw)
    out = np.zeros(2, A.RESULT_DTYPE)
    infos, data = np.zeros(2, A.ENCODED_INFO_DTYPE), np.zeros(4096, np.uint8)
    enc = A.zke_encoded_out(infos.ctypes.data, 2, data.ctypes.data, 4096, 0, 0)
    t = C.c_uint64()
    call = lambda e, inp, o=out.ctypes.data, en=enc, tk=t: lib.zke_verify_emails_encoded_async(
        e, refs, 2, C.byref(inp) if inp is not None else None, o, C.byref(en) if en is not None else None, C.byref(tk) if tk is not None else None)
    assert call(None, None) == E_ARG and lib.zke_verify_emails_encoded(None, refs, 2, None, out.ctypes.data, C.byref(enc)) == E_ARG
    assert call(FAKE, None, en=None) == E_ARG and call(FAKE, None, tk=None) == E_ARG and call(FAKE, None, o=None) == E_ARG
    lists, mixed = A.zke_regex_lists(), A.MixedLists([], [A.CONFIG_NONE, A.CONFIG_NONE])
    both = A.zke_encode_in(C.pointer(lists), C.pointer(mixed.c), None, None, None)
    assert call(FAKE, both) == E_ARG and b"both" in lib.zke_last_error(None)
    ext = A.StringTable([["n", "v"], ["name", "value"]])
    dmg = ext.off.copy(); dmg[1] = 9
    assert call(FAKE, A.zke_encode_in(None, None, dmg.ctypes.data, ext.str_off.ctypes.data, ext.blob.ctypes.data)) == E_ARG
    assert call(FAKE, A.zke_encode_in(None, None, ext.off.ctypes.data, None, ext.blob.ctypes.data)) == E_ARG and b"non-zero tail" in lib.zke_last_error(None)
    assert call(FAKE, A.zke_encode_in(None, None, ext.off.ctypes.data, ext.str_off.ctypes.data, None)) == E_ARG
    badcfg = A.MixedLists([], [A.CONFIG_NONE, A.CONFIG_NONE])
    badcfg.config_of[0] = 0                                                  # names no config
    assert call(FAKE, A.zke_encode_in(None, C.pointer(badcfg.c), None, None, None)) == E_ARG
    # the sizes: exact, set before anything is staged, for all three forms of `in`
    good = A.zke_encode_in(None, None, ext.off.ctypes.data, ext.str_off.ctypes.data, ext.blob.ctypes.data)
    need = [A.encoded_len(0, [1, 1]), A.encoded_len(0, [4, 5])]
    for en in (A.zke_encoded_out(infos.ctypes.data, 1, data.ctypes.data, 4096, 0, 0), A.zke_encoded_out(infos.ctypes.data, 2, data.ctypes.data, sum(need) - 1, 0, 0)):
        assert call(FAKE, good, en=en) == E_NOMEM and (en.infos_need, en.bytes_need) == (2, sum(need))
    caps = A.StringTable([["cap0"], [], ["c"], ["dd", "e"]])                # 2 e-mails x 2 parts
    ids = np.array([0, 1], np.uint32)
    lists.n_header_parts, lists.header_part_ids, lists.n_body_parts, lists.body_part_ids = 1, ids.ctypes.data, 1, ids.ctypes.data + 4
    lists.cap_off, lists.cap_str_off, lists.cap_blob = caps.off.ctypes.data, caps.str_off.ctypes.data, caps.blob.ctypes.data
    en = A.zke_encoded_out()
    assert call(FAKE, A.zke_encode_in(C.pointer(lists), None, ext.off.ctypes.data, ext.str_off.ctypes.data, ext.blob.ctypes.data), en=en) == E_NOMEM
    assert en.bytes_need == A.encoded_len(1, [1, 1], [4]) + A.encoded_len(1, [4, 5], [1, 2, 1])
    mx = A.MixedLists([([0], [1])], [A.CONFIG_NONE, 0], [None, [["x"], ["yy", "z"]]])
    en = A.zke_encoded_out()
    assert call(FAKE, A.zke_encode_in(None, C.pointer(mx.c), None, None, None), en=en) == E_NOMEM
    assert en.bytes_need == A.encoded_len(0, []) + A.encoded_len(1, [], [1, 2, 1])
