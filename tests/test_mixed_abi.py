"""CPU (-m "not gpu"): the C-ABI of mixed regex batches (zke_verify_emails_mixed): the two symbols, the struct sizes in the header,
the ctypes mirror and the Rust sys crate, the argument checks that come before anything touches a GPU, and the tables the Python
packer builds for a hand-written three-config list."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_sys as g  # noqa: E402

E_ARG = -1


def test_symbols_are_exported_and_abi_version_stays():
    build.build_engine()
    lib = C.CDLL(build.ENGINE_SO)
    for name in ("zke_verify_emails_mixed", "zke_verify_emails_mixed_async"):
        assert hasattr(lib, name) and name in engine.EXPORTED_SYMBOLS
    lib.zke_abi_version.restype = C.c_uint32
    assert lib.zke_abi_version() == 3                      # additive: no existing struct changes


def test_struct_sizes_agree_between_header_ctypes_and_rust(tmp_path):
    """sizeof / offsetof as the C compiler lays the header out, against ctypes; field for field against the generated Rust."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkemail_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(zke_regex_config), sizeof(zke_regex_mixed), offsetof(zke_regex_config, n_body_parts),\n'
                   '         offsetof(zke_regex_mixed, config_of), offsetof(zke_regex_mixed, cap_blob), sizeof(zke_regex_lists), sizeof(zke_email_ref));\n'
                   '  printf("%u %u %u\\n", ZKE_MIXED_MAX_CONFIGS, ZKE_MIXED_MAX_PARTS, ZKE_CONFIG_NONE);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    b = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out[:7]] == [C.sizeof(A.zke_regex_config), C.sizeof(A.zke_regex_mixed), A.zke_regex_config.n_body_parts.offset,
                                         A.zke_regex_mixed.config_of.offset, A.zke_regex_mixed.cap_blob.offset, C.sizeof(A.zke_regex_lists),
                                         C.sizeof(A.zke_email_ref)]
    assert [int(x) for x in out[:2]] == [32, 48] and [int(x) for x in out[5:7]] == [56, 56]       # the older structs keep their sizes
    assert [int(x) for x in out[7:]] == [A.MIXED_MAX_CONFIGS, A.MIXED_MAX_PARTS, A.CONFIG_NONE] == [64, 64, 0xFFFFFFFF]
    rs = open(os.path.join(ROOT, "bindings", "zkemail-amd-sys", "src", "lib.rs")).read()
    assert rs == g.generate()
    structs = {m.group(1): re.findall(r"pub ([\w#]+): ([^,\n]+),", m.group(2))
               for m in re.finditer(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct (\w+) \{(.*?)\n\}", rs, flags=re.S)}
    width = {"u32": 4}
    for name in ("zke_regex_config", "zke_regex_mixed"):
        py = getattr(A, name)._fields_
        assert [f for f, _ in structs[name]] == [f for f, _ in py], name
        size = 0
        for (_, rt), (_, pt) in zip(structs[name], py):        # repr(C): natural alignment, as the C compiler
            w = 8 if rt.startswith("*") else width[rt]
            assert w == C.sizeof(pt), (name, rt)
            size = (size + w - 1) // w * w + w
        assert (size + 7) // 8 * 8 == C.sizeof(getattr(A, name)), name
    assert ("configs", "*const zke_regex_config") in structs["zke_regex_mixed"] and ("config_of", "*const u32") in structs["zke_regex_mixed"]
    assert "pub const ZKE_CONFIG_NONE: u32 = 4294967295;" in rs and "pub const ZKE_MIXED_MAX_CONFIGS: u32 = 64;" in rs
    ext = re.search(r'extern "C" \{(.*?)\n\}', rs, flags=re.S).group(1)
    assert "pub fn zke_verify_emails_mixed(e: *mut zke_engine, emails: *const zke_email_ref, n: u32, mixed: *const zke_regex_mixed, out: *mut zke_result) -> c_int;" in ext
    assert "pub fn zke_verify_emails_mixed_async(e: *mut zke_engine, emails: *const zke_email_ref, n: u32, mixed: *const zke_regex_mixed, out: *mut zke_result, ticket: *mut u64) -> c_int;" in ext
    core = open(os.path.join(ROOT, "bindings", "zkemail-core-amd", "src", "lib.rs")).read()
    assert "pub fn verify_emails_mixed(" in core and "sys::zke_verify_emails_mixed(" in core


def test_null_and_out_of_range_arguments_are_refused():
    """The engine handle is looked at first (null: ZKE_E_ARG, nothing dereferenced)."""
    lib = engine.load_library()
    refs = A.EmailRefs([A.Email("example.com", b"From: a@example.com\r\n\r\nx\r\n", A.PublicKey(b"k"))])
    out = np.zeros(1, dtype=A.RESULT_DTYPE)
    ml = A.MixedLists([([1], [2])], [0], [[["a"], []]])
    t = C.c_uint64()
    assert lib.zke_verify_emails_mixed(None, refs.arr, 1, C.byref(ml.c), out.ctypes.data) == E_ARG
    assert lib.zke_verify_emails_mixed(None, None, 0, None, None) == E_ARG
    assert lib.zke_verify_emails_mixed_async(None, refs.arr, 1, C.byref(ml.c), out.ctypes.data, C.byref(t)) == E_ARG
    assert lib.zke_verify_emails_mixed_async(None, refs.arr, 1, C.byref(ml.c), out.ctypes.data, None) == E_ARG
    ml.config_of[0] = 7                                       # out of range (with an engine: tests/test_gpu_mixed_regex.py, test_call_failures)
    assert lib.zke_verify_emails_mixed(None, refs.arr, 1, C.byref(ml.c), out.ctypes.data) == E_ARG
    with pytest.raises(IndexError):
        A.MixedLists([([1], [2])], [7], None)                 # the packer's own tables need a config that exists


def test_packer_tables_for_a_three_config_list():
    """Engine.pack_mixed over a hand-written list: configs by equal id lists in order of first appearance, CONFIG_NONE for a plain
    Email, job_off the prefix sum of the part counts, the capture CSR e-mail-major with header parts first."""
    d = [A.DFA(b"fwd%d" % k, b"bwd%d" % k) for k in range(4)]
    ids = {}

    class Packer(engine.Engine):                              # the packer alone: ids are handed out in order of first registration
        def __init__(self):
            pass

        def dfa_register(self, fwd, bwd):
            return ids.setdefault((bytes(fwd), bytes(bwd)), 10 + len(ids))

    em = [A.Email("example.com", b"raw%d" % k, A.PublicKey(b"key")) for k in range(7)]
    cr = A.CompiledRegex
    inputs = [
        A.EmailWithRegex(em[0], A.RegexInfo([cr(d[0], ["a", "bc"])], [cr(d[1], None)])),             # config 0: H [10] B [11]
        em[1],                                                                                       # no config
        A.EmailWithRegex(em[2], A.RegexInfo(None, [cr(d[2], ["x"]), cr(d[0], []), cr(d[1], ["y", "", "zz"])])),   # config 1: B [12, 10, 11]
        A.EmailWithRegex(em[3], A.RegexInfo([cr(d[0], [])], [cr(d[1], ["q"])])),                     # config 0 again
        A.EmailWithRegex(em[4], A.RegexInfo(None, None)),                                            # config 2: zero parts
        A.EmailWithRegex(em[5], A.RegexInfo([cr(d[1], ["h"])], [cr(d[0], ["w"])])),                  # config 3: the ids of config 0, sides swapped
        A.EmailWithRegex(em[6], A.RegexInfo([], [cr(d[2], ["x2"]), cr(d[0], ["é"]), cr(d[1], None)])),   # config 1 again ([] = no header parts)
    ]
    ml = Packer().pack_mixed(inputs)
    assert ml.configs == [([10], [11]), ([], [12, 10, 11]), ([], []), ([11], [10])]
    assert list(ml.config_of) == [0, A.CONFIG_NONE, 1, 0, 2, 3, 1]
    assert list(ml.job_off) == [0, 2, 2, 5, 7, 7, 9, 12]
    assert list(ml.cap_off) == [0, 2, 2, 3, 3, 6, 6, 7, 8, 9, 10, 11, 11]
    blob = bytes(ml.cap_blob)
    strs = [blob[ml.cap_str_off[k]:ml.cap_str_off[k + 1]] for k in range(len(ml.cap_str_off) - 1)]
    assert strs == [b"a", b"bc", b"x", b"y", b"", b"zz", b"q", b"h", b"w", b"x2", "é".encode(), ]
    c = ml.c
    assert c.n_configs == 4 and c.cap_off == ml.cap_off.ctypes.data and c.config_of == ml.config_of.ctypes.data
    assert [(c.configs[k].n_header_parts, c.configs[k].n_body_parts) for k in range(4)] == [(1, 1), (0, 3), (0, 0), (1, 1)]
    assert C.cast(c.configs[1].body_part_ids, C.POINTER(C.c_uint32))[0:3] == [12, 10, 11]
    # nothing but plain e-mails: no configs, no capture table
    ml0 = Packer().pack_mixed(em[:2])
    assert ml0.c.n_configs == 0 and not ml0.c.cap_off and list(ml0.job_off) == [0, 0, 0]
    # pack_with_regex keeps refusing a mixed list
    with pytest.raises(engine.EngineError, match="share one part list"):
        Packer().pack_with_regex([inputs[0], inputs[2]])
