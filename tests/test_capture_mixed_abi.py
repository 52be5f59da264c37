"""CPU (-m "not gpu"): the C-ABI of mixed extractions (zke_extract_captures_mixed): the two symbols, the struct sizes and offsets in the
header, the ctypes mirror and the Rust sys crate, the packer's deduplication by content, and J / Gt / job_off / col_off on a
hand-written example."""
import ctypes as C
import os
import re
import subprocess
import sys

from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import build, engine
from zkemail_rs_amd import regex_compile as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_sys as g  # noqa: E402


def test_symbols_are_exported_and_abi_version_stays():
    build.build_engine()
    lib = C.CDLL(build.ENGINE_SO)
    for name in ("zke_extract_captures_mixed", "zke_extract_captures_mixed_async"):
        assert hasattr(lib, name) and name in engine.EXPORTED_SYMBOLS
    lib.zke_abi_version.restype = C.c_uint32
    assert lib.zke_abi_version() == 3                      # additive: no existing struct changes
    # the engine handle is looked at first: null is ZKE_E_ARG, nothing is dereferenced
    assert lib.zke_extract_captures_mixed(None, None, 0, None, None, None, None) == -1
    assert lib.zke_extract_captures_mixed_async(None, None, 0, None, None, None, None, None) == -1


def test_struct_sizes_agree_between_header_ctypes_and_rust(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkemail_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(zke_capture_config), sizeof(zke_capture_mixed),\n'
                   '         offsetof(zke_capture_config, header_parts), offsetof(zke_capture_config, n_body_parts), offsetof(zke_capture_config, body_parts),\n'
                   '         offsetof(zke_capture_mixed, configs), offsetof(zke_capture_mixed, config_of), sizeof(zke_capture_part), sizeof(zke_capture_out));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    b = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    cc, cm = A.zke_capture_config, A.zke_capture_mixed
    assert out == [C.sizeof(cc), C.sizeof(cm), cc.header_parts.offset, cc.n_body_parts.offset, cc.body_parts.offset, cm.configs.offset,
                   cm.config_of.offset, C.sizeof(A.zke_capture_part), C.sizeof(A.zke_capture_out)]
    assert out[:2] == [32, 24] and out[7:] == [24, 128]          # the older structs keep their sizes
    rs = open(os.path.join(ROOT, "bindings", "zkemail-amd-sys", "src", "lib.rs")).read()
    assert rs == g.generate()
    structs = {m.group(1): re.findall(r"pub ([\w#]+): ([^,\n]+),", m.group(2))
               for m in re.finditer(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct (\w+) \{(.*?)\n\}", rs, flags=re.S)}
    for name in ("zke_capture_config", "zke_capture_mixed"):
        py = getattr(A, name)._fields_
        assert [f for f, _ in structs[name]] == [f for f, _ in py], name
        size = 0
        for (_, rt), (_, pt) in zip(structs[name], py):        # repr(C): natural alignment, as the C compiler
            w = 8 if rt.startswith("*") else {"u32": 4}[rt]
            assert w == C.sizeof(pt), (name, rt)
            size = (size + w - 1) // w * w + w
        assert (size + 7) // 8 * 8 == C.sizeof(getattr(A, name)), name
    assert ("header_parts", "*const zke_capture_part") in structs["zke_capture_config"]
    assert ("configs", "*const zke_capture_config") in structs["zke_capture_mixed"] and ("config_of", "*const u32") in structs["zke_capture_mixed"]
    ext = re.search(r'extern "C" \{(.*?)\n\}', rs, flags=re.S).group(1)
    assert ("pub fn zke_extract_captures_mixed(e: *mut zke_engine, emails: *const zke_email_ref, n: u32, mixed: *const zke_capture_mixed, "
            "out: *mut zke_result, caps: *mut zke_capture_out, org: *mut zke_capture_origin) -> c_int;") in ext
    assert ("pub fn zke_extract_captures_mixed_async(e: *mut zke_engine, emails: *const zke_email_ref, n: u32, mixed: *const zke_capture_mixed, "
            "out: *mut zke_result, caps: *mut zke_capture_out, org: *mut zke_capture_origin, ticket: *mut u64) -> c_int;") in ext
    core = open(os.path.join(ROOT, "bindings", "zkemail-core-amd", "src", "lib.rs")).read()
    assert "pub fn extract_captures_mixed(" in core and "sys::zke_extract_captures_mixed(" in core
    hpp = open(os.path.join(ROOT, "include", "zkemail_core.hpp")).read()
    assert "extract_captures_mixed(" in hpp and "zke_extract_captures_mixed(e_," in hpp


class Packer(engine.Engine):
    """The packer alone: ids are handed out in order of first compilation, nothing touches a GPU."""

    def __init__(self):
        self.ids = {}

    def compile_pattern(self, pattern, unicode=True):
        k = self.ids.setdefault((pattern, bool(unicode)), len(self.ids))
        return (A.DFA(b"f%d" % k, b"b%d" % k), 100 + k, 200 + k)


def test_packer_dedups_by_content_and_lays_the_ragged_tables_out():
    P = rc.RegexPattern
    a = rc.RegexConfig([P("from:(x)", [1])], [P("body(a)(b)", [1, 2]), P("tok", [0])])          # P = 3, G = 4
    a_again = rc.RegexConfig.from_json({"header_parts": [{"pattern": "from:(x)", "capture_indices": [1]}],
                                        "body_parts": [{"pattern": "body(a)(b)", "capture_indices": [1, 2]}, {"pattern": "tok", "capture_indices": [0]}]})
    other_groups = rc.RegexConfig([P("from:(x)", [0])], [P("body(a)(b)", [1, 2]), P("tok", [0])])  # the same patterns, other indices: distinct
    gzero = rc.RegexConfig([P("subj", []), P("from:(x)", None)], None)                            # P = 2, G = 0
    cfgs = [a, None, gzero, a_again, other_groups, None, a]
    lists, distinct = Packer().pack_capture_mixed(cfgs, unicode=False)
    assert distinct == [a, gzero, other_groups]
    assert list(lists.config_of) == [0, A.CONFIG_NONE, 1, 0, 2, A.CONFIG_NONE, 0]
    assert lists.configs[0] == ([(100, 200, [1])], [(101, 201, [1, 2]), (102, 202, [0])])
    assert lists.configs[1] == ([(103, 203, []), (100, 200, [])], []) and lists.configs[2][0] == [(100, 200, [0])]
    assert lists.gbase == [[0, 1, 3, 4], [0, 0, 0], [0, 1, 3, 4]]
    assert list(lists.job_off) == [0, 3, 3, 5, 8, 11, 11, 14] and list(lists.col_off) == [0, 4, 4, 4, 8, 12, 12, 16]
    assert (lists.J, lists.Gt) == (14, 16)
    c = lists.c
    assert c.n_configs == 3 and c.config_of == lists.config_of.ctypes.data
    assert [(c.configs[k].n_header_parts, c.configs[k].n_body_parts) for k in range(3)] == [(1, 2), (2, 0), (1, 2)]
    body = c.configs[0].body_parts
    assert (body[0].dfa_id, body[0].prog_id, body[0].n_groups) == (101, 201, 2) and C.cast(body[0].groups, C.POINTER(C.c_uint32))[0:2] == [1, 2]
    assert (body[1].dfa_id, body[1].n_groups) == (102, 1) and c.configs[1].header_parts[1].n_groups == 0
    # a hand-written example with a None, a config with G = 0 and an unpopulated config (index 1)
    hand = A.CaptureMixedLists([([(1, 2, [1, 0])], [(3, 4, [2])]), ([(9, 9, [1])] * 5, []), ([(5, 6, []), (7, 8, [])], [])],
                               [2, 0, A.CONFIG_NONE, 0, 2])
    assert list(hand.job_off) == [0, 2, 4, 4, 6, 8] and list(hand.col_off) == [0, 0, 3, 3, 6, 6] and (hand.J, hand.Gt) == (8, 6)
    # nothing but plain e-mails: no configs, no jobs, no columns
    none = Packer().pack_capture_mixed([None, None], unicode=False)[0]
    assert none.c.n_configs == 0 and (none.J, none.Gt) == (0, 0) and list(none.job_off) == [0, 0, 0]
