"""CPU: the serial UTF-8 repair (zkemail.rs_amd/csrc/utf8_lossy.hip.h: utf8_lossy_len, utf8_lossy_write — String::from_utf8_lossy,
helpers/src/regex.rs:35) under AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/utf8_lossy_fuzz.cpp), byte for byte against
Python's decode("utf-8", "replace"): the Unicode standard's example, every 1- and 2-byte string, every 3- and 4-byte string over the
boundary alphabet of Table 3-7 (345 600), 2 000 seeded random strings of 0..200 bytes from that alphabet.  Each case is read from and
written into heap blocks of exactly its size.  A stand-alone program with its own main(), built with the flags of
tests/test_encode_plan_sanitizers.py; the header's serial half makes no HIP call and the program compiles nothing else of it."""
import os
import shutil
import struct
import subprocess

import pytest

import utf8_lossy_cases as U

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_reference_is_the_rule_of_from_utf8_lossy():
    """The pins that do not come from Python: the test reference reads them as the Unicode standard and Utf8Chunks do."""
    for src, want in U.pins():
        assert U.reference(src) == want, src.hex()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_utf8_lossy_under_asan_ubsan(tmp_path):
    exe = tmp_path / "utf8_lossy_fuzz"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
           os.path.join(HERE, "cpp", "utf8_lossy_fuzz.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    cases = [p[0] for p in U.pins()] + U.exhaustive_short() + U.exhaustive_alphabet() + U.random_strings()
    assert len(cases) == 5 + 1 + 256 + 65536 + 24 ** 3 + 24 ** 4 + 2000
    tape = b"".join(struct.pack("<I", len(c)) + c for c in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], input=tape, capture_output=True, timeout=600, env=env)
    tail = ("utf8_lossy_fuzz ok %d\n" % len(cases)).encode()
    assert r.returncode == 0 and r.stdout.endswith(tail), (r.stdout[-200:], r.stderr[-4000:])
    out, at = r.stdout[:-len(tail)], 0
    for c in cases:
        (n,) = struct.unpack_from("<I", out, at)
        got = out[at + 4:at + 4 + n]
        assert got == U.reference(c), (c.hex(), got.hex())
        at += 4 + n
    assert at == len(out)
