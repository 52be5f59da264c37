"""CPU: the host plan of an output encoding (zkemail.rs_amd/csrc/encode_plan.hip.h) under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/cpp/encode_plan_fuzz.cpp): random tables in the three row shapes — jobs that name exactly their
e-mail's strings, lengths equal to a word-by-word writer's, places without a gap, every encoding written inside a heap block of
exactly the planned size — and damaged ones: decreasing offsets, a null table with a non-zero tail, both list forms, an encoding
that reaches 2^32 bytes, a total that leaves 64 bits, each refused before a write.  A stand-alone program with its own main(), built
with the flags of tests/test_mixed_plan_sanitizers.py; the plan header makes no HIP call, so there is no device code in it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_encode_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "encode_plan_fuzz"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
           os.path.join(HERE, "cpp", "encode_plan_fuzz.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "encode_plan_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])
