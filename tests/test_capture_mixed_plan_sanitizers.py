"""CPU: the ragged half of the host plan of a mixed extraction (zkemail.rs_amd/csrc/mixed_plan.hip.h: capmix_plan_check,
capmix_plan_build, capmix_image) under AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/capture_mixed_plan_fuzz.cpp): random
configs and config_of arrays, the ragged offsets against a naive recomputation, every ZKE_E_ARG condition refused before a write, the
column limit at 2^20 - 1 and 2^20.  A stand-alone program with its own main(), built exactly as tests/test_mixed_plan_sanitizers.py
builds its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_capture_mixed_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "capture_mixed_plan_fuzz"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
           os.path.join(HERE, "cpp", "capture_mixed_plan_fuzz.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "capture_mixed_plan_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])
