"""CPU: the host side of zke_extract_bodies under AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/body_fuzz.cpp): the
argument checks, which come before anything is staged, the buffer layout, and the compaction of an extraction into caller-sized
buffers (first and second places, exact need, ZKE_E_NOMEM, hostile info tables refused or served inside the buffer).  A stand-alone
program with its own main(): the engine's translation unit compiled with host sanitizers; device code is built but never run.
One build, about a minute."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_body_host_side_under_asan_ubsan(tmp_path):
    exe = tmp_path / "body_fuzz"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DZKE_BUILD", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "zkemail.rs_amd", "csrc"), "-Wno-unused-function", "-o", str(exe), os.path.join(HERE, "cpp", "body_fuzz.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "body_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])
