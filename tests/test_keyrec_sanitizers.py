"""CPU: the host side of the key-record entry points under AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/keyrec_fuzz.cpp):
the argument checks of zke_decode_key_records / zke_select_keys_from_records, which come before anything is staged, and the
delivery of a decode into caller-sized buffers (exact need, ZKE_E_NOMEM, a second call succeeds).  The engine's translation unit is
compiled with host sanitizers; device code is built but never run.  One build, about a minute."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_keyrec_host_side_under_asan_ubsan(tmp_path):
    exe = tmp_path / "keyrec_fuzz"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DZKE_BUILD", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "zkemail.rs_amd", "csrc"), "-Wno-unused-function", "-o", str(exe), os.path.join(HERE, "cpp", "keyrec_fuzz.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "keyrec_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])
