"""CPU: the host-side reader of capture programs under AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/capture_fuzz.cpp),
the way tests/test_host_sanitizers.py drives the DFA blob reader: the engine's translation unit compiled with host sanitizers
(device code is built but never run), the golden programs truncated, bit-flipped and randomly substituted.  One build, ≈45 s."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_capture_program_reader_under_asan_ubsan(tmp_path):
    exe = tmp_path / "capture_fuzz"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DZKE_BUILD", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "zkemail.rs_amd", "csrc"), "-Wno-unused-function", "-o", str(exe), os.path.join(HERE, "cpp", "capture_fuzz.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    g = os.path.join(HERE, "golden")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)] + [os.path.join(g, n) for n in ("capture_from_header.zkcp", "capture_alternation.zkcp", "capture_unicode_lazy.zkcp")],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "capture_fuzz ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])
