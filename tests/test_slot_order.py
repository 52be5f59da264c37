"""CPU: the ticket order over the hardware queues the slot streams share (zkemail.rs_amd/csrc/slot_order.hip.h) under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/cpp/slot_order_test.cpp): every slot count 1 .. 64 split into 1 .. 8 groups of sizes differing by at
most 2, the splits HIP's queue pool produces (6/6/5/5, 5/5/4/4, 4/4/4/4) and an uneven 7/1 — an unknown map and all-singleton groups give
t % slots; any n_queues consecutive tickets hit every queue once; a queue's slots come round in ascending order; every slot is used
within n_queues x max count tickets; the sequence is continuous across 2^32.  A stand-alone program with its own main(), built with the
flags of tests/test_mixed_plan_sanitizers.py; the header makes no HIP call, so the build takes seconds."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_slot_order_under_asan_ubsan(tmp_path):
    exe = tmp_path / "slot_order_test"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
           os.path.join(HERE, "cpp", "slot_order_test.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "slot_order_test ok" in r.stdout, (r.stdout[-500:], r.stderr[-4000:])
