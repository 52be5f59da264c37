"""In-tree builds: the HIP engine (hipcc, gfx950) and the CPU oracle (gcc).

``python -m zkemail_rs_amd.build`` or ``__graft_entry__.build()``.  Outputs stay in the tree
(``zkemail.rs_amd/libzkemail_amd.so``, ``oracle/libzke_oracle.so``) so they travel to the GPU
box with the snapshot; they are git-ignored.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
ENGINE_SO = os.path.join(PKG, "libzkemail_amd.so")
ORACLE_SO = os.path.join(ROOT, "oracle", "libzke_oracle.so")

ENGINE_SOURCES = ["engine.hip"]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _deps(dirpath: str):
    out = []
    for base, _, files in os.walk(dirpath):
        out += [os.path.join(base, f) for f in files if f.endswith((".hip", ".h", ".hpp", ".c", ".cpp"))]
    return out


def build_engine(force: bool = False, verbose: bool = False) -> str:
    deps = _deps(CSRC) + _deps(os.path.join(ROOT, "include"))
    if not force and not _newer(ENGINE_SO, deps):
        return ENGINE_SO
    srcs = [os.path.join(CSRC, s) for s in ENGINE_SOURCES]
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DZKE_BUILD",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-Wall", "-Wno-unused-function",
           "-o", ENGINE_SO] + srcs
    if verbose:
        cmd[1:1] = ["-Rpass-analysis=kernel-resource-usage", "-DZKE_LIST_GROUP_KERNELS"]     # rsa_group_kernel<4> / <8> listed too
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed building libzkemail_amd.so")
    if verbose:
        sys.stderr.write(r.stderr)
    return ENGINE_SO


def build_oracle(force: bool = False) -> str:
    srcs = [os.path.join(ROOT, "oracle", "zke_oracle.c"), os.path.join(ROOT, "oracle", "zke_ed25519.c")]
    deps = srcs + [os.path.join(ROOT, "oracle", "zke_oracle.h"), os.path.join(ROOT, "include", "zkemail_amd.h")]
    if not force and not _newer(ORACLE_SO, deps):
        return ORACLE_SO
    cmd = ["gcc", "-O3", "-fPIC", "-shared", "-pthread", "-Wall", "-Wextra", "-o", ORACLE_SO] + srcs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("gcc failed building libzke_oracle.so")
    return ORACLE_SO


CPP_EXAMPLE = os.path.join(ROOT, "tests", "cpp", "mirror_test")
CPP_SIGSCAN = os.path.join(ROOT, "tests", "cpp", "sigscan_test")
CPP_KEYREC = os.path.join(ROOT, "tests", "cpp", "keyrec_test")
CPP_QPMAP = os.path.join(ROOT, "tests", "cpp", "qpmap_test")
CPP_BODY = os.path.join(ROOT, "tests", "cpp", "body_test")
CPP_MIXED = os.path.join(ROOT, "tests", "cpp", "mixed_test")
CPP_ENCODE = os.path.join(ROOT, "tests", "cpp", "encode_test")
CPP_EXTRACT_ENCODED = os.path.join(ROOT, "tests", "cpp", "extract_encoded_test")
ED_PROBE = os.path.join(ROOT, "tests", "cpp", "ed_probe")
SHA_PROBE = os.path.join(ROOT, "tests", "cpp", "sha_probe")


def _build_cpp(exe: str, force: bool) -> str:
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "include", "zkemail_core.hpp"), os.path.join(ROOT, "include", "zkemail_amd.h"), ENGINE_SO]
    if not force and not _newer(exe, deps):
        return exe
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
           "-L", PKG, "-lzkemail_amd", "-L", "/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("g++ failed building " + os.path.relpath(exe, ROOT))
    return exe


def build_cpp_example(force: bool = False) -> str:
    """The C++ host mirror (include/zkemail_core.hpp) compiled against the built library: the verify program, whose path is
    returned, the generator program (build_cpp_sigscan), the key-record program (build_cpp_keyrec) and the index-map program
    (build_cpp_qpmap); and the Ed25519 probe (build_ed_probe), which needs no library."""
    build_cpp_sigscan(force)
    build_cpp_keyrec(force)
    if os.path.exists(CPP_QPMAP + ".cpp"):
        build_cpp_qpmap(force)
    if os.path.exists(CPP_BODY + ".cpp"):
        build_cpp_body(force)
    if os.path.exists(CPP_MIXED + ".cpp"):
        build_cpp_mixed(force)
    if os.path.exists(CPP_ENCODE + ".cpp"):
        build_cpp_encode(force)
    if os.path.exists(CPP_EXTRACT_ENCODED + ".cpp"):
        build_cpp_extract_encoded(force)
    if os.path.exists(ED_PROBE + ".hip"):      # test infrastructure that lives in tests/: a tree whose tests/ does not carry the probe
        build_ed_probe(force)                   # has nothing that runs it, and the three programs below do not depend on it
    if os.path.exists(SHA_PROBE + ".hip"):
        build_sha_probe(force)
    return _build_cpp(CPP_EXAMPLE, force)


def build_cpp_sigscan(force: bool = False) -> str:
    """tests/cpp/sigscan_test: scan_signatures / select_keys / generate_email_inputs of the C++ mirror."""
    return _build_cpp(CPP_SIGSCAN, force)


def build_cpp_keyrec(force: bool = False) -> str:
    """tests/cpp/keyrec_test: decode_key_records / generate_email_inputs_from_records of the C++ mirror."""
    return _build_cpp(CPP_KEYREC, force)


def build_cpp_qpmap(force: bool = False) -> str:
    """tests/cpp/qpmap_test: remove_quoted_printable_soft_breaks and the extract_captures overload with origins of the C++ mirror."""
    return _build_cpp(CPP_QPMAP, force)


def build_cpp_body(force: bool = False) -> str:
    """tests/cpp/body_test: extract_email_bodies / extract_email_body of the C++ mirror."""
    return _build_cpp(CPP_BODY, force)


def build_cpp_mixed(force: bool = False) -> str:
    """tests/cpp/mixed_test: verify_emails_mixed of the C++ mirror."""
    return _build_cpp(CPP_MIXED, force)


def build_cpp_encode(force: bool = False) -> str:
    """tests/cpp/encode_test: verify_emails_encoded / verify_emails_with_regex_encoded of the C++ mirror."""
    return _build_cpp(CPP_ENCODE, force)


def build_cpp_extract_encoded(force: bool = False) -> str:
    """tests/cpp/extract_encoded_test: extract_captures_encoded / utf8_lossy of the C++ mirror."""
    return _build_cpp(CPP_EXTRACT_ENCODED, force)


def build_ed_probe(force: bool = False) -> str:
    """tests/cpp/ed_probe: the device routines of csrc/ed25519.hip.h, one per case of a tape (tests/ed_field_cases.py).  A stand-alone
    HIP program compiled from the product header with the engine's target and optimisation flags; it does not link the library.
    Called directly (tests/test_gpu_ed_field.py) it raises when the source is missing."""
    src = ED_PROBE + ".hip"
    if not os.path.exists(src):
        raise RuntimeError("tests/cpp/ed_probe.hip is missing")
    deps = [src] + [d for d in _deps(CSRC) if d.endswith(".h")] + _deps(os.path.join(ROOT, "include"))
    if not force and not _newer(ED_PROBE, deps):
        return ED_PROBE
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-Wall", "-Wno-unused-function", "-o", ED_PROBE, src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed building tests/cpp/ed_probe")
    return ED_PROBE


def build_sha_probe(force: bool = False, stamps: bool = True) -> str:
    """tests/cpp/sha_probe: the two-role SHA-256 routines of csrc/sha256.hip.h alone on 1 024 messages of 4 KB, timed
    (tools/sha_timeline.py).  Stand-alone like the Ed25519 probe.  `stamps`: compiled with ZKE_SHA_PROBE, the routines record where
    their waves ran and when they met each barrier; without, tests/cpp/sha_probe_plain runs the code the library runs."""
    src = SHA_PROBE + ".hip"
    if not os.path.exists(src):
        raise RuntimeError("tests/cpp/sha_probe.hip is missing")
    exe = SHA_PROBE if stamps else SHA_PROBE + "_plain"
    deps = [src] + [d for d in _deps(CSRC) if d.endswith(".h")]
    if not force and not _newer(exe, deps):
        return exe
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-Wall", "-Wno-unused-function", "-o", exe, src] + (["-DZKE_SHA_PROBE"] if stamps else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed building tests/cpp/sha_probe")
    return exe


SHA_TWIN_PROBE = os.path.join(ROOT, "tests", "cpp", "sha_twin_probe")


def build_sha_twin_probe(force: bool = False, stamps: bool = True) -> str:
    """tests/cpp/sha_twin_probe: sha256_ring_kernel against sha256_twin_kernel on the messages of sha_probe
    (tools/sha_twin_timeline.py).  Built on request only, with the flags of build_sha_probe."""
    src = SHA_TWIN_PROBE + ".hip"
    exe = SHA_TWIN_PROBE if stamps else SHA_TWIN_PROBE + "_plain"
    deps = [src] + [d for d in _deps(CSRC) if d.endswith(".h")]
    if not force and not _newer(exe, deps):
        return exe
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-Wall", "-Wno-unused-function", "-o", exe, src] + (["-DZKE_SHA_PROBE"] if stamps else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed building tests/cpp/sha_twin_probe")
    return exe


if __name__ == "__main__":
    force = "--force" in sys.argv
    print(build_oracle(force))
    print(build_engine(force, verbose="-v" in sys.argv))
    print(build_cpp_example(force))
