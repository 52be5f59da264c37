"""ctypes binding of libzkemail_amd.so and the Python mirror of ``verify_email`` /
``verify_email_with_regex`` (core/src/circuits.rs:9-68).

The mirror keeps the reference's names, argument meaning and error behaviour: where the
reference panics (``assert!`` / ``unwrap`` / ``expect``) these raise :class:`VerifyPanic`
carrying the status that names the panic site.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _abi as A
from ._abi import (CompiledRegex, DebugBuffers, Email, EmailVerifierOutput, EmailWithRegex,
                   EmailWithRegexVerifierOutput, PackedBatch)

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("ZKE_LIB") or os.path.join(_PKG, "libzkemail_amd.so")   # ZKE_LIB: A/B runs of two builds
_lib = None


class EngineError(RuntimeError):
    """The C-ABI call itself failed (bad arguments, no device, library missing)."""


class VerifyPanic(AssertionError):
    """The reference would have panicked on this e-mail (status names the site)."""

    def __init__(self, status: int, detail: int, index: int = 0):
        self.status, self.detail, self.index = status, detail, index
        super().__init__(f"email {index}: {A.STATUS_NAMES.get(status, status)} (detail {detail}) — "
                         f"reference panics at {A.STATUS_SITE.get(status, '?')}")


def load_library(path: Optional[str] = None):
    """Load the HIP engine.  Fails loudly: there is no CPU implementation behind this API."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or _LIB_PATH
    if not os.path.exists(p):
        raise EngineError(f"{p} not built — run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(p)
    vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)
    lib.zke_engine_create.argtypes = [C.POINTER(A.zke_options), C.POINTER(vp)]
    lib.zke_engine_create.restype = C.c_int
    lib.zke_engine_destroy.argtypes = [vp]
    lib.zke_engine_destroy.restype = None
    lib.zke_last_error.argtypes = [vp]
    lib.zke_last_error.restype = C.c_char_p
    lib.zke_dfa_register.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, u32p]
    lib.zke_dfa_register.restype = C.c_int
    lib.zke_verify_batch.argtypes = [vp, C.POINTER(A.zke_batch), vp, C.POINTER(A.zke_debug_out)]
    lib.zke_verify_batch.restype = C.c_int
    lib.zke_verify_batch_async.argtypes = [vp, C.POINTER(A.zke_batch), vp, C.POINTER(C.c_uint64)]
    lib.zke_verify_batch_async.restype = C.c_int
    lib.zke_batch_wait.argtypes = [vp, C.c_uint64]
    lib.zke_batch_wait.restype = C.c_int
    lib.zke_verify_emails.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, vp]
    lib.zke_verify_emails.restype = C.c_int
    lib.zke_verify_emails_async.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, vp, C.POINTER(C.c_uint64)]
    lib.zke_verify_emails_async.restype = C.c_int
    lib.zke_verify_emails_with_regex.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, C.POINTER(A.zke_regex_lists), vp]
    lib.zke_verify_emails_with_regex.restype = C.c_int
    lib.zke_verify_emails_with_regex_async.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, C.POINTER(A.zke_regex_lists), vp, C.POINTER(C.c_uint64)]
    lib.zke_verify_emails_with_regex_async.restype = C.c_int
    if hasattr(lib, "zke_verify_emails_mixed"):     # (a ZKE_LIB build of an older tree, for an A/B run, has no such entry)
        lib.zke_verify_emails_mixed.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, C.POINTER(A.zke_regex_mixed), vp]
        lib.zke_verify_emails_mixed.restype = C.c_int
        lib.zke_verify_emails_mixed_async.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, C.POINTER(A.zke_regex_mixed), vp, C.POINTER(C.c_uint64)]
        lib.zke_verify_emails_mixed_async.restype = C.c_int
    lib.zke_status_name.argtypes = [C.c_uint32]
    lib.zke_status_name.restype = C.c_char_p
    lib.zke_dfa_status.argtypes = [vp, C.c_uint32, u32p]
    lib.zke_dfa_status.restype = C.c_int
    lib.zke_dfa_unregister.argtypes = [vp, C.c_uint32]
    lib.zke_dfa_unregister.restype = C.c_int
    lib.zke_process_init.argtypes = [C.c_uint32]
    lib.zke_process_init.restype = C.c_int
    lib.zke_abi_version.argtypes = []
    lib.zke_abi_version.restype = C.c_uint32
    lib.zke_verify_batch_device.argtypes = [vp, C.POINTER(A.zke_batch), C.c_uint64, C.c_uint64, C.c_uint64, vp, vp]
    lib.zke_verify_batch_device.restype = C.c_int
    lib.zke_engine_sync.argtypes = [vp]
    lib.zke_engine_sync.restype = C.c_int
    lib.zke_engine_join.argtypes = [vp, vp]
    lib.zke_engine_join.restype = C.c_int
    lib.zke_get_timings.argtypes = [vp, C.POINTER(A.zke_timings)]
    lib.zke_get_timings.restype = C.c_int
    lib.zke_set_timing.argtypes = [vp, C.c_int]
    lib.zke_set_timing.restype = C.c_int
    lib.zke_verify_email.argtypes = [vp, vp, C.c_size_t, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp]
    lib.zke_verify_email.restype = C.c_int
    lib.zke_verify_email_with_regex.argtypes = [vp, vp, C.c_size_t, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_uint32,
                                                C.POINTER(A.zke_regex_part), C.c_uint32, C.POINTER(A.zke_regex_part), C.c_uint32, vp]
    lib.zke_verify_email_with_regex.restype = C.c_int
    lib.zke_engine_reserve.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.zke_engine_reserve.restype = C.c_int
    lib.zke_engine_reserve_host.argtypes = [vp, C.c_uint32, C.c_uint64]
    lib.zke_engine_reserve_host.restype = C.c_int
    lib.zke_wire_decode.argtypes = [C.c_uint32, vp, C.c_size_t, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.zke_wire_decode.restype = C.c_int
    lib.zke_wire_free.argtypes = [vp]
    lib.zke_wire_free.restype = None
    lib.zke_wire_view.argtypes = [vp, C.POINTER(A.zke_wire_email)]
    lib.zke_wire_view.restype = C.c_int
    lib.zke_wire_external_input.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_size_t), u32p]
    lib.zke_wire_external_input.restype = C.c_int
    lib.zke_verify_wire.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.c_uint32, vp]
    lib.zke_verify_wire.restype = C.c_int
    lib.zke_shard_bounds.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    lib.zke_shard_bounds.restype = C.c_int
    lib.zke_get_slot_timings.argtypes = [vp, C.c_uint32, C.POINTER(A.zke_timings)]
    lib.zke_get_slot_timings.restype = C.c_int
    lib.zke_sha256_batch.argtypes = [vp, vp, vp, C.c_uint32, vp]
    lib.zke_sha256_batch.restype = C.c_int
    lib.zke_sha256_batch_device.argtypes = [vp, vp, vp, C.c_uint32, vp, vp]
    lib.zke_sha256_batch_device.restype = C.c_int
    lib.zke_rsa_modexp_batch.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp]
    lib.zke_rsa_modexp_batch.restype = C.c_int
    lib.zke_ed25519_verify_batch.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp]
    lib.zke_ed25519_verify_batch.restype = C.c_int
    lib.zke_abi_encode.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t),
                                   C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.zke_abi_encode.restype = C.c_int
    lib.zke_capture_validate.argtypes = [vp, C.c_size_t, u32p]
    lib.zke_capture_validate.restype = C.c_int
    lib.zke_capture_register.argtypes = [vp, vp, C.c_size_t, u32p]
    lib.zke_capture_register.restype = C.c_int
    lib.zke_capture_status.argtypes = [vp, C.c_uint32, u32p]
    lib.zke_capture_status.restype = C.c_int
    lib.zke_capture_unregister.argtypes = [vp, C.c_uint32]
    lib.zke_capture_unregister.restype = C.c_int
    cpp, cop = C.POINTER(A.zke_capture_part), C.POINTER(A.zke_capture_out)
    lib.zke_extract_captures.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, cpp, C.c_uint32, cpp, C.c_uint32, vp, cop]
    lib.zke_extract_captures.restype = C.c_int
    lib.zke_extract_captures_async.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, cpp, C.c_uint32, cpp, C.c_uint32, vp, cop,
                                               C.POINTER(C.c_uint64)]
    lib.zke_extract_captures_async.restype = C.c_int
    lib.zke_capture_batch.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint32, vp, cop]
    lib.zke_capture_batch.restype = C.c_int
    if hasattr(lib, "zke_qp_clean_batch"):          # (as zke_engine_sha_ring below: an older tree's library has none of the three)
        orp = C.POINTER(A.zke_capture_origin)
        lib.zke_qp_clean_batch.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp]
        lib.zke_qp_clean_batch.restype = C.c_int
        lib.zke_extract_captures_mapped.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, cpp, C.c_uint32, cpp, C.c_uint32, vp, cop, orp]
        lib.zke_extract_captures_mapped.restype = C.c_int
        lib.zke_extract_captures_mapped_async.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, cpp, C.c_uint32, cpp, C.c_uint32, vp, cop, orp,
                                                          C.POINTER(C.c_uint64)]
        lib.zke_extract_captures_mapped_async.restype = C.c_int
    if hasattr(lib, "zke_extract_captures_mixed"):  # (likewise)
        cmp_, orp = C.POINTER(A.zke_capture_mixed), C.POINTER(A.zke_capture_origin)
        lib.zke_extract_captures_mixed.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, cmp_, vp, cop, orp]
        lib.zke_extract_captures_mixed.restype = C.c_int
        lib.zke_extract_captures_mixed_async.argtypes = [vp, C.POINTER(A.zke_email_ref), C.c_uint32, cmp_, vp, cop, orp, C.POINTER(C.c_uint64)]
        lib.zke_extract_captures_mixed_async.restype = C.c_int
    erp =C.POINTER(A.zke_email_ref)
    lib.zke_scan_signatures.argtypes = [vp, erp, C.c_uint32, C.c_uint32, C.POINTER(A.zke_sig_scan)]
    lib.zke_scan_signatures.restype = C.c_int
    lib.zke_scan_signatures_async.argtypes = [vp, erp, C.c_uint32, C.c_uint32, C.POINTER(A.zke_sig_scan), C.POINTER(C.c_uint64)]
    lib.zke_scan_signatures_async.restype = C.c_int
    lib.zke_select_keys.argtypes = [vp, erp, C.c_uint32, vp, C.POINTER(A.zke_key_ref), vp, vp]
    lib.zke_select_keys.restype = C.c_int
    lib.zke_select_keys_async.argtypes = [vp, erp, C.c_uint32, vp, C.POINTER(A.zke_key_ref), vp, vp, C.POINTER(C.c_uint64)]
    lib.zke_select_keys_async.restype = C.c_int
    krp, kop = C.POINTER(A.zke_keyrec_ref), C.POINTER(A.zke_keyrec_out)
    lib.zke_decode_key_records.argtypes = [vp, krp, C.c_uint32, C.c_uint32, kop]
    lib.zke_decode_key_records.restype = C.c_int
    lib.zke_decode_key_records_async.argtypes = [vp, krp, C.c_uint32, C.c_uint32, kop, C.POINTER(C.c_uint64)]
    lib.zke_decode_key_records_async.restype = C.c_int
    lib.zke_select_keys_from_records.argtypes = [vp, erp, C.c_uint32, vp, krp, C.c_uint32, vp, vp, kop]
    lib.zke_select_keys_from_records.restype = C.c_int
    lib.zke_select_keys_from_records_async.argtypes = [vp, erp, C.c_uint32, vp, krp, C.c_uint32, vp, vp, kop, C.POINTER(C.c_uint64)]
    lib.zke_select_keys_from_records_async.restype = C.c_int
    bop = C.POINTER(A.zke_body_out)
    lib.zke_extract_bodies.argtypes = [vp, erp, C.c_uint32, C.c_uint32, bop]
    lib.zke_extract_bodies.restype = C.c_int
    lib.zke_extract_bodies_async.argtypes = [vp, erp, C.c_uint32, C.c_uint32, bop, C.POINTER(C.c_uint64)]
    lib.zke_extract_bodies_async.restype = C.c_int
    if hasattr(lib, "zke_verify_emails_encoded"):   # (a ZKE_LIB build of an older tree, for an A/B run, has none of the three)
        eip, eop = C.POINTER(A.zke_encode_in), C.POINTER(A.zke_encoded_out)
        lib.zke_verify_emails_encoded.argtypes = [vp, erp, C.c_uint32, eip, vp, eop]
        lib.zke_verify_emails_encoded.restype = C.c_int
        lib.zke_verify_emails_encoded_async.argtypes = [vp, erp, C.c_uint32, eip, vp, eop, C.POINTER(C.c_uint64)]
        lib.zke_verify_emails_encoded_async.restype = C.c_int
        lib.zke_encode_outputs.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, eop]
        lib.zke_encode_outputs.restype = C.c_int
    if hasattr(lib, "zke_utf8_lossy_batch"):        # (likewise)
        lib.zke_utf8_lossy_batch.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
        lib.zke_utf8_lossy_batch.restype = C.c_int
        eop = C.POINTER(A.zke_encoded_out)
        lib.zke_extract_captures_encoded.argtypes = [vp, erp, C.c_uint32, cpp, C.c_uint32, cpp, C.c_uint32, vp, cop, vp, vp, vp, eop]
        lib.zke_extract_captures_encoded.restype = C.c_int
        lib.zke_extract_captures_encoded_async.argtypes = lib.zke_extract_captures_encoded.argtypes + [C.POINTER(C.c_uint64)]
        lib.zke_extract_captures_encoded_async.restype = C.c_int
    if hasattr(lib, "zke_engine_sha_ring"):         # (a ZKE_LIB build of an older tree, for an A/B run, has no such entry)
        lib.zke_engine_sha_ring.argtypes = [vp]
        lib.zke_engine_sha_ring.restype = C.c_int
    if hasattr(lib, "zke_engine_sha_twin"):         # (likewise)
        lib.zke_engine_sha_twin.argtypes = [vp]
        lib.zke_engine_sha_twin.restype = C.c_int
    if hasattr(lib, "zke_engine_front_helper"):     # (likewise)
        lib.zke_engine_front_helper.argtypes = [vp, C.c_uint32]
        lib.zke_engine_front_helper.restype = C.c_int
    if hasattr(lib, "zke_engine_queue_count"):      # (likewise)
        lib.zke_engine_queue_count.argtypes = [vp]
        lib.zke_engine_queue_count.restype = C.c_int
        lib.zke_engine_slot_queue.argtypes = [vp, C.c_uint32]
        lib.zke_engine_slot_queue.restype = C.c_int
        lib.zke_engine_last_slot.argtypes = [vp]
        lib.zke_engine_last_slot.restype = C.c_int
    lib.zke_version.argtypes = []
    lib.zke_version.restype = C.c_char_p
    lib.zke_device_available.argtypes = []
    lib.zke_device_available.restype = C.c_int
    if path is None:
        _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "zke_engine_create", "zke_engine_destroy", "zke_last_error", "zke_dfa_register", "zke_verify_batch",
    "zke_verify_batch_device", "zke_engine_sync", "zke_get_timings", "zke_set_timing", "zke_verify_email",
    "zke_sha256_batch", "zke_sha256_batch_device", "zke_rsa_modexp_batch", "zke_version", "zke_device_available",
    "zke_ed25519_verify_batch", "zke_engine_reserve", "zke_get_slot_timings", "zke_verify_email_with_regex",
    "zke_abi_encode", "zke_engine_join", "zke_verify_batch_async", "zke_batch_wait", "zke_dfa_status", "zke_dfa_unregister",
    "zke_process_init", "zke_abi_version", "zke_engine_reserve_host", "zke_wire_decode", "zke_wire_free", "zke_wire_view",
    "zke_wire_external_input", "zke_verify_wire", "zke_shard_bounds", "zke_status_name", "zke_verify_emails", "zke_verify_emails_async",
    "zke_verify_emails_with_regex", "zke_verify_emails_with_regex_async", "zke_verify_emails_mixed", "zke_verify_emails_mixed_async",
    "zke_capture_validate", "zke_capture_register", "zke_capture_status", "zke_capture_unregister", "zke_extract_captures",
    "zke_extract_captures_async", "zke_capture_batch",
    "zke_scan_signatures", "zke_scan_signatures_async", "zke_select_keys", "zke_select_keys_async",
    "zke_decode_key_records", "zke_decode_key_records_async", "zke_select_keys_from_records", "zke_select_keys_from_records_async",
    "zke_engine_sha_ring", "zke_engine_sha_twin", "zke_engine_front_helper",
    "zke_qp_clean_batch", "zke_extract_captures_mapped", "zke_extract_captures_mapped_async",
    "zke_extract_bodies", "zke_extract_bodies_async",
    "zke_extract_captures_mixed", "zke_extract_captures_mixed_async",
    "zke_verify_emails_encoded", "zke_verify_emails_encoded_async", "zke_encode_outputs",
    "zke_engine_queue_count", "zke_engine_slot_queue", "zke_engine_last_slot",
    "zke_utf8_lossy_batch", "zke_extract_captures_encoded", "zke_extract_captures_encoded_async",
]


class SigInfo(NamedTuple):
    """One DKIM-Signature header as zke_scan_signatures reports it (zke_sig_info, the selector as bytes)."""
    header_index: int
    code: int                      # 0 candidate | D_NEUTRAL other domain | D_* why validate_header refuses it
    algo: int                      # SIG_ALGO_*; meaningful when code is 0 or D_NEUTRAL
    selector: bytes
    value_span: Tuple[int, int]    # the header's value in raw_email


class SigScan(NamedTuple):
    """A scan's answer for one e-mail: (status, detail, sigs) and the true counts (sigs holds the first max_sigs)."""
    status: int
    detail: int
    sigs: List[SigInfo]
    n_signatures: int = 0
    n_candidates: int = 0


class _ScanBuffers:
    """The caller-sized buffers of one zke_sig_scan (kept alive until the batch has been waited for)."""

    def __init__(self, n: int, max_sigs: int, blob_bytes: int):
        self.n = n
        self.status = np.zeros((max(n, 1), 4), np.uint32)
        self.sig_off = np.zeros(n + 1, np.uint32)
        self.sigs = np.zeros(max(n * max_sigs, 1), A.SIG_INFO_DTYPE)
        self.blob = np.zeros(max(blob_bytes, 1), np.uint8)
        o = self.c = A.zke_sig_scan()
        o.scan_status, o.scan_status_cap, o.sig_off, o.sig_off_cap = self.status.ctypes.data, 4 * n, self.sig_off.ctypes.data, n + 1
        o.sigs, o.sigs_cap, o.sel_blob, o.sel_blob_cap = self.sigs.ctypes.data, n * max_sigs, self.blob.ctypes.data, blob_bytes

    def result(self) -> List[SigScan]:
        blob = self.blob.tobytes()
        out = []
        for i in range(self.n):
            st = self.status[i]
            sigs = [SigInfo(int(r["header_index"]), int(r["code"]), int(r["algo"]),
                            blob[int(r["sel_off"]):int(r["sel_off"]) + int(r["sel_len"])], (int(r["val_start"]), int(r["val_end"])))
                    for r in self.sigs[int(self.sig_off[i]):int(self.sig_off[i + 1])]]
            out.append(SigScan(int(st[0]), int(st[1]), sigs, int(st[2]), int(st[3])))
        return out


class KeyInfo(NamedTuple):
    """One DKIM key record as zke_decode_key_records reports it (zke_key_info, the key as bytes)."""
    code: int                      # 0 a key | D_KEYREC_* why the record yields none
    key_type: int                  # KEY_RSA / KEY_ED25519 as far as the record got (KEY_OTHER with D_KEYREC_TYPE)
    key: bytes                     # PKCS#1 DER or 32 raw bytes; b"" unless code is 0

    def public_key(self) -> "A.PublicKey":
        """Email.public_key of a record that decoded."""
        return A.PublicKey(self.key, "ed25519" if self.key_type == A.KEY_ED25519 else "rsa")


class _KeyrecBuffers:
    """The records of one call as zke_keyrec_ref[m] and the caller-sized buffers of its zke_keyrec_out (kept alive until the batch
    has been waited for).  None stands for an empty record: the fetch failed."""

    def __init__(self, records: Sequence[Optional[bytes]], keys_bytes: Optional[int] = None, off=None):
        self.m = m = len(records)
        self.off = off                           # cand_off of a selection: result() is then one list per e-mail
        self._keep = [bytes(r) if r else b"" for r in records]
        self.arr = (A.zke_keyrec_ref * max(m, 1))()
        for j, r in enumerate(self._keep):
            self.arr[j].txt = C.cast(C.c_char_p(r), C.c_void_p).value if r else None
            self.arr[j].len = len(r)
        if keys_bytes is None:                   # 3/4 of the records' bytes always suffice
            keys_bytes = sum(min(len(r), A.KEYREC_MAX_BYTES) for r in self._keep) * 3 // 4
        self.infos = np.zeros(max(m, 1), A.KEY_INFO_DTYPE)
        self.keys = np.zeros(max(keys_bytes, 1), np.uint8)
        o = self.c = A.zke_keyrec_out()
        o.infos, o.infos_cap, o.keys, o.keys_cap = self.infos.ctypes.data, m, self.keys.ctypes.data, keys_bytes

    def result(self):
        blob = self.keys.tobytes()
        flat = [KeyInfo(int(f["code"]), int(f["key_type"]), blob[int(f["key_off"]):int(f["key_off"]) + int(f["key_len"])])
                for f in self.infos[:self.m]]
        if self.off is None:
            return flat
        return [flat[int(self.off[i]):int(self.off[i + 1])] for i in range(len(self.off) - 1)]


class BodyInfo(NamedTuple):
    """One e-mail's extract_email_body as zke_extract_bodies reports it (zke_body_info, the decoded body as bytes)."""
    status: int                    # ZKE_OK | ZKE_PARSE_FAIL | ZKE_BODY_DECODE_FAIL | ZKE_UNSUPPORTED
    detail: int
    part: int                      # 0 the message itself | k its k-th direct subpart; bit 31 (BODY_PART_HTML): chosen as text/html
    encoding: int                  # CTE_IDENTITY / CTE_BASE64 / CTE_QP
    src_off: int                   # body_bytes of the chosen part in the raw e-mail, before decoding
    src_len: int
    body: bytes                    # b"" unless status is ZKE_OK


class _BodyBuffers:
    """The e-mails of one call as zke_email_ref[n] (raw bytes only) and the caller-sized buffers of its zke_body_out (kept alive
    until the batch has been waited for)."""

    def __init__(self, raw_emails: Sequence[bytes], body_bytes: Optional[int] = None):
        self.n = n = len(raw_emails)
        self._keep = [bytes(r) for r in raw_emails]
        self.arr = (A.zke_email_ref * max(n, 1))()
        for j, r in enumerate(self._keep):
            self.arr[j].raw = C.cast(C.c_char_p(r), C.c_void_p).value if r else None
            self.arr[j].raw_len = len(r)
        if body_bytes is None:                   # a decoded body is at most twice its source (lone LF line ends of a QP body become CRLF)
            body_bytes = 2 * sum(len(r) for r in self._keep)
        self.infos = np.zeros(max(n, 1), A.BODY_INFO_DTYPE)
        self.bytes = np.zeros(max(body_bytes, 1), np.uint8)
        o = self.c = A.zke_body_out()
        o.infos, o.infos_cap, o.bytes, o.bytes_cap = self.infos.ctypes.data, n, self.bytes.ctypes.data, body_bytes

    def result(self) -> List[BodyInfo]:
        blob = self.bytes.tobytes()
        return [BodyInfo(int(f["status"]), int(f["detail"]), int(f["part"]), int(f["encoding"]), int(f["src_off"]), int(f["src_len"]),
                         blob[int(f["body_off"]):int(f["body_off"]) + int(f["body_len"])]) for f in self.infos[:self.n]]


class _EncodedCall:
    """Everything one zke_verify_emails_encoded call points to, kept alive until the batch has been waited for: the e-mails, the
    list form (`lists` / `mixed` of a zke_encode_in, or neither), the external-input table, the record array and the encoding buffers."""

    def __init__(self, eng: "Engine", inputs: Sequence, form: Optional[str], bytes_cap: Optional[int], infos_cap: Optional[int]):
        inputs = list(inputs)
        emails = [i if isinstance(i, Email) else i.email for i in inputs]
        if form is None:
            form = "plain" if all(isinstance(i, Email) for i in inputs) else "mixed" if any(isinstance(i, Email) for i in inputs) else "lists"
        self.form = form
        self.refs = A.EmailRefs(emails)
        n = self.refs.n
        self.ext = A.StringTable([A.flat_external_inputs(e.external_inputs) for e in emails])
        c = self.c = A.zke_encode_in()
        c.ext_off, c.ext_str_off, c.ext_blob = self.ext.off.ctypes.data, self.ext.str_off.ctypes.data, self.ext.blob.ctypes.data
        matches: List[Optional[List[str]]] = [None] * n
        if form == "lists":
            p = self._packed = eng.pack_with_regex(inputs)
            l = self._lists = A.zke_regex_lists()
            l.n_header_parts, l.n_body_parts = p.nh, p.nb
            l.header_part_ids, l.body_part_ids = p.hdr_ids.ctypes.data, p.body_ids.ctypes.data
            if p.has_caps:
                l.cap_off, l.cap_str_off, l.cap_blob = p.cap_off.ctypes.data, p.cap_str_off.ctypes.data, p.cap_blob.ctypes.data
            c.lists = C.pointer(l)
            matches = [regex_matches_of(i) for i in inputs]
        elif form == "mixed":
            self._mixed = eng.pack_mixed(inputs)
            c.mixed = C.pointer(self._mixed.c)
            matches = [None if isinstance(i, Email) else regex_matches_of(i) for i in inputs]
        elif form != "plain":
            raise ValueError("form must be 'plain', 'lists', 'mixed' or None")
        u8 = lambda xs: [len(s.encode("utf-8")) for s in xs]
        self.planned = [A.encoded_len(A.ENC_KIND_EMAIL if m is None else A.ENC_KIND_WITH_REGEX,
                                      u8(A.flat_external_inputs(e.external_inputs)), u8(m or [])) for e, m in zip(emails, matches)]
        self.out = np.zeros(max(n, 1), dtype=A.RESULT_DTYPE)
        self.enc = A.EncodedBuffers(n, sum(self.planned) if bytes_cap is None else bytes_cap)
        if infos_cap is not None:
            self.enc.c.infos_cap = infos_cap

    @property
    def records(self) -> np.ndarray:
        return self.out[:self.refs.n]


class ExtractEncoded:
    """One zke_extract_captures_encoded call (Engine.extract_captures_encoded_call): its return code, everything it points to —
    kept alive until the batch has been waited for — and the reading of what it delivered.  spans [n, G, 2], flags [n, G],
    cap_off [n * P + 1], cap_str_off, blob: the zke_capture_out arrays as they lie (blob with its guard bytes behind blob_bytes);
    enc: the ``_abi.EncodedBuffers``."""
    rc = 0
    ticket = 0

    def strings(self) -> List[List[bytes]]:
        """Per e-mail its capture strings in part order, as the device delivered them (repaired)."""
        raw = self.blob.tobytes()
        P, so = self.P, self.cap_str_off
        return [[raw[int(so[k]):int(so[k + 1])] for k in range(int(self.cap_off[i * P]), int(self.cap_off[(i + 1) * P]))] for i in range(self.n)]

    def regex_infos(self) -> List[Optional["A.RegexInfo"]]:
        """What compile_regex_parts returns per e-mail (None where the record is not OK): the strings are valid UTF-8 as they come."""
        raw, P, out = self.blob.tobytes(), self.P, []
        nh = len(self.regex_config.header_parts or [])
        for i in range(self.n):
            if self.records[i]["status"] != A.ZKE_OK:
                out.append(None)
                continue
            parts = [CompiledRegex(self.comp[p][0], [raw[int(self.cap_str_off[k]):int(self.cap_str_off[k + 1])].decode("utf-8")
                                                      for k in range(int(self.cap_off[i * P + p]), int(self.cap_off[i * P + p + 1]))])
                     for p in range(P)]
            out.append(A.RegexInfo(parts[:nh] if self.regex_config.header_parts is not None else None,
                                   parts[nh:] if self.regex_config.body_parts is not None else None))
        return out


class Engine:
    """One engine per GPU (``zke_engine``): owns the device workspace, the stream and the
    registered DFA tables."""

    def __init__(self, device: int = -1, max_sig_rounds: int = 0, **options):
        """`options`: any other field of ``zke_options`` by name — ``slots``, ``host_threads``, ``disable_key_cache``,
        ``max_dfas``, the kernel variants ``rsa_lane_groups`` / ``dfa_mapping`` / ``sha_mapping`` (0 by batch size, 1 / 2 forced;
        ``sha_mapping`` 1: the hash stage always runs one wave per 64 messages, 2: always two),
        ``replay_graphs``, the strictness flags of ``_abi.STRICT_FLAGS`` and ``now_unix``."""
        self.lib = load_library()
        if not self.lib.zke_device_available():
            raise EngineError("no HIP device visible; the engine has no CPU path")
        opt = A.zke_options()
        opt.device = device
        opt.max_sig_rounds = max_sig_rounds          # same-domain signatures tried per e-mail (0 = the default, 16)
        names = {f[0] for f in A.zke_options._fields_} - {"reserved"}
        for k, v in options.items():
            if k not in names:
                raise TypeError(f"zke_options has no field {k!r}")
            setattr(opt, k, int(v))
        self.options = opt
        h = C.c_void_p()
        rc = self.lib.zke_engine_create(C.byref(opt), C.byref(h))
        if rc != 0:
            msg = self.lib.zke_last_error(None)
            raise EngineError(f"zke_engine_create failed ({rc}): {msg.decode() if msg else ''}")
        self.h = h
        self._dfa_cache: Dict[Tuple[bytes, bytes], int] = {}
        self._capture_cache: Dict[bytes, int] = {}
        self._pattern_cache: Dict[Tuple[str, bool], Tuple[A.DFA, int, int]] = {}

    def close(self):
        if getattr(self, "h", None):
            self.lib.zke_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.zke_last_error(self.h)
            raise EngineError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    # ---- registration (replaces the per-email DFA::from_bytes of core/src/regex.rs:32-33)
    def dfa_register(self, fwd: bytes, bwd: bytes) -> int:
        key = (bytes(fwd), bytes(bwd))
        if key in self._dfa_cache:
            return self._dfa_cache[key]
        out = C.c_uint32()
        f = (C.c_uint8 * max(len(fwd), 1)).from_buffer_copy(fwd or b"\0")
        b = (C.c_uint8 * max(len(bwd), 1)).from_buffer_copy(bwd or b"\0")
        self._check(self.lib.zke_dfa_register(self.h, C.addressof(f), len(fwd), C.addressof(b), len(bwd),
                                              C.byref(out)), "zke_dfa_register")
        self._dfa_cache[key] = out.value
        return out.value

    def dfa_status(self, dfa_id: int) -> int:
        """0 when both blobs of the pair deserialise, else the ZKE_D_DFA_* section at which from_bytes gives up."""
        d = C.c_uint32()
        self._check(self.lib.zke_dfa_status(self.h, dfa_id, C.byref(d)), "zke_dfa_status")
        return d.value

    def dfa_unregister(self, dfa_id: int):
        self._check(self.lib.zke_dfa_unregister(self.h, dfa_id), "zke_dfa_unregister")
        self._dfa_cache = {k: v for k, v in self._dfa_cache.items() if v != dfa_id}
        self._pattern_cache = {k: v for k, v in self._pattern_cache.items() if v[1] != dfa_id}

    # ---- capture extraction (helpers/src/regex.rs:16-51 on the device)
    def capture_register(self, prog: bytes) -> int:
        prog = bytes(prog)
        if prog in self._capture_cache:
            return self._capture_cache[prog]
        out = C.c_uint32()
        buf = np.frombuffer(prog or b"\0", np.uint8)
        self._check(self.lib.zke_capture_register(self.h, buf.ctypes.data, len(prog), C.byref(out)), "zke_capture_register")
        self._capture_cache[prog] = out.value
        return out.value

    def capture_status(self, prog_id: int) -> int:
        """0, D_U_CAPTURE_PROGRAM (the blob does not decode) or D_U_CAPTURE_STATES (beyond the engine's limits)."""
        d = C.c_uint32()
        self._check(self.lib.zke_capture_status(self.h, prog_id, C.byref(d)), "zke_capture_status")
        return d.value

    def capture_unregister(self, prog_id: int):
        self._check(self.lib.zke_capture_unregister(self.h, prog_id), "zke_capture_unregister")
        self._capture_cache = {k: v for k, v in self._capture_cache.items() if v != prog_id}
        self._pattern_cache = {k: v for k, v in self._pattern_cache.items() if v[2] != prog_id}

    def compile_pattern(self, pattern: str, unicode: bool = True):
        """(DFA pair, its id, the capture program's id) of a pattern: compiled and registered once per engine."""
        key = (pattern, bool(unicode))
        if key not in self._pattern_cache:
            from . import regex_compile as rc
            dfa = rc.create_dfa(pattern, unicode=unicode)
            self._pattern_cache[key] = (dfa, self.dfa_register(dfa.fwd, dfa.bwd),
                                        self.capture_register(rc.create_capture_program(pattern, unicode=unicode)))
        return self._pattern_cache[key]

    def _run_captures(self, n: int, P: int, G: int, call, blob_bytes: int):
        """The caller-sized buffers of a zke_capture_out, one retry with the blob size the engine reports."""
        rc, spans, flags, cap_off, cap_str_off, blob = self._run_captures_sized(n * P, n * G, call, blob_bytes)
        return rc, spans.reshape(n, G, 2), flags.reshape(n, G), cap_off, cap_str_off, blob

    def _run_captures_sized(self, NP: int, NG: int, call, blob_bytes: int):
        """The same for NP (e-mail, part) jobs and NG columns, spans [NG, 2] and flags [NG] as they lie."""
        spans = np.zeros(max(NG * 2, 1), np.uint32)
        flags = np.zeros(max(NG, 1), np.uint8)
        cap_off = np.zeros(NP + 1, np.uint32)
        cap_str_off = np.zeros(NG + 1, np.uint32)
        for attempt in (0, 1):
            blob = np.zeros(max(blob_bytes, 1), np.uint8)
            o = A.zke_capture_out()
            o.spans, o.spans_cap, o.flags, o.flags_cap = spans.ctypes.data, NG * 2, flags.ctypes.data, NG
            o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = cap_off.ctypes.data, NP + 1, cap_str_off.ctypes.data, NG + 1
            o.cap_blob, o.cap_blob_cap = blob.ctypes.data, blob_bytes
            rc = call(o)
            if rc == -3 and attempt == 0 and o.cap_blob_need > blob_bytes:        # ZKE_E_NOMEM: the strings need a larger blob
                blob_bytes = int(o.cap_blob_need)
                continue
            return rc, spans[:NG * 2].reshape(NG, 2), flags[:NG], cap_off, cap_str_off[:int(o.n_strings) + 1], blob[:int(o.cap_blob_need)]

    def capture_batch(self, dfa_id: int, prog_id: int, groups: Sequence[int], haystacks: Sequence[bytes]):
        """zke_capture_batch: one pattern over plain haystacks.  Returns (matches [n, 4] = code, count, start, end;
        spans [n, G, 2]; flags [n, G]; strings: per haystack the list of raw group bytes, [] where the haystack failed)."""
        n, G = len(haystacks), len(groups)
        blob, off = A._csr(list(haystacks))
        g = np.array(list(groups), np.uint32)
        matches = np.zeros((max(n, 1), 4), np.uint32)
        rc, spans, flags, cap_off, cap_str_off, cblob = self._run_captures(
            n, 1, G, lambda o: self.lib.zke_capture_batch(self.h, dfa_id, prog_id, g.ctypes.data, G, blob.ctypes.data, off.ctypes.data, n,
                                                         matches.ctypes.data, C.byref(o)), 32 * n * G)
        self._check(rc, "zke_capture_batch")
        raw = cblob.tobytes()
        strings = [[raw[cap_str_off[k]:cap_str_off[k + 1]] for k in range(cap_off[i], cap_off[i + 1])] for i in range(n)]
        return matches[:n], spans, flags, strings

    def qp_clean_batch(self, bodies: Sequence[bytes]):
        """zke_qp_clean_batch: remove_quoted_printable_soft_breaks (core/src/email.rs:61-86) over a batch of bodies, both return
        values.  Returns (cleaned: the bodies without their soft breaks, zero-padded to their lengths; index_maps: per body a
        uint32 array, entry j = the position in the body of cleaned byte j, QP_NO_INDEX over the padding; clean_len: uint32[n],
        the bytes kept)."""
        n = len(bodies)
        blob, off = A._csr(list(bodies))
        total = int(off[n]) if n else 0
        cleaned = np.zeros(max(total, 1), np.uint8)
        imap = np.zeros(max(total, 1), np.uint32)
        clen = np.zeros(max(n, 1), np.uint32)
        self._check(self.lib.zke_qp_clean_batch(self.h, blob.ctypes.data, off.ctypes.data, n, cleaned.ctypes.data, imap.ctypes.data,
                                                clen.ctypes.data), "zke_qp_clean_batch")
        raw = cleaned.tobytes()
        return ([raw[int(off[i]):int(off[i + 1])] for i in range(n)], [imap[int(off[i]):int(off[i + 1])].copy() for i in range(n)], clen[:n])

    def utf8_lossy(self, strings: Sequence[bytes]):
        """zke_utf8_lossy_batch: String::from_utf8_lossy (helpers/src/regex.rs:35) over a batch of byte strings.  Returns (repaired:
        the strings as UTF-8 bytes, every ill-formed chunk one U+FFFD; changed: bool[n], the string was not valid UTF-8).  One
        call when three times the input fits the first buffer's guess, else a second with the exact need."""
        n = len(strings)
        blob, off = A._csr(list(strings))
        total = int(off[n]) if n else 0
        out_off = np.zeros(n + 1, np.uint32)
        flags = np.zeros(max(n, 1), np.uint8)
        need = C.c_size_t(0)
        out = np.zeros(max(total + total // 8, 64), np.uint8)
        for _ in range(2):
            rc = self.lib.zke_utf8_lossy_batch(self.h, blob.ctypes.data, off.ctypes.data, n, out_off.ctypes.data, out.ctypes.data, out.size,
                                               C.byref(need), flags.ctypes.data)
            if rc != -3:                                       # ZKE_E_NOMEM: the repaired strings need a larger blob
                break
            out = np.zeros(need.value, np.uint8)
        self._check(rc, "zke_utf8_lossy_batch")
        raw = out.tobytes()
        return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(n)], (flags[:n] & 1).astype(bool)

    def remove_quoted_printable_soft_breaks(self, body: bytes):
        """The reference's function on one body (a batch of one): (cleaned, index_map) with usize::MAX = 2**64 - 1 over the padding."""
        cleaned, maps, _ = self.qp_clean_batch([bytes(body)])
        return cleaned[0], [2 ** 64 - 1 if int(x) == A.QP_NO_INDEX else int(x) for x in maps[0]]

    def extract_captures(self, emails: Sequence[Email], regex_config, *, unicode: bool = True, origins: bool = False):
        """helpers/src/generator.rs:55-87 without the key fetch: verify_email + canonicalise + QP clean + exactly one match per
        pattern + the groups named by capture_indices, one batch on the GPU.  `regex_config`: a regex_compile.RegexConfig (or
        its JSON dict).  Returns (records, regex_infos): regex_infos[i] is the RegexInfo of e-mail i — what
        compile_regex_parts returns for it — or None where the record is not OK (the reference returns Err / panics there).
        origins=True (zke_extract_captures_mapped): a third value (origin_spans [n, G, 2], origin_flags [n, G]) — where each
        requested group lies in its haystack BEFORE the QP filter (the canonical body as it was signed), ORGF_* per group."""
        from . import regex_compile as rc
        if isinstance(regex_config, dict):
            regex_config = rc.RegexConfig.from_json(regex_config)
        hp, bp = list(regex_config.header_parts or []), list(regex_config.body_parts or [])
        comp = [self.compile_pattern(p.pattern, unicode) for p in hp + bp]
        groups = [np.array(list(p.capture_indices or []), np.uint32) for p in hp + bp]
        arr = (A.zke_capture_part * max(len(comp), 1))()
        for k, ((_, dfa_id, prog_id), g) in enumerate(zip(comp, groups)):
            arr[k].dfa_id, arr[k].prog_id, arr[k].n_groups, arr[k].groups = dfa_id, prog_id, len(g), g.ctypes.data
        refs = emails if isinstance(emails, A.EmailRefs) else A.EmailRefs(emails)
        n, P, G = refs.n, len(comp), sum(len(g) for g in groups)
        out = np.zeros(max(n, 1), dtype=A.RESULT_DTYPE)
        body = C.cast(C.byref(arr, len(hp) * C.sizeof(A.zke_capture_part)), C.POINTER(A.zke_capture_part))
        call = lambda o: self.lib.zke_extract_captures(self.h, refs.arr, n, arr, len(hp), body, len(bp), out.ctypes.data, C.byref(o))
        if origins:
            ospans, oflags = np.zeros(max(n * G * 2, 1), np.uint32), np.zeros(max(n * G, 1), np.uint8)
            org = A.zke_capture_origin()
            org.spans, org.spans_cap, org.flags, org.flags_cap = ospans.ctypes.data, n * G * 2, oflags.ctypes.data, n * G
            call = lambda o: self.lib.zke_extract_captures_mapped(self.h, refs.arr, n, arr, len(hp), body, len(bp), out.ctypes.data,
                                                                  C.byref(o), C.byref(org))
        rcode, spans, flags, cap_off, cap_str_off, cblob = self._run_captures(n, P, G, call, 32 * n * G)
        self._check(rcode, "zke_extract_captures_mapped" if origins else "zke_extract_captures")
        raw = cblob.tobytes()
        infos: List[Optional[A.RegexInfo]] = []
        for i in range(n):
            if out[i]["status"] != A.ZKE_OK:
                infos.append(None)
                continue
            parts, col = [], 0
            for p in range(P):
                strs = []
                for k in range(cap_off[i * P + p], cap_off[i * P + p + 1]):
                    b = raw[cap_str_off[k]:cap_str_off[k + 1]]
                    # regex.rs:35 String::from_utf8_lossy — only the strings the device flagged need the repair
                    strs.append(b.decode("utf-8", errors="replace") if flags[i, col] & A.CAPF_NOT_UTF8 else b.decode("utf-8"))
                    col += 1
                parts.append(CompiledRegex(comp[p][0], strs))
            infos.append(A.RegexInfo(parts[:len(hp)] if regex_config.header_parts is not None else None,
                                     parts[len(hp):] if regex_config.body_parts is not None else None))
        if origins:
            return out[:n], infos, (ospans[:n * G * 2].reshape(n, G, 2), oflags[:n * G].reshape(n, G))
        return out[:n], infos

    def extract_captures_encoded_call(self, emails: Sequence[Email], regex_config, external_inputs=None, *, unicode: bool = True,
                                      blob_bytes: Optional[int] = None, bytes_cap: Optional[int] = None, want_caps: bool = True,
                                      guard: int = 0, fill: int = 0, ticket: bool = False):
        """ONE zke_extract_captures_encoded with caller-sized buffers and no retry: returns an ``ExtractEncoded`` — rc (0, or -3 =
        ZKE_E_NOMEM when `blob_bytes` / `bytes_cap` is too small: everything but the short buffer's bytes is delivered and the needs
        are exact), the records, the capture tables (None with want_caps=False: caps is NULL) and the ``_abi.EncodedBuffers``.
        `external_inputs`: per e-mail its list of ExternalInput (default: each Email's own), flattened as the reference does.
        `guard` / `fill`: bytes behind both variable-size buffers and their initial value, for tests that watch what is written.
        ticket=True: the asynchronous form; `.ticket` is to be waited for (``wait``) before anything is read, and rc is the submit's."""
        from . import regex_compile as rc
        if isinstance(regex_config, dict):
            regex_config = rc.RegexConfig.from_json(regex_config)
        hp, bp = list(regex_config.header_parts or []), list(regex_config.body_parts or [])
        comp = [self.compile_pattern(p.pattern, unicode) for p in hp + bp]
        groups = [np.array(list(p.capture_indices or []), np.uint32) for p in hp + bp]
        arr = (A.zke_capture_part * max(len(comp), 1))()
        for k, ((_, dfa_id, prog_id), g) in enumerate(zip(comp, groups)):
            arr[k].dfa_id, arr[k].prog_id, arr[k].n_groups, arr[k].groups = dfa_id, prog_id, len(g), g.ctypes.data
        body = C.cast(C.byref(arr, len(hp) * C.sizeof(A.zke_capture_part)), C.POINTER(A.zke_capture_part))
        emails = list(emails)
        refs = A.EmailRefs(emails)
        n, P, G = refs.n, len(comp), sum(len(g) for g in groups)
        ext_lists = [e.external_inputs for e in emails] if external_inputs is None else list(external_inputs)
        ext = A.StringTable([A.flat_external_inputs(x) for x in ext_lists])
        r = ExtractEncoded()
        r.n, r.P, r.G, r.comp, r.regex_config = n, P, G, comp, regex_config
        r.keep = (refs, arr, groups, ext)
        r.records = np.zeros(max(n, 1), dtype=A.RESULT_DTYPE)[:n]
        out_ptr = r.records.ctypes.data if n else None
        r.blob_bytes = 64 * n * G if blob_bytes is None else blob_bytes
        r.spans, r.flags = np.zeros(max(n * G * 2, 1), np.uint32), np.zeros(max(n * G, 1), np.uint8)
        r.cap_off, r.cap_str_off = np.zeros(n * P + 1, np.uint32), np.zeros(n * G + 1, np.uint32)
        r.blob = np.full(max(r.blob_bytes + guard, 1), fill, np.uint8)
        o = r.caps = A.zke_capture_out()
        o.spans, o.spans_cap, o.flags, o.flags_cap = r.spans.ctypes.data, n * G * 2, r.flags.ctypes.data, n * G
        o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = r.cap_off.ctypes.data, n * P + 1, r.cap_str_off.ctypes.data, n * G + 1
        o.cap_blob, o.cap_blob_cap = r.blob.ctypes.data, r.blob_bytes
        r.want_caps = want_caps
        # an encoding: 192 bytes of head, the external inputs, per match 64 bytes and its padded bytes (_abi.encoded_len)
        r.enc = A.EncodedBuffers(n, (256 * n + 2 * int(ext.str_off[-1]) + 64 * ext.n_strings + 160 * n * G) if bytes_cap is None else bytes_cap,
                                 guard, fill)
        args = (self.h, refs.arr, n, arr, len(hp), body, len(bp), out_ptr, C.byref(o) if want_caps else None,
                ext.off.ctypes.data if ext.n_strings else None, ext.str_off.ctypes.data, ext.blob.ctypes.data, C.byref(r.enc.c))
        r.args = args                            # (the synchronous entry's arguments: a caller that times it calls it again with these)
        if ticket:
            t = C.c_uint64()
            r.rc = self.lib.zke_extract_captures_encoded_async(*args, C.byref(t))
            r.ticket = t.value
        else:
            r.rc = self.lib.zke_extract_captures_encoded(*args)
        return r

    def extract_captures_encoded(self, emails: Sequence[Email], regex_config, external_inputs=None, *, unicode: bool = True):
        """zke_extract_captures_encoded: from raw e-mails, keys and a regex config to the public values, one batch on the GPU —
        verify_email, the extraction, String::from_utf8_lossy, abi_encode and SHA-256.  Returns (records, regex_infos, encodings,
        digests): regex_infos[i] as ``extract_captures`` gives it, the strings taken from the device as they are (they are repaired
        there); encodings[i] / digests[i] the bytes of EmailWithRegexVerifierOutput.abi_encode() and their SHA-256, b"" and 32 zero
        bytes where the record is not OK.  One call when the first guess of the two variable-size buffers holds, else a second
        with the exact needs."""
        r = self.extract_captures_encoded_call(emails, regex_config, external_inputs, unicode=unicode)
        if r.rc == -3:                                         # ZKE_E_NOMEM: the needs are exact
            r = self.extract_captures_encoded_call(emails, regex_config, external_inputs, unicode=unicode,
                                                   blob_bytes=max(int(r.caps.cap_blob_need), r.blob_bytes),
                                                   bytes_cap=max(int(r.enc.c.bytes_need), r.enc.nbytes))
        self._check(r.rc, "zke_extract_captures_encoded")
        res = r.enc.result()
        return r.records, r.regex_infos(), [x[0] for x in res], [x[1] for x in res]

    def pack_capture_mixed(self, regex_configs: Sequence, *, unicode: bool = True):
        """The tables of zke_extract_captures_mixed for one ``RegexConfig`` (or its JSON dict, or None: verify_email only) per
        e-mail: compiles and registers every pattern, deduplicates the configs by content (patterns and capture_indices, first
        appearance first).  Returns (``_abi.CaptureMixedLists``, the distinct RegexConfig values in its order)."""
        from . import regex_compile as rc
        index: Dict[object, int] = {}
        distinct, configs, config_of = [], [], []
        for cfg in regex_configs:
            if cfg is None:
                config_of.append(A.CONFIG_NONE)
                continue
            if isinstance(cfg, dict):
                cfg = rc.RegexConfig.from_json(cfg)
            side = lambda parts: None if parts is None else tuple((p.pattern, tuple(p.capture_indices or [])) for p in parts)
            key = (side(cfg.header_parts), side(cfg.body_parts))
            if key not in index:
                if len(configs) == A.MIXED_MAX_CONFIGS:
                    raise EngineError("more than ZKE_MIXED_MAX_CONFIGS regex configs in one batch; split it")
                index[key] = len(configs)
                distinct.append(cfg)
                part = lambda p: (*self.compile_pattern(p.pattern, unicode)[1:], list(p.capture_indices or []))
                configs.append(([part(p) for p in cfg.header_parts or []], [part(p) for p in cfg.body_parts or []]))
            config_of.append(index[key])
        return A.CaptureMixedLists(configs, config_of), distinct

    def _capture_mixed_call(self, refs, lists, origins: bool, blob_bytes: Optional[int] = None):
        """One synchronous zke_extract_captures_mixed with caller-sized buffers (one retry with the blob size the engine reports)."""
        n, J, Gt = refs.n, lists.J, lists.Gt
        out = np.zeros(max(n, 1), dtype=A.RESULT_DTYPE)
        ospans, oflags = np.zeros(max(Gt * 2, 1), np.uint32), np.zeros(max(Gt, 1), np.uint8)
        org = A.zke_capture_origin()
        org.spans, org.spans_cap, org.flags, org.flags_cap = ospans.ctypes.data, Gt * 2, oflags.ctypes.data, Gt
        call = lambda o: self.lib.zke_extract_captures_mixed(self.h, refs.arr, n, C.byref(lists.c), out.ctypes.data, C.byref(o),
                                                             C.byref(org) if origins else None)
        rcode, spans, flags, cap_off, cap_str_off, cblob = self._run_captures_sized(J, Gt, call, 32 * Gt if blob_bytes is None else blob_bytes)
        self._check(rcode, "zke_extract_captures_mixed")
        return out[:n], spans, flags, cap_off, cap_str_off, cblob, (ospans[:Gt * 2].reshape(Gt, 2), oflags[:Gt])

    def extract_captures_mixed(self, emails: Sequence[Email], regex_configs: Sequence, *, unicode: bool = True, origins: bool = False):
        """zke_extract_captures_mixed: `extract_captures` for e-mails that carry different regex configs, one batch on the GPU.
        `regex_configs[i]`: e-mail i's RegexConfig (or its JSON dict), or None for an e-mail that is verify_email only.  Returns
        (records, regex_infos): regex_infos[i] is the RegexInfo of e-mail i, or None where the record is not OK or the e-mail has no
        config.  origins=True: a third value (origin_spans, origin_flags), per e-mail ragged arrays [G_i, 2] and [G_i] — where
        each requested group lies in its haystack BEFORE the QP filter."""
        if len(emails) != len(regex_configs):
            raise ValueError("one regex config (or None) per e-mail")
        lists, distinct = self.pack_capture_mixed(regex_configs, unicode=unicode)
        refs = emails if isinstance(emails, A.EmailRefs) else A.EmailRefs(emails)
        out, spans, flags, cap_off, cap_str_off, cblob, (ospans, oflags) = self._capture_mixed_call(refs, lists, origins)
        raw = cblob.tobytes()
        infos: List[Optional[A.RegexInfo]] = []
        for i in range(refs.n):
            c = int(lists.config_of[i])
            if c == A.CONFIG_NONE or out[i]["status"] != A.ZKE_OK:
                infos.append(None)
                continue
            cfg, j0, col = distinct[c], int(lists.job_off[i]), int(lists.col_off[i])
            pats = list(cfg.header_parts or []) + list(cfg.body_parts or [])
            parts = []
            for p, pat in enumerate(pats):
                strs = []
                for k in range(cap_off[j0 + p], cap_off[j0 + p + 1]):
                    b = raw[cap_str_off[k]:cap_str_off[k + 1]]
                    strs.append(b.decode("utf-8", errors="replace") if flags[col] & A.CAPF_NOT_UTF8 else b.decode("utf-8"))
                    col += 1
                parts.append(CompiledRegex(self.compile_pattern(pat.pattern, unicode)[0], strs))
            nh = len(cfg.header_parts or [])
            infos.append(A.RegexInfo(parts[:nh] if cfg.header_parts is not None else None, parts[nh:] if cfg.body_parts is not None else None))
        if origins:
            cut = lambda a: [a[int(lists.col_off[i]):int(lists.col_off[i + 1])].copy() for i in range(refs.n)]
            return out, infos, (cut(ospans), cut(oflags))
        return out, infos

    # ---- DKIM-Signature scan and key selection (helpers/src/generator.rs:11-53 around the caller's DNS fetch)
    @staticmethod
    def _scan_refs(raw_emails: Sequence[bytes], from_domains: Sequence[str]) -> "A.EmailRefs":
        if len(raw_emails) != len(from_domains):
            raise ValueError("one from_domain per raw e-mail")
        return A.EmailRefs([Email(d, bytes(r), A.PublicKey(b"")) for r, d in zip(raw_emails, from_domains)])

    def scan_signatures(self, raw_emails: Sequence[bytes], from_domains: Sequence[str], max_sigs: int = 8, *, blob_bytes: Optional[int] = None) -> List[SigScan]:
        """zke_scan_signatures: per e-mail (status, detail, [SigInfo]) — every DKIM-Signature header with validate_header's verdict,
        whether d= names from_domain (code 0), a= classified and the selector; plus the true counts n_signatures / n_candidates
        (the list holds the first `max_sigs`).  `blob_bytes`: the selector buffer's size (default 32 bytes per record slot; the
        call is repeated once with the size the engine reports when that is too small)."""
        refs = self._scan_refs(raw_emails, from_domains)
        n = refs.n
        blob_bytes = 32 * n * max_sigs if blob_bytes is None else blob_bytes
        for attempt in (0, 1):
            b = _ScanBuffers(n, max_sigs, blob_bytes)
            rc = self.lib.zke_scan_signatures(self.h, refs.arr, n, max_sigs, C.byref(b.c))
            if rc == -3 and attempt == 0 and b.c.sel_blob_need > blob_bytes:           # ZKE_E_NOMEM: the selectors need a larger blob
                blob_bytes = int(b.c.sel_blob_need)
                continue
            self._check(rc, "zke_scan_signatures")
            return b.result()

    def scan_signatures_async(self, raw_emails: Sequence[bytes], from_domains: Sequence[str], max_sigs: int = 8, *, blob_bytes: Optional[int] = None):
        """zke_scan_signatures_async: (ticket, pending); ``pending.result()`` is valid once ``wait(ticket)`` has returned."""
        refs = self._scan_refs(raw_emails, from_domains)
        b = _ScanBuffers(refs.n, max_sigs, 32 * refs.n * max_sigs if blob_bytes is None else blob_bytes)
        b.refs = refs
        t = C.c_uint64()
        self._check(self.lib.zke_scan_signatures_async(self.h, refs.arr, refs.n, max_sigs, C.byref(b.c), C.byref(t)), "zke_scan_signatures_async")
        return t.value, b

    @staticmethod
    def _key_refs(candidate_keys):
        flat = [k for ks in candidate_keys for k in ks]
        off = np.zeros(len(candidate_keys) + 1, np.uint32)
        off[1:] = np.cumsum([len(ks) for ks in candidate_keys])
        arr = (A.zke_key_ref * max(len(flat), 1))()
        keep = []
        for j, k in enumerate(flat):
            kb = bytes(k.key) if k is not None else b""
            keep.append(kb)
            arr[j].key = C.cast(C.c_char_p(kb), C.c_void_p).value if kb else None
            arr[j].key_len = len(kb)
            arr[j].key_type = A.key_type_code(k.key_type) if k is not None else A.KEY_RSA
        return off, arr, keep

    def select_keys(self, emails, candidate_keys: Sequence[Sequence[Optional["A.PublicKey"]]]):
        """zke_select_keys: candidate_keys[i] = the keys fetched for e-mail i's candidates, in the scan's order (None or an empty
        key: the fetch failed).  Returns (records, chosen): chosen[i] = the first key under which the e-mail verifies (bit 31,
        _abi.SEL_AFTER_UNSUPPORTED: an earlier candidate was outside what the engine implements) or _abi.SEL_NONE; records[i] = that
        verification's record.  The e-mails' own public_key fields are ignored."""
        refs = emails if isinstance(emails, A.EmailRefs) else A.EmailRefs(emails)
        if refs.n != len(candidate_keys):
            raise ValueError("one candidate list per e-mail")
        off, arr, keep = self._key_refs(candidate_keys)
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        chosen = np.zeros(max(refs.n, 1), np.uint32)
        self._check(self.lib.zke_select_keys(self.h, refs.arr, refs.n, off.ctypes.data, arr, out.ctypes.data, chosen.ctypes.data), "zke_select_keys")
        return out[:refs.n], chosen[:refs.n]

    def select_keys_async(self, emails, candidate_keys):
        """zke_select_keys_async: (ticket, records, chosen), valid once ``wait(ticket)`` has returned."""
        refs = emails if isinstance(emails, A.EmailRefs) else A.EmailRefs(emails)
        off, arr, keep = self._key_refs(candidate_keys)
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        chosen = np.zeros(max(refs.n, 1), np.uint32)
        t = C.c_uint64()
        self._check(self.lib.zke_select_keys_async(self.h, refs.arr, refs.n, off.ctypes.data, arr, out.ctypes.data, chosen.ctypes.data, C.byref(t)),
                    "zke_select_keys_async")
        return t.value, out[:refs.n], chosen[:refs.n]

    # ---- DKIM key records (helpers/src/dkim.rs:67-111: what the resolver returns -> Email.public_key)
    def decode_key_records(self, records: Sequence[Optional[bytes]], mode: int = A.KEYREC_DNS, *, keys_bytes: Optional[int] = None) -> List[KeyInfo]:
        """zke_decode_key_records: one KeyInfo per record (None or b"": the fetch failed).  `mode`: _abi.KEYREC_DNS, the TXT record
        of RFC 6376 3.6.1, or _abi.KEYREC_ARCHIVE, the archive value as helpers/src/dkim.rs:67-111 reads it.  `keys_bytes`: the
        key buffer's size (default: 3/4 of the records' bytes, which always suffices)."""
        b = _KeyrecBuffers(records, keys_bytes)
        self._check(self.lib.zke_decode_key_records(self.h, b.arr, b.m, mode, C.byref(b.c)), "zke_decode_key_records")
        return b.result()

    def decode_key_records_async(self, records: Sequence[Optional[bytes]], mode: int = A.KEYREC_DNS, *, keys_bytes: Optional[int] = None):
        """zke_decode_key_records_async: (ticket, pending); ``pending.result()`` is valid once ``wait(ticket)`` has returned."""
        b = _KeyrecBuffers(records, keys_bytes)
        t = C.c_uint64()
        self._check(self.lib.zke_decode_key_records_async(self.h, b.arr, b.m, mode, C.byref(b.c), C.byref(t)), "zke_decode_key_records_async")
        return t.value, b

    def select_keys_from_records(self, emails, candidate_records: Sequence[Sequence[Optional[bytes]]], mode: int = A.KEYREC_DNS):
        """zke_select_keys_from_records: select_keys with the resolver's raw answers in place of keys — candidate_records[i] = the
        records fetched for e-mail i's candidates, in the scan's order (None or b"": the fetch failed).  The records are decoded on
        the GPU in front of the verify launches; the decoded keys stay in HBM on their way there.  Returns (records, chosen, infos):
        infos[i][k] = the KeyInfo of e-mail i's candidate k, from which Email.public_key of the chosen one is built."""
        refs = emails if isinstance(emails, A.EmailRefs) else A.EmailRefs(emails)
        if refs.n != len(candidate_records):
            raise ValueError("one candidate list per e-mail")
        t, out, chosen, pend = self.select_keys_from_records_async(refs, candidate_records, mode)
        self.wait(t)
        return out, chosen, pend.result()

    def select_keys_from_records_async(self, emails, candidate_records, mode: int = A.KEYREC_DNS):
        """zke_select_keys_from_records_async: (ticket, records, chosen, pending), valid once ``wait(ticket)`` has returned;
        ``pending.result()`` is the per-e-mail lists of KeyInfo."""
        refs = emails if isinstance(emails, A.EmailRefs) else A.EmailRefs(emails)
        off = np.zeros(len(candidate_records) + 1, np.uint32)
        off[1:] = np.cumsum([len(r) for r in candidate_records])
        b = _KeyrecBuffers([r for row in candidate_records for r in row], off=off)
        b.refs = refs
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        chosen = np.zeros(max(refs.n, 1), np.uint32)
        t = C.c_uint64()
        self._check(self.lib.zke_select_keys_from_records_async(self.h, refs.arr, refs.n, off.ctypes.data, b.arr, mode, out.ctypes.data,
                                                                chosen.ctypes.data, C.byref(b.c), C.byref(t)), "zke_select_keys_from_records_async")
        return t.value, out[:refs.n], chosen[:refs.n], b

    # ---- extract_email_body (core/src/email.rs:7-23): the text/html part, transfer-decoded
    def extract_bodies(self, raw_emails: Sequence[bytes], *, part_keeps_eol: bool = False, body_bytes: Optional[int] = None) -> List[BodyInfo]:
        """zke_extract_bodies: one BodyInfo per raw e-mail.  `part_keeps_eol`: ZKE_BODYF_PART_KEEPS_EOL, the line break in front of a
        boundary line stays part of the body.  `body_bytes`: the byte buffer's size (default: twice the e-mails' bytes, which always
        suffices); too small raises EngineError(ZKE_E_NOMEM)."""
        b = _BodyBuffers(raw_emails, body_bytes)
        self._check(self.lib.zke_extract_bodies(self.h, b.arr, b.n, A.BODYF_PART_KEEPS_EOL if part_keeps_eol else 0, C.byref(b.c)), "zke_extract_bodies")
        return b.result()

    def extract_bodies_async(self, raw_emails: Sequence[bytes], *, part_keeps_eol: bool = False, body_bytes: Optional[int] = None):
        """zke_extract_bodies_async: (ticket, pending); ``pending.result()`` is valid once ``wait(ticket)`` has returned."""
        b = _BodyBuffers(raw_emails, body_bytes)
        t = C.c_uint64()
        self._check(self.lib.zke_extract_bodies_async(self.h, b.arr, b.n, A.BODYF_PART_KEEPS_EOL if part_keeps_eol else 0, C.byref(b.c), C.byref(t)),
                    "zke_extract_bodies_async")
        return t.value, b

    # ---- batches
    def verify_batch_async(self, batch: PackedBatch):
        """zke_verify_batch_async: returns (ticket, records); the records are valid once ``wait(ticket)`` has returned.
        The batch's buffers may be reused as soon as this returns."""
        out = np.zeros(max(batch.n, 1), dtype=A.RESULT_DTYPE)
        t = C.c_uint64()
        self._check(self.lib.zke_verify_batch_async(self.h, C.byref(batch.c), out.ctypes.data, C.byref(t)), "zke_verify_batch_async")
        return t.value, out[:batch.n]

    def wait(self, ticket: int):
        self._check(self.lib.zke_batch_wait(self.h, ticket), "zke_batch_wait")

    def verify_batch(self, batch: PackedBatch, debug: Optional[DebugBuffers] = None) -> np.ndarray:
        out = np.zeros(max(batch.n, 1), dtype=A.RESULT_DTYPE)
        self._check(self.lib.zke_verify_batch(self.h, C.byref(batch.c), out.ctypes.data,
                                              C.byref(debug.c) if debug is not None else None), "zke_verify_batch")
        return out[:batch.n]

    def verify_batch_device(self, cbatch: A.zke_batch, raw_total: int, domain_total: int, key_total: int,
                            out_dev_ptr: int, stream: int = 0):
        self._check(self.lib.zke_verify_batch_device(self.h, C.byref(cbatch), raw_total, domain_total, key_total,
                                                     out_dev_ptr, stream), "zke_verify_batch_device")

    def reserve(self, max_n: int, max_raw_total: int, slots: int = 1, max_regex_parts: int = 0):
        """Size `slots` submission slots for batches of up to max_n e-mails / max_raw_total raw bytes: nothing is
        allocated in the submit path afterwards; `slots` batches can be in flight (zke_engine_reserve)."""
        self._check(self.lib.zke_engine_reserve(self.h, max_n, max_raw_total, slots, max_regex_parts), "zke_engine_reserve")

    def reserve_host(self, max_n: int, max_input_bytes: int):
        """Size every slot's pinned staging for host-entry batches of up to max_n e-mails / max_input_bytes of inputs."""
        self._check(self.lib.zke_engine_reserve_host(self.h, max_n, max_input_bytes), "zke_engine_reserve_host")

    def sync(self):
        self._check(self.lib.zke_engine_sync(self.h), "zke_engine_sync")

    def sha_ring(self) -> bool:
        """Whether the two-wave SHA-256 groups take the ring routine as the engine stands now (zke_engine_sha_ring)."""
        r = self.lib.zke_engine_sha_ring(self.h)
        self._check(min(r, 0), "zke_engine_sha_ring")
        return r == 1

    def sha_twin(self) -> bool:
        """Whether the ring's rounds wave takes two lanes per message as the engine stands now (zke_engine_sha_twin)."""
        r = self.lib.zke_engine_sha_twin(self.h)
        self._check(min(r, 0), "zke_engine_sha_twin")
        return r == 1

    def front_helper(self, n: int) -> bool:
        """Whether a batch of n e-mails takes the two-wave front end as the engine stands now (zke_engine_front_helper)."""
        r = self.lib.zke_engine_front_helper(self.h, n)
        self._check(min(r, 0), "zke_engine_front_helper")
        return r == 1

    def queue_count(self) -> int:
        """How many groups of slots share a hardware queue each, 0 while the map is unknown (zke_engine_queue_count)."""
        r = self.lib.zke_engine_queue_count(self.h)
        self._check(min(r, 0), "zke_engine_queue_count")
        return r

    def slot_queue(self, slot: int) -> int:
        """The group of slots `slot` shares its hardware queue with, or -1 if unknown (zke_engine_slot_queue)."""
        return self.lib.zke_engine_slot_queue(self.h, slot)

    def last_slot(self) -> int:
        """The slot the most recent submission took (zke_engine_last_slot)."""
        r = self.lib.zke_engine_last_slot(self.h)
        self._check(min(r, 0), "zke_engine_last_slot")
        return r

    def join(self, stream: int = 0):
        """Work enqueued on `stream` (a hipStream_t handle; 0 = the null stream) from now on runs behind every batch
        submitted so far; the host does not wait (zke_engine_join)."""
        self._check(self.lib.zke_engine_join(self.h, stream), "zke_engine_join")

    def slot_timings(self, slot: int) -> dict:
        t = A.zke_timings()
        self._check(self.lib.zke_get_slot_timings(self.h, slot, C.byref(t)), "zke_get_slot_timings")
        return {k: getattr(t, k) for k, _ in A.zke_timings._fields_}

    def set_timing(self, on: bool):
        self._check(self.lib.zke_set_timing(self.h, 1 if on else 0), "zke_set_timing")

    def timings(self) -> dict:
        t = A.zke_timings()
        self._check(self.lib.zke_get_timings(self.h, C.byref(t)), "zke_get_timings")
        return {k: getattr(t, k) for k, _ in A.zke_timings._fields_}

    def verify_wire(self, data: bytes, fmt: str = "borsh", with_regex: bool = False) -> np.ndarray:
        """zke_verify_wire: one borsh / bincode serialised Email or EmailWithRegex (core/src/structs.rs:1-6) -> its record."""
        out = np.zeros(1, dtype=A.RESULT_DTYPE)
        buf = np.frombuffer(bytes(data) or b"\0", np.uint8)
        self._check(self.lib.zke_verify_wire(self.h, {"borsh": 0, "bincode": 1}[fmt], buf.ctypes.data, len(data), 1 if with_regex else 0,
                                             out.ctypes.data), "zke_verify_wire")
        return out[0]

    # ---- building blocks
    def sha256_batch(self, msgs: Sequence[bytes]) -> np.ndarray:
        """hash_bytes (core/src/crypto.rs:3-7) over a list of messages, on the GPU."""
        blob, off = A._csr(list(msgs))
        out = np.zeros((max(len(msgs), 1), 32), np.uint8)
        self._check(self.lib.zke_sha256_batch(self.h, blob.ctypes.data, off.ctypes.data, len(msgs), out.ctypes.data),
                    "zke_sha256_batch")
        return out[:len(msgs)]

    def rsa_modexp_batch(self, sigs: Sequence[bytes], mods: Sequence[bytes], exps: Sequence[int], nbytes: int):
        n = len(sigs)
        s = np.frombuffer(b"".join(x.rjust(nbytes, b"\0") for x in sigs), np.uint8).copy()
        m = np.frombuffer(b"".join(x.rjust(nbytes, b"\0") for x in mods), np.uint8).copy()
        e = np.array(list(exps), dtype=np.uint64)
        em = np.zeros((n, nbytes), np.uint8)
        ok = np.zeros(n, np.uint8)
        self._check(self.lib.zke_rsa_modexp_batch(self.h, s.ctypes.data, m.ctypes.data, e.ctypes.data, nbytes, n,
                                                  em.ctypes.data, ok.ctypes.data), "zke_rsa_modexp_batch")
        return em, ok

    def ed25519_verify_batch(self, keys: Sequence[bytes], msgs: Sequence[bytes], sigs: Sequence[bytes]) -> np.ndarray:
        """0 = key does not decode, 1 = rejected, 2 = valid (ed25519-dalek verify_strict); equal-length messages <= 32 B."""
        n = len(keys)
        ml = len(msgs[0]) if n else 32
        assert all(len(k) == 32 for k in keys) and all(len(x) == 64 for x in sigs) and all(len(m) == ml for m in msgs)
        k = np.frombuffer(b"".join(keys), np.uint8).copy()
        m = np.frombuffer(b"".join(msgs), np.uint8).copy()
        g = np.frombuffer(b"".join(sigs), np.uint8).copy()
        out = np.zeros(n, np.uint32)
        self._check(self.lib.zke_ed25519_verify_batch(self.h, k.ctypes.data, m.ctypes.data, ml, g.ctypes.data, n,
                                                      out.ctypes.data), "zke_ed25519_verify_batch")
        return out

    # ---- zkemail_core mirror
    def pack_with_regex(self, inputs: Sequence[EmailWithRegex]) -> PackedBatch:
        """All inputs must share one part list (one regex_config per batch); captures are per e-mail."""
        first = inputs[0].regex_info
        hp = first.header_parts or []
        bp = first.body_parts or []
        hids = [self.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in hp]
        bids = [self.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in bp]
        caps = []
        for inp in inputs:
            h2, b2 = inp.regex_info.header_parts or [], inp.regex_info.body_parts or []
            if [self.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in h2] != hids or \
               [self.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in b2] != bids:
                raise EngineError("a batch must share one part list; split it per regex_config")
            caps.append([list(p.captures or []) for p in list(h2) + list(b2)])
        return PackedBatch([i.email for i in inputs], hids, bids, caps, with_regex=True)

    def _email_args(self, email: Email):
        raw = np.frombuffer(email.raw_email or b"\0", np.uint8)
        key = np.frombuffer(email.public_key.key or b"\0", np.uint8)
        dom = email.from_domain.encode("utf-8")
        ext = 1 if any(x.value is None for x in email.external_inputs) else 0
        return (raw, key), [raw.ctypes.data, len(email.raw_email), dom, len(dom), key.ctypes.data, len(email.public_key.key),
                            A.key_type_code(email.public_key.key_type), ext]

    def verify_emails(self, emails) -> np.ndarray:
        """zke_verify_emails: a list of Email values (or a prepared ``_abi.EmailRefs``), each with its own buffers, gathered by the
        engine — no concatenation on the caller's side.  Returns the records."""
        refs = emails if isinstance(emails, A.EmailRefs) else A.EmailRefs(emails)
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        self._check(self.lib.zke_verify_emails(self.h, refs.arr, refs.n, out.ctypes.data), "zke_verify_emails")
        return out[:refs.n]

    def verify_emails_with_regex(self, inputs: Sequence[EmailWithRegex]) -> np.ndarray:
        """zke_verify_emails_with_regex: a list of EmailWithRegex that share one part list; the e-mails stay in their own buffers,
        the part ids and capture tables are built as ``pack_with_regex`` builds them."""
        p = self.pack_with_regex(inputs)                      # (registers the pairs; only its id lists and capture tables are used)
        refs = A.EmailRefs([i.email for i in inputs])
        lists = A.zke_regex_lists()
        lists.n_header_parts, lists.n_body_parts = p.nh, p.nb
        lists.header_part_ids, lists.body_part_ids = p.hdr_ids.ctypes.data, p.body_ids.ctypes.data
        if p.has_caps:
            lists.cap_off, lists.cap_str_off, lists.cap_blob = p.cap_off.ctypes.data, p.cap_str_off.ctypes.data, p.cap_blob.ctypes.data
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        self._check(self.lib.zke_verify_emails_with_regex(self.h, refs.arr, refs.n, C.byref(lists), out.ctypes.data), "zke_verify_emails_with_regex")
        return out[:refs.n]

    def pack_mixed(self, inputs: Sequence) -> "A.MixedLists":
        """The tables of zke_verify_emails_mixed for a sequence of ``Email`` / ``EmailWithRegex`` values: registers every pair, derives
        the configs by equal id lists (first appearance first), config_of (an ``Email`` is ``_abi.CONFIG_NONE``: verify_email only)
        and the e-mail-major capture tables."""
        index: Dict[Tuple[Tuple[int, ...], Tuple[int, ...]], int] = {}
        configs, config_of, caps = [], [], []
        for inp in inputs:
            if isinstance(inp, Email):
                config_of.append(A.CONFIG_NONE)
                caps.append(None)
                continue
            hp, bp = list(inp.regex_info.header_parts or []), list(inp.regex_info.body_parts or [])
            key = (tuple(self.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in hp),
                   tuple(self.dfa_register(p.verify_re.fwd, p.verify_re.bwd) for p in bp))
            if key not in index:
                if len(configs) == A.MIXED_MAX_CONFIGS:
                    raise EngineError("more than ZKE_MIXED_MAX_CONFIGS regex configs in one batch; split it")
                index[key] = len(configs)
                configs.append(key)
            config_of.append(index[key])
            caps.append([list(p.captures or []) for p in hp + bp])
        return A.MixedLists(configs, config_of, caps)

    @staticmethod
    def _mixed_refs(inputs: Sequence) -> "A.EmailRefs":
        return A.EmailRefs([i if isinstance(i, Email) else i.email for i in inputs])

    def verify_emails_mixed(self, inputs: Sequence) -> np.ndarray:
        """zke_verify_emails_mixed: ``Email`` and ``EmailWithRegex`` values in one batch, every EmailWithRegex with its own RegexInfo
        (core/src/circuits.rs:31-68 takes them one at a time).  Record i is what verify_emails_with_regex gives input i in a batch
        of its own config, or what verify_emails gives an ``Email``."""
        lists, refs = self.pack_mixed(inputs), self._mixed_refs(inputs)
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        self._check(self.lib.zke_verify_emails_mixed(self.h, refs.arr, refs.n, C.byref(lists.c), out.ctypes.data), "zke_verify_emails_mixed")
        return out[:refs.n]

    def verify_emails_mixed_async(self, inputs: Sequence):
        """zke_verify_emails_mixed_async: (ticket, records); the records are valid once ``wait(ticket)`` has returned."""
        lists, refs = self.pack_mixed(inputs), self._mixed_refs(inputs)
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        t = C.c_uint64()
        self._check(self.lib.zke_verify_emails_mixed_async(self.h, refs.arr, refs.n, C.byref(lists.c), out.ctypes.data, C.byref(t)),
                    "zke_verify_emails_mixed_async")
        return t.value, out[:refs.n]

    # ---- the verifier outputs encoded on the device (core/src/io.rs:28-44): ABI bytes and their SHA-256 per e-mail
    def _encoded_call(self, inputs: Sequence, form: Optional[str], bytes_cap: Optional[int], infos_cap: Optional[int]) -> "_EncodedCall":
        return _EncodedCall(self, inputs, form, bytes_cap, infos_cap)

    def verify_emails_encoded(self, inputs: Sequence, *, form: Optional[str] = None, bytes_cap: Optional[int] = None,
                              infos_cap: Optional[int] = None):
        """zke_verify_emails_encoded over ``Email`` / ``EmailWithRegex`` values: (records, encoded) with ``encoded[i]`` =
        (encoding, digest) — VerificationOutput::from_parts(..).abi_encode() and its SHA-256 — or (b"", 32 zero bytes) for an e-mail
        whose record is not ZKE_OK.  `form`: "plain" (every input an Email: zke_verify_emails' pipeline), "lists" (EmailWithRegex
        values that share one part list) or "mixed" (any of both, a RegexInfo per value); None picks the first that fits.
        `bytes_cap` / `infos_cap`: the buffers' sizes (default: exact); too small raises EngineError(ZKE_E_NOMEM)."""
        c = self._encoded_call(inputs, form, bytes_cap, infos_cap)
        self._check(self.lib.zke_verify_emails_encoded(self.h, c.refs.arr, c.refs.n, C.byref(c.c), c.out.ctypes.data, C.byref(c.enc.c)),
                    "zke_verify_emails_encoded")
        return c.records, c.enc.result()

    def verify_emails_encoded_async(self, inputs: Sequence, *, form: Optional[str] = None, bytes_cap: Optional[int] = None,
                                    infos_cap: Optional[int] = None):
        """zke_verify_emails_encoded_async: (ticket, pending); ``pending.records`` and ``pending.enc.result()`` are valid once
        ``wait(ticket)`` has returned.  `pending` keeps the output arrays (and the input tables) alive: hold on to it until then."""
        c = self._encoded_call(inputs, form, bytes_cap, infos_cap)
        t = C.c_uint64()
        self._check(self.lib.zke_verify_emails_encoded_async(self.h, c.refs.arr, c.refs.n, C.byref(c.c), c.out.ctypes.data, C.byref(c.enc.c),
                                                             C.byref(t)), "zke_verify_emails_encoded_async")
        return t.value, c

    def encode_outputs(self, outputs: Sequence, statuses: Optional[Sequence[int]] = None, *, bytes_cap: Optional[int] = None,
                       guard: int = 0, fill: int = 0) -> "A.EncodedBuffers":
        """zke_encode_outputs over EmailVerifierOutput / EmailWithRegexVerifierOutput values (or a prepared ``_abi.EncodeTables``): the
        encode and digest launches alone.  `statuses`: the records' statuses (default ZKE_OK: everything is encoded).  Returns the
        buffers; ``.result()`` is the (encoding, digest) list.  `guard` / `fill`: bytes behind bytes_cap and the buffer's initial
        value, for tests that watch what is written."""
        tb = outputs if isinstance(outputs, A.EncodeTables) else A.EncodeTables(outputs, statuses)
        need = A.zke_encoded_out()
        rc = self.lib.zke_encode_outputs(self.h, tb.records.ctypes.data, tb.n, tb.kinds.ctypes.data, tb.ext.off.ctypes.data,
                                         tb.ext.str_off.ctypes.data, tb.ext.blob.ctypes.data, tb.matches.off.ctypes.data,
                                         tb.matches.str_off.ctypes.data, tb.matches.blob.ctypes.data, C.byref(need))
        if rc not in (0, -3):
            self._check(rc, "zke_encode_outputs")
        enc = A.EncodedBuffers(tb.n, int(need.bytes_need) if bytes_cap is None else bytes_cap, guard, fill)
        self._check(self.lib.zke_encode_outputs(self.h, tb.records.ctypes.data, tb.n, tb.kinds.ctypes.data, tb.ext.off.ctypes.data,
                                                tb.ext.str_off.ctypes.data, tb.ext.blob.ctypes.data, tb.matches.off.ctypes.data,
                                                tb.matches.str_off.ctypes.data, tb.matches.blob.ctypes.data, C.byref(enc.c)),
                    "zke_encode_outputs")
        return enc

    def verify_emails_async(self, refs: "A.EmailRefs"):
        """zke_verify_emails_async: (ticket, records); the records are valid once ``wait(ticket)`` has returned."""
        out = np.zeros(max(refs.n, 1), dtype=A.RESULT_DTYPE)
        t = C.c_uint64()
        self._check(self.lib.zke_verify_emails_async(self.h, refs.arr, refs.n, out.ctypes.data, C.byref(t)), "zke_verify_emails_async")
        return t.value, out[:refs.n]

    def verify_email(self, email: Email) -> EmailVerifierOutput:
        """core/src/circuits.rs:9-29, through the single-e-mail C entry point zke_verify_email."""
        keep, args = self._email_args(email)
        out = np.zeros(1, dtype=A.RESULT_DTYPE)
        self._check(self.lib.zke_verify_email(self.h, *args, out.ctypes.data), "zke_verify_email")
        r = out[0]
        if r["status"] != A.ZKE_OK:
            raise VerifyPanic(int(r["status"]), int(r["detail"]))
        return _email_output(email, r)

    def verify_email_with_regex(self, inp: EmailWithRegex) -> EmailWithRegexVerifierOutput:
        """core/src/circuits.rs:31-68, through the single-e-mail C entry point zke_verify_email_with_regex."""
        keep, args = self._email_args(inp.email)
        hold = []

        def parts_array(parts):
            parts = list(parts or [])
            arr = (A.zke_regex_part * max(len(parts), 1))()
            for k, p in enumerate(parts):
                f = np.frombuffer(p.verify_re.fwd or b"\0", np.uint8)
                b = np.frombuffer(p.verify_re.bwd or b"\0", np.uint8)
                caps = [c.encode("utf-8") if isinstance(c, str) else bytes(c) for c in (p.captures or [])]
                bufs = [np.frombuffer(c or b"\0", np.uint8) for c in caps]
                ptrs = (C.c_void_p * max(len(caps), 1))(*[x.ctypes.data for x in bufs])
                lens = (C.c_size_t * max(len(caps), 1))(*[len(c) for c in caps])
                hold.extend([f, b, bufs, ptrs, lens])
                arr[k].fwd, arr[k].fwd_len = f.ctypes.data, len(p.verify_re.fwd)
                arr[k].bwd, arr[k].bwd_len = b.ctypes.data, len(p.verify_re.bwd)
                arr[k].n_captures = len(caps)
                arr[k].captures = C.cast(ptrs, C.POINTER(C.c_void_p))
                arr[k].capture_lens = C.cast(lens, C.POINTER(C.c_size_t))
            return arr, len(parts)

        ha, nh = parts_array(inp.regex_info.header_parts)
        ba, nb = parts_array(inp.regex_info.body_parts)
        out = np.zeros(1, dtype=A.RESULT_DTYPE)
        self._check(self.lib.zke_verify_email_with_regex(self.h, *args, ha, nh, ba, nb, out.ctypes.data),
                    "zke_verify_email_with_regex")
        r = out[0]
        if r["status"] != A.ZKE_OK:
            raise VerifyPanic(int(r["status"]), int(r["detail"]))
        return EmailWithRegexVerifierOutput(_email_output(inp.email, r), regex_matches_of(inp))


def _email_output(email: Email, r) -> EmailVerifierOutput:
    ext: List[str] = []
    for x in email.external_inputs:            # circuits.rs:18-27
        ext += [x.name, x.value]
    return EmailVerifierOutput(bytes(r["from_domain_hash"]), bytes(r["public_key_hash"]), ext)


def regex_matches_of(inp: EmailWithRegex) -> List[str]:
    """regex_matches = header captures ++ body captures (circuits.rs:58-62); the strings are the
    *input* capture strings (regex.rs:47), valid only once the engine reported OK."""
    out: List[str] = []
    for parts in (inp.regex_info.header_parts, inp.regex_info.body_parts):
        for p in parts or []:
            out += list(p.captures or [])
    return out


_default: Optional[Engine] = None


def default_engine() -> Engine:
    global _default
    if _default is None:
        _default = Engine()
    return _default


def verify_email(email: Email) -> EmailVerifierOutput:
    return default_engine().verify_email(email)


def verify_email_with_regex(inp: EmailWithRegex) -> EmailWithRegexVerifierOutput:
    return default_engine().verify_email_with_regex(inp)


def extract_email_body(raw: bytes, *, engine: Optional[Engine] = None) -> bytes:
    """extract_email_body(&parse_mail(raw).unwrap()) (core/src/email.rs:7-23): the decoded body, or VerifyPanic where the reference
    panics (email.rs:26 the parse, email.rs:17-21 get_body_raw) or the input is outside what the engine decides."""
    f = (engine or default_engine()).extract_bodies([raw])[0]
    if f.status != A.ZKE_OK:
        raise VerifyPanic(f.status, f.detail)
    return f.body


def generate_email_with_regex_inputs(emails: Sequence[Email], regex_config, *, unicode: bool = True, engine: Optional[Engine] = None):
    """helpers/src/generator.rs:55-87 generate_email_with_regex_inputs for a batch, minus the DNS key fetch and the file IO: the
    e-mails (raw bytes, from_domain and key already at hand) and a regex_config in, one EmailWithRegex per e-mail out — values
    `verify_emails_with_regex` accepts.  Raises VerifyPanic for the first e-mail the reference would have returned an error for
    ("Input doesn't match regex pattern", "Capture group not found") or panicked on."""
    eng = engine or default_engine()
    records, infos = eng.extract_captures(emails, regex_config, unicode=unicode)
    for i, r in enumerate(records):
        if r["status"] != A.ZKE_OK:
            raise VerifyPanic(int(r["status"]), int(r["detail"]), i)
    return [EmailWithRegex(e, info) for e, info in zip(emails, infos)]


def generate_email_with_regex_inputs_mixed(emails: Sequence[Email], regex_configs: Sequence, *, unicode: bool = True,
                                           engine: Optional[Engine] = None):
    """generate_email_with_regex_inputs for e-mails that carry different regex configs (`regex_configs[i]`: a RegexConfig, its JSON
    dict, or None), one batch: an EmailWithRegex per e-mail with a config, the Email itself for one without — values
    `Engine.verify_emails_mixed` accepts.  Raises VerifyPanic as generate_email_with_regex_inputs does."""
    eng = engine or default_engine()
    records, infos = eng.extract_captures_mixed(emails, regex_configs, unicode=unicode)
    for i, r in enumerate(records):
        if r["status"] != A.ZKE_OK:
            raise VerifyPanic(int(r["status"]), int(r["detail"]), i)
    return [e if cfg is None else EmailWithRegex(e, info) for e, cfg, info in zip(emails, regex_configs, infos)]


NO_SIGNATURES = "No DKIM signatures found"                        # helpers/src/generator.rs:21
NO_VALID_KEY = "No valid DKIM key found for any signature"        # helpers/src/generator.rs:52


def _scan_candidates(eng, from_domains, raw_emails, fetch, max_sigs):
    """The scan and the resolver loop: `fetch(from_domain, selector)` once per distinct pair -> (scans, per-e-mail answers)."""
    scans = eng.scan_signatures(raw_emails, from_domains, max_sigs)
    cache: Dict[Tuple[str, bytes], object] = {}
    cands: List[list] = []
    for dom, sc in zip(from_domains, scans):
        row = []
        for sig in sc.sigs:
            if sig.code != 0:
                continue
            k = (dom, sig.selector)
            if k not in cache:
                cache[k] = fetch(dom, sig.selector)
            row.append(cache[k])
        cands.append(row)
    return scans, cands


def _emails_of_selection(from_domains, raw_emails, external_inputs, max_sigs, scans, cands, records, chosen, key_of) -> List[Email]:
    """generator.rs:36-52 over a selection's answer: one Email per e-mail under `key_of(i, k)`, or the reference's Err."""
    def err(status, detail, i, reason):
        e = VerifyPanic(status, detail, i)
        e.reason = reason
        e.args = (f"email {i}: {reason} ({A.STATUS_NAMES.get(status, status)}, detail {detail})",)
        return e

    out = []
    for i, sc in enumerate(scans):
        if sc.status != A.ZKE_OK:
            raise err(sc.status, sc.detail, i, "parse_mail failed" if sc.status == A.ZKE_PARSE_FAIL else "outside what the engine implements")
        if sc.n_signatures == 0:
            raise err(A.ZKE_DKIM_NOT_PASS, A.D_NO_SIGNATURE, i, NO_SIGNATURES)
        if sc.n_candidates > len(cands[i]) and int(chosen[i]) == A.SEL_NONE:
            raise err(A.ZKE_UNSUPPORTED, A.D_U_TOO_MANY_SIGS, i, f"more than {max_sigs} DKIM-Signature headers: the list was cut before a key passed")
        if int(chosen[i]) == A.SEL_NONE:
            r = records[i]
            st = int(r["status"]) if int(r["status"]) == A.ZKE_UNSUPPORTED else A.ZKE_DKIM_NOT_PASS
            raise err(st, int(r["detail"]), i, NO_VALID_KEY)
        if int(chosen[i]) & A.SEL_AFTER_UNSUPPORTED:
            raise err(A.ZKE_UNSUPPORTED, A.D_U_ALGO_ED25519, i, "a candidate in front of the passing key is outside what the engine implements")
        key = key_of(i, int(chosen[i]))
        ext = list(external_inputs[i] or []) if external_inputs is not None else []
        out.append(Email(from_domains[i], bytes(raw_emails[i]), A.PublicKey(bytes(key.key), key.key_type), ext))
    return out


def generate_email_inputs(from_domains: Sequence[str], raw_emails: Sequence[bytes],
                          fetch_key: Callable[[str, bytes], Optional["A.PublicKey"]],
                          external_inputs: Optional[Sequence[Optional[Sequence["A.ExternalInput"]]]] = None, *,
                          max_sigs: int = A.SCAN_MAX_SIGS, engine: Optional[Engine] = None) -> List[Email]:
    """helpers/src/generator.rs:11-53 generate_email_inputs for a batch: scan the DKIM-Signature headers on the GPU, ask
    `fetch_key(from_domain, selector)` — the caller's resolver, the only place network code would live; called once per distinct
    pair, on the host, between the two GPU calls; None: the fetch failed — for the key of every candidate, and keep the first key
    under which the e-mail verifies.  Returns one Email per e-mail.  Raises VerifyPanic (its ``reason`` holds the reference's text)
    for the first e-mail where the reference returns Err: a parse_mail error, "No DKIM signatures found", "No valid DKIM key found
    for any signature".  An e-mail whose answer the engine cannot give (ZKE_UNSUPPORTED) raises too, with that status."""
    eng = engine or default_engine()
    scans, cands = _scan_candidates(eng, from_domains, raw_emails, fetch_key, max_sigs)
    probe = [Email(d, bytes(r), A.PublicKey(b"")) for d, r in zip(from_domains, raw_emails)]
    records, chosen = eng.select_keys(probe, cands)
    return _emails_of_selection(from_domains, raw_emails, external_inputs, max_sigs, scans, cands, records, chosen, lambda i, k: cands[i][k])


def generate_email_inputs_from_records(from_domains: Sequence[str], raw_emails: Sequence[bytes],
                                       fetch_record: Callable[[str, bytes], Optional[bytes]],
                                       external_inputs: Optional[Sequence[Optional[Sequence["A.ExternalInput"]]]] = None, *,
                                       mode: int = A.KEYREC_DNS, max_sigs: int = A.SCAN_MAX_SIGS, engine: Optional[Engine] = None) -> List[Email]:
    """generate_email_inputs with the resolver's RAW answers: `fetch_record(from_domain, selector)` returns the TXT record of
    selector._domainkey.from_domain as bytes (the character-strings of a multi-string answer joined; `mode` = _abi.KEYREC_DNS) or
    the archive's `value` (_abi.KEYREC_ARCHIVE), None when the fetch failed.  Turning the record into the (key, key_type) pair —
    helpers/src/dkim.rs:67-111: base64, SubjectPublicKeyInfo or PKCS#1 in, PKCS#1 out — happens on the GPU in front of the verify
    launches (zke_select_keys_from_records); the caller is left with network code only.  Errors as generate_email_inputs."""
    eng = engine or default_engine()
    scans, cands = _scan_candidates(eng, from_domains, raw_emails, fetch_record, max_sigs)
    probe = [Email(d, bytes(r), A.PublicKey(b"")) for d, r in zip(from_domains, raw_emails)]
    records, chosen, infos = eng.select_keys_from_records(probe, cands, mode)
    return _emails_of_selection(from_domains, raw_emails, external_inputs, max_sigs, scans, cands, records, chosen,
                                lambda i, k: infos[i][k].public_key())


def abi_encode_native(email: EmailVerifierOutput, matches: Optional[Sequence[str]] = None) -> bytes:
    """VerificationOutput::from_parts(email, matches).abi_encode() (core/src/io.rs:28-44) through the C entry point
    zke_abi_encode — what a zkVM host linking the C-ABI commits as public values.  (zkemail.rs_amd/abi_encode.py is the
    same encoding in Python, with the decoder of helpers/src/io.rs.)"""
    lib = load_library()

    def table(strs):
        bs = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strs]
        bufs = [np.frombuffer(b or b"\0", np.uint8) for b in bs]
        ptrs = (C.c_void_p * max(len(bs), 1))(*[x.ctypes.data for x in bufs])
        lens = (C.c_size_t * max(len(bs), 1))(*[len(b) for b in bs])
        return bufs, ptrs, lens, len(bs)

    fd = np.frombuffer(bytes(email.from_domain_hash), np.uint8)
    pk = np.frombuffer(bytes(email.public_key_hash), np.uint8)
    if len(fd) != 32 or len(pk) != 32:                                    # io.rs:49-50 try_into().unwrap()
        raise ValueError("hashes must be 32 bytes")
    k1, p1, l1, n1 = table(email.external_inputs)
    k2, p2, l2, n2 = table(matches or [])
    need = C.c_size_t()
    args = [fd.ctypes.data, pk.ctypes.data, p1, l1, n1, 0 if matches is None else 1, p2, l2, n2]
    rc = lib.zke_abi_encode(*args, None, 0, C.byref(need))
    if rc != 0:
        raise EngineError(f"zke_abi_encode failed ({rc})")
    out = np.zeros(need.value, np.uint8)
    rc = lib.zke_abi_encode(*args, out.ctypes.data, need.value, C.byref(need))
    if rc != 0:
        raise EngineError(f"zke_abi_encode failed ({rc})")
    return out.tobytes()
