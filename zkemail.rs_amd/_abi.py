"""ctypes mirror of include/zkemail_amd.h (struct layouts, status codes) and the
struct-of-arrays packing of ``&[Email]`` / ``&[EmailWithRegex]`` that the C-ABI takes.

Nothing here computes anything on the verify path; it only marshals buffers.
Reference types: core/src/structs.rs:8-75.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

# ---- status codes (include/zkemail_amd.h) -------------------------------------------
ZKE_OK = 0
ZKE_PARSE_FAIL = 1
ZKE_KEY_DECODE_FAIL = 2
ZKE_DKIM_ERROR = 3
ZKE_DKIM_NOT_PASS = 4
ZKE_EXTERNAL_INPUT_NULL = 5
ZKE_CANON_FAIL = 6
ZKE_DFA_DECODE_FAIL = 7
ZKE_HEADER_REGEX_FAIL = 8
ZKE_BODY_REGEX_FAIL = 9
ZKE_UNSUPPORTED = 10
ZKE_BODY_DECODE_FAIL = 11

STATUS_NAMES = {
    0: "OK", 1: "PARSE_FAIL", 2: "KEY_DECODE_FAIL", 3: "DKIM_ERROR", 4: "DKIM_NOT_PASS",
    5: "EXTERNAL_INPUT_NULL", 6: "CANON_FAIL", 7: "DFA_DECODE_FAIL", 8: "HEADER_REGEX_FAIL",
    9: "BODY_REGEX_FAIL", 10: "UNSUPPORTED", 11: "BODY_DECODE_FAIL",
}
# the reference panic site each status stands for
STATUS_SITE = {
    1: "core/src/email.rs:26", 2: "core/src/email.rs:29", 3: "core/src/email.rs:33",
    4: "core/src/circuits.rs:13", 5: "core/src/circuits.rs:24", 6: "core/src/circuits.rs:35",
    7: "core/src/regex.rs:32-33", 8: "core/src/circuits.rs:45", 9: "core/src/circuits.rs:54",
    10: "outside this engine's implemented subset", 11: "core/src/email.rs:17-21",
}

D_NONE = 0
D_NEUTRAL = 1
D_SIG_SYNTAX = 2
D_MISSING_TAG = 3
D_INCOMPATIBLE_VERSION = 4
D_DOMAIN_MISMATCH = 5
D_FROM_NOT_SIGNED = 6
D_BAD_QUERY_METHOD = 7
D_BAD_CANON = 8
D_BAD_ALGO = 9
D_BAD_LENGTH = 10
D_BODY_HASH_MISMATCH = 11
D_SIG_B64 = 12
D_SIG_MISMATCH = 13
D_SIG_EXPIRED = 14
D_HDR_LEADING_SPACE = 20
D_HDR_LONE_CR = 21
D_SUBPART_LEADING_SPACE = 23
D_SUBPART_LONE_CR = 24
D_KEY_TYPE = 30
D_KEY_DER = 31
D_KEY_RANGE = 32
D_KEY_ED25519_POINT = 33
D_NO_SIGNATURE = 40
D_U_ALGO_SHA1 = 50
D_U_ALGO_ED25519 = 51
D_U_SIG_NON_ASCII = 52
D_U_TOO_MANY_HEADERS = 53
D_U_PREIMAGE_OVERFLOW = 54
D_U_EVEN_MODULUS = 55
D_U_TOO_MANY_TAGS = 56
D_U_CAPTURE_FFFD = 57
D_U_EMAIL_TOO_LARGE = 58
D_RE_MATCH_COUNT = 60
D_RE_CAPTURE_MISSING = 61
D_RE_QUIT = 62
D_U_SIG_TOO_LONG = 63
D_U_TOO_MANY_SIGS = 64
D_U_SIG_B_REPEATED = 65
D_U_DOMAIN_FOLD = 66
D_U_MIME_CTYPE = 67
D_U_MIME_BOUNDARY = 68
D_U_MIME_DEPTH = 69
D_DFA_LABEL, D_DFA_ENDIAN_VERSION, D_DFA_FLAGS, D_DFA_TRANSITIONS, D_DFA_START_TABLE = 70, 71, 72, 73, 74
D_DFA_MATCH_STATES, D_DFA_SPECIAL, D_DFA_ACCELS, D_DFA_QUITSET, D_DFA_UNREGISTERED = 75, 76, 77, 78, 79
D_DFA_BWD_OFFSET = 10
D_RE_GROUP_MISSING = 90
D_U_CAPTURE_STATES, D_U_CAPTURE_SPAN, D_U_CAPTURE_WALK, D_U_CAPTURE_PROGRAM = 91, 92, 93, 94
CAP_MAX_STATES, CAP_MAX_PROGRAM_GROUPS, CAP_MAX_GROUPS, CAP_MAX_SPAN, CAP_MAX_PARTS = 8192, 32, 16, 4096, 16
CAPF_NOT_UTF8 = 1

KEY_RSA, KEY_ED25519, KEY_OTHER = 0, 1, 2
F_HDR_RELAXED, F_BODY_RELAXED, F_HAS_LENGTH, F_SHA1, F_ED25519 = 1, 2, 4, 8, 16


class zke_result(C.Structure):
    _fields_ = [
        ("status", C.c_uint32), ("detail", C.c_uint32), ("sig_index", C.c_uint32), ("flags", C.c_uint32),
        ("canon_header_len", C.c_uint32), ("canon_body_len", C.c_uint32),
        ("body_offset", C.c_uint32), ("n_headers", C.c_uint32),
        ("from_domain_hash", C.c_uint8 * 32), ("public_key_hash", C.c_uint8 * 32),
        ("body_hash", C.c_uint8 * 32), ("header_hash", C.c_uint8 * 32),
        ("regex_part", C.c_uint32), ("match_count", C.c_uint32),
        ("match_start", C.c_uint32), ("match_end", C.c_uint32),
        ("rsa_bits", C.c_uint32), ("reserved", C.c_uint32 * 3),
    ]


assert C.sizeof(zke_result) == 192

RESULT_DTYPE = np.dtype([
    ("status", "<u4"), ("detail", "<u4"), ("sig_index", "<u4"), ("flags", "<u4"),
    ("canon_header_len", "<u4"), ("canon_body_len", "<u4"), ("body_offset", "<u4"), ("n_headers", "<u4"),
    ("from_domain_hash", "u1", 32), ("public_key_hash", "u1", 32), ("body_hash", "u1", 32), ("header_hash", "u1", 32),
    ("regex_part", "<u4"), ("match_count", "<u4"), ("match_start", "<u4"), ("match_end", "<u4"),
    ("rsa_bits", "<u4"), ("reserved", "<u4", 3),
])
assert RESULT_DTYPE.itemsize == 192

# What verify_email returns per e-mail (EmailVerifierOutput, core/src/structs.rs:64-69, plus the panic site): the part of
# a zke_result the ranks of a multi-GPU job exchange.  Bytes [0, 8) and [32, 96) of the record.
WITNESS_DTYPE = np.dtype([("status", "<u4"), ("detail", "<u4"), ("from_domain_hash", "u1", 32), ("public_key_hash", "u1", 32)])
assert WITNESS_DTYPE.itemsize == 72


class zke_batch(C.Structure):
    _fields_ = [
        ("n", C.c_uint32),
        ("raw_blob", C.c_void_p), ("raw_off", C.c_void_p),
        ("domain_blob", C.c_void_p), ("domain_off", C.c_void_p),
        ("key_blob", C.c_void_p), ("key_off", C.c_void_p),
        ("key_type", C.c_void_p), ("ext_null", C.c_void_p),
        ("with_regex", C.c_uint32), ("n_header_parts", C.c_uint32), ("n_body_parts", C.c_uint32),
        ("header_part_ids", C.c_void_p), ("body_part_ids", C.c_void_p),
        ("cap_off", C.c_void_p), ("cap_str_off", C.c_void_p), ("cap_blob", C.c_void_p),
    ]


class zke_debug_out(C.Structure):
    _fields_ = [
        ("canon_header", C.c_void_p), ("canon_header_stride", C.c_size_t),
        ("canon_body", C.c_void_p), ("canon_body_stride", C.c_size_t),
        ("clean_body", C.c_void_p), ("clean_body_stride", C.c_size_t),
        ("em", C.c_void_p), ("em_stride", C.c_size_t),
        ("canon_body_full_len", C.c_void_p),
        ("rsa_route", C.c_void_p),
    ]


class zke_regex_part(C.Structure):
    """One CompiledRegex (core/src/structs.rs:24-27) as zke_verify_email_with_regex takes it."""
    _fields_ = [
        ("fwd", C.c_void_p), ("fwd_len", C.c_size_t), ("bwd", C.c_void_p), ("bwd_len", C.c_size_t),
        ("n_captures", C.c_uint32), ("captures", C.POINTER(C.c_void_p)), ("capture_lens", C.POINTER(C.c_size_t)),
    ]


class zke_capture_part(C.Structure):
    """One part of an extraction (zke_extract_captures): the DFA pair that finds the match, the capture program, the groups."""
    _fields_ = [("dfa_id", C.c_uint32), ("prog_id", C.c_uint32), ("n_groups", C.c_uint32), ("groups", C.c_void_p)]


class zke_capture_out(C.Structure):
    """Caller-sized buffers of an extraction; capacities in entries, the sizes needed written back."""
    _fields_ = [
        ("spans", C.c_void_p), ("spans_cap", C.c_size_t), ("flags", C.c_void_p), ("flags_cap", C.c_size_t),
        ("cap_off", C.c_void_p), ("cap_off_cap", C.c_size_t), ("cap_str_off", C.c_void_p), ("cap_str_off_cap", C.c_size_t),
        ("cap_blob", C.c_void_p), ("cap_blob_cap", C.c_size_t),
        ("spans_need", C.c_size_t), ("flags_need", C.c_size_t), ("cap_off_need", C.c_size_t), ("cap_str_off_need", C.c_size_t),
        ("cap_blob_need", C.c_size_t), ("n_strings", C.c_size_t),
    ]


QP_NO_INDEX = 0xFFFFFFFF
ORGF_SPLIT, ORGF_PADDING = 1, 2
UTF8_LOSSY_MAX_BYTES = (2 ** 32 - 1) // 3     # zke_utf8_lossy_batch: the repaired offsets are 32-bit


class zke_capture_origin(C.Structure):
    """Where the spans of a mapped extraction lie before the QP filter (zke_extract_captures_mapped); capacities in entries."""
    _fields_ = [
        ("spans", C.c_void_p), ("spans_cap", C.c_size_t), ("flags", C.c_void_p), ("flags_cap", C.c_size_t),
        ("spans_need", C.c_size_t), ("flags_need", C.c_size_t),
    ]


SCAN_MAX_SIGS = 64
SIG_ALGO_RSA_SHA256, SIG_ALGO_RSA_SHA1, SIG_ALGO_ED25519_SHA256, SIG_ALGO_OTHER = 0, 1, 2, 3
SEL_NONE, SEL_AFTER_UNSUPPORTED = 0xFFFFFFFF, 0x80000000
MAX_HEADERS, MAX_TAGS, MAX_TAGBUF = 256, 32, 2048


class zke_sig_info(C.Structure):
    """One DKIM-Signature header of a scan (zke_scan_signatures)."""
    _fields_ = [("header_index", C.c_uint32), ("code", C.c_uint32), ("algo", C.c_uint32), ("sel_off", C.c_uint32), ("sel_len", C.c_uint32),
                ("val_start", C.c_uint32), ("val_end", C.c_uint32), ("reserved", C.c_uint32)]


SIG_INFO_DTYPE = np.dtype([("header_index", "<u4"), ("code", "<u4"), ("algo", "<u4"), ("sel_off", "<u4"), ("sel_len", "<u4"),
                           ("val_start", "<u4"), ("val_end", "<u4"), ("reserved", "<u4")])
assert C.sizeof(zke_sig_info) == 32 == SIG_INFO_DTYPE.itemsize


class zke_sig_scan(C.Structure):
    """Caller-sized buffers of a scan; capacities in entries, the sizes needed written back."""
    _fields_ = [
        ("scan_status", C.c_void_p), ("scan_status_cap", C.c_size_t), ("sig_off", C.c_void_p), ("sig_off_cap", C.c_size_t),
        ("sigs", C.c_void_p), ("sigs_cap", C.c_size_t), ("sel_blob", C.c_void_p), ("sel_blob_cap", C.c_size_t),
        ("scan_status_need", C.c_size_t), ("sig_off_need", C.c_size_t), ("sigs_need", C.c_size_t), ("sel_blob_need", C.c_size_t),
        ("n_sigs", C.c_size_t),
    ]


class zke_key_ref(C.Structure):
    """One candidate key of zke_select_keys; key_len 0: the fetch failed."""
    _fields_ = [("key", C.c_void_p), ("key_len", C.c_size_t), ("key_type", C.c_uint32), ("reserved", C.c_uint32)]


# DKIM key records (zke_decode_key_records, zke_select_keys_from_records)
KEYREC_ARCHIVE, KEYREC_DNS = 0, 1
KEYREC_MAX_BYTES = 4096
(D_KEYREC_NO_KEY, D_KEYREC_B64, D_KEYREC_TYPE, D_KEYREC_DER, D_KEYREC_RANGE, D_KEYREC_ED25519_LEN, D_KEYREC_VERSION, D_KEYREC_SYNTAX,
 D_KEYREC_NON_ASCII_EDGE, D_KEYREC_TOO_LONG) = range(100, 110)
KEYREC_NAMES = {0: "ok", 100: "no key", 101: "base64", 102: "unsupported key type", 103: "DER", 104: "range", 105: "Ed25519 length",
                106: "version", 107: "tag-list syntax", 108: "non-ASCII edge", 109: "record too long"}


class zke_keyrec_ref(C.Structure):
    """One record of zke_decode_key_records; len 0: the fetch failed."""
    _fields_ = [("txt", C.c_void_p), ("len", C.c_size_t)]


class zke_key_info(C.Structure):
    """What one record decodes to."""
    _fields_ = [("code", C.c_uint32), ("key_type", C.c_uint32), ("key_off", C.c_uint32), ("key_len", C.c_uint32)]


KEY_INFO_DTYPE = np.dtype([("code", "<u4"), ("key_type", "<u4"), ("key_off", "<u4"), ("key_len", "<u4")])
assert C.sizeof(zke_key_info) == 16 == KEY_INFO_DTYPE.itemsize


class zke_keyrec_out(C.Structure):
    """Caller-sized buffers of a decode; capacities in entries, the sizes needed written back."""
    _fields_ = [("infos", C.c_void_p), ("infos_cap", C.c_size_t), ("keys", C.c_void_p), ("keys_cap", C.c_size_t),
                ("infos_need", C.c_size_t), ("keys_need", C.c_size_t)]


# extract_email_body for whole batches (zke_extract_bodies)
BODYF_PART_KEEPS_EOL = 1
CTE_IDENTITY, CTE_BASE64, CTE_QP = 0, 1, 2
D_BODY_B64_CHAR, D_BODY_B64_LENGTH, D_BODY_B64_TRAILING_BITS, D_U_BODY_CTE = 110, 111, 112, 113
BODY_PART_HTML = 0x80000000          # zke_body_info.part, bit 31: chosen as text/html


class zke_body_info(C.Structure):
    """What one e-mail's extraction gives: verdict, the chosen part, its body_bytes in the raw e-mail, the decoded bytes."""
    _fields_ = [("status", C.c_uint32), ("detail", C.c_uint32), ("part", C.c_uint32), ("encoding", C.c_uint32), ("src_off", C.c_uint32),
                ("src_len", C.c_uint32), ("body_len", C.c_uint32), ("reserved", C.c_uint32), ("body_off", C.c_uint64)]


BODY_INFO_DTYPE = np.dtype([("status", "<u4"), ("detail", "<u4"), ("part", "<u4"), ("encoding", "<u4"), ("src_off", "<u4"),
                            ("src_len", "<u4"), ("body_len", "<u4"), ("reserved", "<u4"), ("body_off", "<u8")])
assert C.sizeof(zke_body_info) == 40 == BODY_INFO_DTYPE.itemsize


class zke_body_out(C.Structure):
    """Caller-sized buffers of an extraction; capacities in entries, the sizes needed written back."""
    _fields_ = [("infos", C.c_void_p), ("infos_cap", C.c_size_t), ("bytes", C.c_void_p), ("bytes_cap", C.c_size_t),
                ("infos_need", C.c_size_t), ("bytes_need", C.c_size_t)]


STRICT_FLAGS = ("enforce_expiry_x", "canon_takes_verified_signature", "canon_ignores_l", "i_must_be_subdomain",
                "b_removes_own_span_only")          # zke_options' strictness flags, in ZKE_STRICT_* bit order


class zke_email_ref(C.Structure):
    """One Email with buffers of its own (zke_verify_emails): what `&[Email]` holds in the reference."""
    _fields_ = [
        ("raw", C.c_void_p), ("raw_len", C.c_size_t), ("from_domain", C.c_void_p), ("domain_len", C.c_size_t),
        ("key", C.c_void_p), ("key_len", C.c_size_t), ("key_type", C.c_uint32), ("external_input_null", C.c_uint32),
    ]


class zke_regex_lists(C.Structure):
    _fields_ = [
        ("n_header_parts", C.c_uint32), ("header_part_ids", C.c_void_p), ("n_body_parts", C.c_uint32), ("body_part_ids", C.c_void_p),
        ("cap_off", C.c_void_p), ("cap_str_off", C.c_void_p), ("cap_blob", C.c_void_p),
    ]


MIXED_MAX_CONFIGS = 64           # ZKE_MIXED_MAX_CONFIGS
MIXED_MAX_PARTS = 64             # ZKE_MIXED_MAX_PARTS
CONFIG_NONE = 0xFFFFFFFF         # ZKE_CONFIG_NONE: config_of[i] of an e-mail that is verify_email only


class zke_regex_config(C.Structure):
    """One RegexInfo's part lists (zke_verify_emails_mixed)."""
    _fields_ = [
        ("n_header_parts", C.c_uint32), ("header_part_ids", C.c_void_p), ("n_body_parts", C.c_uint32), ("body_part_ids", C.c_void_p),
    ]


class zke_regex_mixed(C.Structure):
    _fields_ = [
        ("n_configs", C.c_uint32), ("configs", C.POINTER(zke_regex_config)), ("config_of", C.c_void_p),
        ("cap_off", C.c_void_p), ("cap_str_off", C.c_void_p), ("cap_blob", C.c_void_p),
    ]


class MixedLists:
    """The tables of one zke_verify_emails_mixed call: the distinct configs (id lists), config_of[n], job_off[n + 1] (the prefix sum
    of the e-mails' part counts: e-mail i's part p is job job_off[i] + p, header parts first) and the capture strings per job as CSR.
    `configs`: [(header ids, body ids)]; `config_of`: per e-mail an index into it or CONFIG_NONE; `captures`: per e-mail the list
    (one entry per part, header parts first) of its parts' capture strings — [] or None for an e-mail without a config.
    Keeps the numpy buffers alive and exposes a ``zke_regex_mixed``."""

    def __init__(self, configs: Sequence[Tuple[Sequence[int], Sequence[int]]], config_of: Sequence[int],
                 captures: Optional[Sequence[Optional[Sequence[Sequence[str]]]]] = None):
        self.n = len(config_of)
        self.configs = [(list(h), list(b)) for h, b in configs]
        self.config_of = np.array(list(config_of) or [0], dtype=np.uint32)
        self._ids = [(np.array(h or [0], np.uint32), np.array(b or [0], np.uint32)) for h, b in self.configs]
        self.arr = (zke_regex_config * max(len(self.configs), 1))()
        for k, ((h, b), (ha, ba)) in enumerate(zip(self.configs, self._ids)):
            self.arr[k].n_header_parts, self.arr[k].header_part_ids = len(h), ha.ctypes.data
            self.arr[k].n_body_parts, self.arr[k].body_part_ids = len(b), ba.ctypes.data
        parts_of = [0 if c == CONFIG_NONE else len(self.configs[c][0]) + len(self.configs[c][1]) for c in config_of]
        self.job_off = np.zeros(self.n + 1, np.uint32)
        if self.n:
            self.job_off[1:] = np.cumsum(parts_of)
        strs: List[bytes] = []
        cap_off = [0]
        for i, P in enumerate(parts_of):
            per_email = list((captures[i] if captures is not None else None) or [[]] * P)
            assert len(per_email) == P, (i, len(per_email), P)
            for part_caps in per_email:
                strs.extend(s.encode("utf-8") if isinstance(s, str) else s for s in (part_caps or []))
                cap_off.append(len(strs))
        self.cap_off = np.array(cap_off, dtype=np.uint32)
        self.cap_blob, str_off = _csr(strs)
        self.cap_str_off = str_off.astype(np.uint32)
        m = self.c = zke_regex_mixed()
        m.n_configs, m.configs, m.config_of = len(self.configs), self.arr, self.config_of.ctypes.data
        if int(self.job_off[self.n]):
            m.cap_off, m.cap_str_off, m.cap_blob = self.cap_off.ctypes.data, self.cap_str_off.ctypes.data, self.cap_blob.ctypes.data


# the verifier outputs encoded on the device (zke_verify_emails_encoded, zke_encode_outputs)
ENC_KIND_EMAIL, ENC_KIND_WITH_REGEX = 0, 1       # zke_encoded_info.kind: SolEmailOutput, SolEmailWithRegexOutput


class zke_encoded_info(C.Structure):
    """One e-mail's encoding: its place in the byte blob, its length (0: not encoded), its kind, the SHA-256 of its bytes."""
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint32), ("kind", C.c_uint32), ("digest", C.c_uint8 * 32)]


ENCODED_INFO_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("kind", "<u4"), ("digest", "u1", 32)])
assert C.sizeof(zke_encoded_info) == 48 == ENCODED_INFO_DTYPE.itemsize


class zke_encoded_out(C.Structure):
    """Caller-sized buffers of an encoding; capacities in entries, the (exact) sizes needed written back."""
    _fields_ = [("infos", C.c_void_p), ("infos_cap", C.c_size_t), ("bytes", C.c_void_p), ("bytes_cap", C.c_size_t),
                ("infos_need", C.c_size_t), ("bytes_need", C.c_size_t)]


class zke_encode_in(C.Structure):
    _fields_ = [("lists", C.POINTER(zke_regex_lists)), ("mixed", C.POINTER(zke_regex_mixed)),
                ("ext_off", C.c_void_p), ("ext_str_off", C.c_void_p), ("ext_blob", C.c_void_p)]


def flat_external_inputs(inputs: Sequence["ExternalInput"]) -> List[str]:
    """Email.external_inputs as the output carries them: [name1, value1, name2, value2, ...] (circuits.rs:18-27).  (A None value
    is the reference's panic, ZKE_EXTERNAL_INPUT_NULL: such an e-mail is never encoded, and its value travels as "".)"""
    return [s for x in inputs for s in (x.name, x.value if x.value is not None else "")]


class StringTable:
    """A CSR string table as the encode entries take it: ``lists[i]`` are entry i's strings (str or bytes).  off[n + 1] indexes
    str_off[n_strings + 1], which indexes blob.  Keeps the numpy buffers alive."""

    def __init__(self, lists: Sequence[Sequence]):
        strs = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for xs in lists for s in xs]
        self.off = np.zeros(len(lists) + 1, np.uint32)
        if len(lists):
            self.off[1:] = np.cumsum([len(xs) for xs in lists])
        self.blob, so = _csr(strs)
        self.str_off = so.astype(np.uint32)
        self.n_strings = len(strs)


class EncodeTables:
    """The tables of one zke_encode_outputs call from a list of verifier outputs — EmailVerifierOutput (kind 0) or
    EmailWithRegexVerifierOutput (kind 1) values: kinds[n], the external inputs and the matches as two StringTables, and the
    hashes laid into zke_result records (status ZKE_OK unless `statuses` says otherwise)."""

    def __init__(self, outputs: Sequence, statuses: Optional[Sequence[int]] = None):
        self.n = len(outputs)
        emails = [o.email if isinstance(o, EmailWithRegexVerifierOutput) else o for o in outputs]
        self.kinds = np.array([ENC_KIND_WITH_REGEX if isinstance(o, EmailWithRegexVerifierOutput) else ENC_KIND_EMAIL for o in outputs] or [0],
                              np.uint32)
        self.ext = StringTable([e.external_inputs for e in emails])
        self.matches = StringTable([o.regex_matches if isinstance(o, EmailWithRegexVerifierOutput) else [] for o in outputs])
        self.records = np.zeros(max(self.n, 1), RESULT_DTYPE)
        for i, e in enumerate(emails):
            self.records[i]["from_domain_hash"] = np.frombuffer(bytes(e.from_domain_hash), np.uint8)
            self.records[i]["public_key_hash"] = np.frombuffer(bytes(e.public_key_hash), np.uint8)
            self.records[i]["status"] = statuses[i] if statuses is not None else ZKE_OK


class EncodedBuffers:
    """The caller-sized buffers of a zke_encoded_out (kept alive by this object) and their reading."""

    def __init__(self, n: int, nbytes: int, guard: int = 0, fill: int = 0):
        self.n, self.nbytes = n, nbytes
        self.infos = np.zeros(max(n, 1), ENCODED_INFO_DTYPE)
        self.bytes = np.full(max(nbytes + guard, 1), fill, np.uint8)
        o = self.c = zke_encoded_out()
        o.infos, o.infos_cap, o.bytes, o.bytes_cap = self.infos.ctypes.data, n, self.bytes.ctypes.data, nbytes

    def encoding(self, i: int) -> bytes:
        f = self.infos[i]
        return self.bytes[int(f["off"]):int(f["off"]) + int(f["len"])].tobytes()

    def result(self) -> List[Tuple[bytes, bytes]]:
        """Per e-mail (encoding, digest); (b"", 32 zero bytes) for an e-mail that was not encoded."""
        return [(self.encoding(i), self.infos[i]["digest"].tobytes()) for i in range(self.n)]


def encoded_len(kind: int, ext_lens: Sequence[int], match_lens: Sequence[int] = ()) -> int:
    """The plan's size rule (csrc/encode_plan.hip.h): the bytes of an encoding from its kind and its strings' lengths."""
    arr = lambda lens: 32 + sum(64 + (int(ln) + 31) // 32 * 32 for ln in lens)
    return 32 + 96 + arr(ext_lens) + ((64 + arr(match_lens)) if kind == ENC_KIND_WITH_REGEX else 0)


class zke_capture_config(C.Structure):
    """One RegexConfig of a mixed extraction (zke_extract_captures_mixed): the parts with their programs and requested groups."""
    _fields_ = [
        ("n_header_parts", C.c_uint32), ("header_parts", C.POINTER(zke_capture_part)),
        ("n_body_parts", C.c_uint32), ("body_parts", C.POINTER(zke_capture_part)),
    ]


class zke_capture_mixed(C.Structure):
    _fields_ = [("n_configs", C.c_uint32), ("configs", C.POINTER(zke_capture_config)), ("config_of", C.c_void_p)]


class CaptureMixedLists:
    """The tables of one zke_extract_captures_mixed call.  `configs`: [(header parts, body parts)], a part (dfa_id, prog_id, groups);
    `config_of`: per e-mail an index into it or CONFIG_NONE.  Derived, as the header lays them out: job_off / col_off [n + 1] (the
    prefix sums of the e-mails' part and requested-group counts), J, Gt, and per config gbase (the first column of each part among
    the config's G).  Keeps the buffers alive and exposes a ``zke_capture_mixed``."""

    def __init__(self, configs, config_of: Sequence[int]):
        self.n = len(config_of)
        self.configs = [([(int(d), int(p), [int(g) for g in gs]) for d, p, gs in h], [(int(d), int(p), [int(g) for g in gs]) for d, p, gs in b])
                        for h, b in configs]
        self.config_of = np.array(list(config_of) or [0], dtype=np.uint32)
        self.arr = (zke_capture_config * max(len(self.configs), 1))()
        self._keep = []
        self.gbase: List[List[int]] = []
        for k, (h, b) in enumerate(self.configs):
            parts = (zke_capture_part * max(len(h) + len(b), 1))()
            gb = [0]
            for j, (dfa_id, prog_id, gs) in enumerate(h + b):
                g = np.array(gs or [0], np.uint32)
                self._keep.append(g)
                parts[j].dfa_id, parts[j].prog_id, parts[j].n_groups, parts[j].groups = dfa_id, prog_id, len(gs), g.ctypes.data
                gb.append(gb[-1] + len(gs))
            self._keep.append(parts)
            self.gbase.append(gb)
            self.arr[k].n_header_parts, self.arr[k].header_parts = len(h), parts
            self.arr[k].n_body_parts = len(b)
            self.arr[k].body_parts = C.cast(C.byref(parts, len(h) * C.sizeof(zke_capture_part)), C.POINTER(zke_capture_part))
        parts_of = [0 if c == CONFIG_NONE else len(self.configs[c][0]) + len(self.configs[c][1]) for c in config_of]
        groups_of = [0 if c == CONFIG_NONE else self.gbase[c][-1] for c in config_of]
        self.job_off, self.col_off = np.zeros(self.n + 1, np.uint32), np.zeros(self.n + 1, np.uint32)
        if self.n:
            self.job_off[1:] = np.cumsum(parts_of)
            self.col_off[1:] = np.cumsum(groups_of)
        self.J, self.Gt = int(self.job_off[self.n]), int(self.col_off[self.n])
        m = self.c = zke_capture_mixed()
        m.n_configs, m.configs, m.config_of = len(self.configs), self.arr, self.config_of.ctypes.data


class EmailRefs:
    """An array of zke_email_ref over a list of Email values, pointing INTO their bytes objects (nothing is copied; the list is
    kept alive by this object)."""

    def __init__(self, emails: Sequence["Email"]):
        self.n = len(emails)
        self.arr = (zke_email_ref * max(self.n, 1))()
        self._keep = []
        ptr = lambda b: C.cast(C.c_char_p(b), C.c_void_p).value if b else None
        for i, e in enumerate(emails):
            raw, dom, key = bytes(e.raw_email), e.from_domain.encode("utf-8"), bytes(e.public_key.key)
            self._keep.append((raw, dom, key))
            r = self.arr[i]
            r.raw, r.raw_len, r.from_domain, r.domain_len, r.key, r.key_len = ptr(raw), len(raw), ptr(dom), len(dom), ptr(key), len(key)
            r.key_type = key_type_code(e.public_key.key_type)
            r.external_input_null = 1 if any(x.value is None for x in e.external_inputs) else 0


class zke_wire_email(C.Structure):
    """View of one decoded borsh / bincode record (zke_wire_decode): pointers into the caller's buffer."""
    _fields_ = [
        ("raw", C.c_void_p), ("raw_len", C.c_size_t), ("from_domain", C.c_void_p), ("domain_len", C.c_size_t),
        ("key", C.c_void_p), ("key_len", C.c_size_t), ("key_type", C.c_uint32), ("n_external_inputs", C.c_uint32),
        ("external_input_null", C.c_uint32), ("has_header_parts", C.c_uint32), ("has_body_parts", C.c_uint32),
        ("n_header_parts", C.c_uint32), ("n_body_parts", C.c_uint32),
        ("header_parts", C.POINTER(zke_regex_part)), ("body_parts", C.POINTER(zke_regex_part)),
    ]


class zke_options(C.Structure):
    """ABI 0.3: named fields; a zero-filled struct is the default configuration (device 0)."""
    _fields_ = [
        ("device", C.c_int32), ("slots", C.c_uint32), ("max_sig_rounds", C.c_uint32), ("disable_key_cache", C.c_uint32),
        ("host_threads", C.c_uint32), ("max_dfas", C.c_uint32),
        ("rsa_lane_groups", C.c_uint32), ("dfa_mapping", C.c_uint32), ("replay_graphs", C.c_uint32),
        ("enforce_expiry_x", C.c_uint32), ("canon_takes_verified_signature", C.c_uint32), ("canon_ignores_l", C.c_uint32),
        ("i_must_be_subdomain", C.c_uint32), ("b_removes_own_span_only", C.c_uint32), ("sha_mapping", C.c_uint32),
        ("now_unix", C.c_uint64), ("reserved", C.c_uint64 * 4),
    ]


assert C.sizeof(zke_options) == 104


def strict_mask(**flags) -> int:
    """ZKE_STRICT_* mask of the named strictness flags (what the oracle's zko_verify_batch_strict takes)."""
    assert set(flags) <= set(STRICT_FLAGS), flags
    return sum(1 << k for k, name in enumerate(STRICT_FLAGS) if flags.get(name))


class zke_timings(C.Structure):
    _fields_ = [(k, C.c_float) for k in (
        "front_end_us", "hash_modexp_us", "ed_verdict_us", "regex_prep_us", "dfa_us", "total_us", "h2d_us", "d2h_us")]


# ---- the reference's input structs (core/src/structs.rs) ------------------------------
@dataclass
class PublicKey:                       # structs.rs:8-11
    key: bytes
    key_type: str = "rsa"


@dataclass
class ExternalInput:                   # structs.rs:40-44
    name: str
    value: Optional[str]
    max_length: int = 0


@dataclass
class Email:                           # structs.rs:49-54
    from_domain: str
    raw_email: bytes
    public_key: PublicKey
    external_inputs: List[ExternalInput] = field(default_factory=list)


@dataclass
class DFA:                             # structs.rs:16-19
    fwd: bytes
    bwd: bytes


@dataclass
class CompiledRegex:                   # structs.rs:24-27
    verify_re: DFA
    captures: Optional[List[str]] = None


@dataclass
class RegexInfo:                       # structs.rs:32-35
    header_parts: Optional[List[CompiledRegex]] = None
    body_parts: Optional[List[CompiledRegex]] = None


@dataclass
class EmailWithRegex:                  # structs.rs:59-62
    email: Email
    regex_info: RegexInfo


@dataclass
class EmailVerifierOutput:             # structs.rs:65-69
    from_domain_hash: bytes
    public_key_hash: bytes
    external_inputs: List[str]


@dataclass
class EmailWithRegexVerifierOutput:    # structs.rs:72-75
    email: EmailVerifierOutput
    regex_matches: List[str]


def _csr(chunks: Sequence[bytes]):
    off = np.zeros(len(chunks) + 1, dtype=np.uint64)
    if len(chunks):
        off[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    blob = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy() if len(chunks) else np.zeros(0, np.uint8)
    if blob.size == 0:
        blob = np.zeros(1, np.uint8)  # keep a valid pointer
    return blob, off


def key_type_code(s: str) -> int:
    return {"rsa": KEY_RSA, "ed25519": KEY_ED25519}.get(s, KEY_OTHER)


class PackedBatch:
    """Host-side struct-of-arrays image of a list of Email (+ optional shared part ids and
    per-email captures).  Keeps the numpy buffers alive and exposes a ``zke_batch``."""

    def __init__(self, emails: Sequence[Email], header_part_ids: Sequence[int] = (),
                 body_part_ids: Sequence[int] = (), captures: Optional[Sequence[Sequence[Sequence[str]]]] = None,
                 with_regex: bool = False):
        self.n = len(emails)
        self.raw_blob, self.raw_off = _csr([e.raw_email for e in emails])
        self.domain_blob, self.domain_off = _csr([e.from_domain.encode("utf-8") for e in emails])
        self.key_blob, self.key_off = _csr([e.public_key.key for e in emails])
        self.key_type = np.array([key_type_code(e.public_key.key_type) for e in emails] or [0], dtype=np.uint8)
        self.ext_null = np.array(
            [1 if any(x.value is None for x in e.external_inputs) else 0 for e in emails] or [0], dtype=np.uint8)
        self.hdr_ids = np.array(list(header_part_ids) or [0], dtype=np.uint32)
        self.body_ids = np.array(list(body_part_ids) or [0], dtype=np.uint32)
        self.nh, self.nb = len(header_part_ids), len(body_part_ids)
        P = self.nh + self.nb
        self.P = P
        self.with_regex = bool(with_regex)
        strs: List[bytes] = []
        cap_off = [0]
        if P and captures is not None:
            assert len(captures) == self.n
            for per_email in captures:
                assert len(per_email) == P
                for part_caps in per_email:
                    strs.extend(s.encode("utf-8") if isinstance(s, str) else s for s in (part_caps or []))
                    cap_off.append(len(strs))
        elif P:
            cap_off = [0] * (self.n * P + 1)
        self.cap_off = np.array(cap_off, dtype=np.uint32)
        self.cap_blob, str_off = _csr(strs)
        self.cap_str_off = str_off.astype(np.uint32)
        self.has_caps = bool(P)
        self.c = self._make()

    def _make(self) -> zke_batch:
        b = zke_batch()
        b.n = self.n
        b.raw_blob = self.raw_blob.ctypes.data
        b.raw_off = self.raw_off.ctypes.data
        b.domain_blob = self.domain_blob.ctypes.data
        b.domain_off = self.domain_off.ctypes.data
        b.key_blob = self.key_blob.ctypes.data
        b.key_off = self.key_off.ctypes.data
        b.key_type = self.key_type.ctypes.data
        b.ext_null = self.ext_null.ctypes.data
        b.with_regex = 1 if self.with_regex else 0
        b.n_header_parts = self.nh
        b.n_body_parts = self.nb
        b.header_part_ids = self.hdr_ids.ctypes.data
        b.body_part_ids = self.body_ids.ctypes.data
        b.cap_off = self.cap_off.ctypes.data if self.has_caps else None
        b.cap_str_off = self.cap_str_off.ctypes.data
        b.cap_blob = self.cap_blob.ctypes.data
        return b


class DebugBuffers:
    """Optional intermediates (zke_debug_out): canonical header preimage, canonical body,
    QP-cleaned body, recovered EM."""

    def __init__(self, n: int, hdr_stride: int, body_stride: int, em_stride: int = 512):
        self.n = n
        self.canon_header = np.zeros((max(n, 1), hdr_stride), np.uint8)
        self.canon_body = np.zeros((max(n, 1), body_stride), np.uint8)
        self.clean_body = np.zeros((max(n, 1), body_stride), np.uint8)
        self.em = np.zeros((max(n, 1), em_stride), np.uint8)
        self.full_len = np.zeros(max(n, 1), np.uint32)
        self.rsa_route = np.zeros(max(n, 1), np.uint32)
        d = zke_debug_out()
        d.canon_header = self.canon_header.ctypes.data; d.canon_header_stride = hdr_stride
        d.canon_body = self.canon_body.ctypes.data; d.canon_body_stride = body_stride
        d.clean_body = self.clean_body.ctypes.data; d.clean_body_stride = body_stride
        d.em = self.em.ctypes.data; d.em_stride = em_stride
        d.canon_body_full_len = self.full_len.ctypes.data
        d.rsa_route = self.rsa_route.ctypes.data
        self.c = d
