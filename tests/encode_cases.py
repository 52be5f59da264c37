"""Inputs and expectations of the output-encoding tests (zke_encode_outputs, zke_verify_emails_encoded): verifier outputs with
strings of chosen BYTE lengths (non-ASCII included), and the reference for every byte — zkemail_rs_amd.abi_encode.abi_encode, pinned
by the hand-laid vector of tests/test_abi_encode.py, with hashlib.sha256 for the digests.  Places are the prefix sum of the
reference's own lengths: a non-OK e-mail keeps its place and leaves it unused."""
import hashlib
from typing import List, Optional, Sequence

import numpy as np

from zkemail_rs_amd import _abi as A
from zkemail_rs_amd.abi_encode import abi_encode

NON_OK = list(range(1, 12))                    # ZKE_PARSE_FAIL .. ZKE_BODY_DECODE_FAIL
STRING_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4097]
LIST_SIZES = [0, 1, 2, 63, 64, 65, 130]
BATCH_SIZES = [1, 63, 64, 65, 130]
ZERO_DIGEST = b"\0" * 32


def text(nbytes: int, salt: int = 0) -> str:
    """A string of exactly `nbytes` UTF-8 bytes that is not ASCII wherever two bytes fit: 1-, 2-, 3- and 4-byte characters in turn."""
    alphabet = ["a", "é", "漢", "\U0001f511", "Z", "ß", "7", "€"]
    out, used, k = [], 0, salt
    while used < nbytes:
        ch = alphabet[k % len(alphabet)]
        k += 1
        w = len(ch.encode("utf-8"))
        if used + w > nbytes:
            ch, w = chr(ord("b") + (k % 20)), 1
        out.append(ch)
        used += w
    s = "".join(out)
    assert len(s.encode("utf-8")) == nbytes
    return s


def email_output(rng, ext: Sequence[str]) -> A.EmailVerifierOutput:
    return A.EmailVerifierOutput(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), list(ext))


def output(rng, ext: Sequence[str], matches: Optional[Sequence[str]] = None):
    """kind 0 (matches None) or kind 1 (a list, possibly empty) with random hashes."""
    e = email_output(rng, ext)
    return e if matches is None else A.EmailWithRegexVerifierOutput(e, list(matches))


def ref_bytes(o) -> bytes:
    return abi_encode(o.email, o.regex_matches) if isinstance(o, A.EmailWithRegexVerifierOutput) else abi_encode(o)


def expected(outputs: Sequence, statuses: Optional[Sequence[int]] = None):
    """Per e-mail (off, len, kind, digest, bytes) as the infos and the blob must show them, and the blob's size."""
    out, off = [], 0
    for i, o in enumerate(outputs):
        ref = ref_bytes(o)
        kind = A.ENC_KIND_WITH_REGEX if isinstance(o, A.EmailWithRegexVerifierOutput) else A.ENC_KIND_EMAIL
        ok = statuses is None or statuses[i] == A.ZKE_OK
        out.append((off, len(ref) if ok else 0, kind, hashlib.sha256(ref).digest() if ok else ZERO_DIGEST, ref if ok else b""))
        off += len(ref)
    return out, off


def random_outputs(seed: int, n: int, max_strings: int = 4, max_len: int = 70) -> List:
    rng = np.random.default_rng(seed)
    outs = []
    for i in range(n):
        ext = [text(int(rng.integers(0, max_len)), int(rng.integers(0, 8))) for _ in range(2 * int(rng.integers(0, max_strings // 2 + 1)))]
        m = None if rng.integers(0, 2) == 0 else [text(int(rng.integers(0, max_len)), i) for _ in range(int(rng.integers(0, max_strings + 1)))]
        outs.append(output(rng, ext, m))
    return outs


def plan_outputs(seed: int = 7) -> List:
    """500 seeded outputs for the plan test: empty lists, empty strings, lengths 0/1/31/32/33/63/64/65 and 130 strings in one list
    are put in by hand in front of the random ones."""
    rng = np.random.default_rng(seed)
    edge = [0, 1, 31, 32, 33, 63, 64, 65]
    outs = [output(rng, []), output(rng, [], []), output(rng, [""], [""]), output(rng, ["", ""], None),
            output(rng, [text(n) for n in edge], [text(n, 3) for n in reversed(edge)]),
            output(rng, [text(n % 40, n) for n in range(130)], None), output(rng, [], [text(n % 7, n) for n in range(130)])]
    outs += [output(rng, [text(n)], [text(n, 1)] if n % 2 else None) for n in edge]
    return outs + random_outputs(seed + 1, 500 - len(outs), max_strings=6, max_len=100)
