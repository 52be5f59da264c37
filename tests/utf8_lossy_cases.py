"""Case lists for the UTF-8 repair (csrc/utf8_lossy.hip.h), shared by the CPU tier (tests/test_utf8_lossy_sanitizers.py) and the GPU
tier (tests/test_gpu_utf8_lossy.py).  The reference is Python's decode("utf-8", "replace"): one U+FFFD per maximal ill-formed prefix,
the rule of Rust's String::from_utf8_lossy (the pins below say so for the cases where other decoders differ)."""
import itertools

import numpy as np

# every byte value at which Table 3-7 changes its mind
ALPHABET = bytes([0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1,
                  0xF3, 0xF4, 0xF5, 0xFF])
UNICODE_EXAMPLE = bytes.fromhex("61 F1 80 80 E1 80 C2 62 80 63 80 BF 64")
FFFD = b"\xef\xbf\xbd"


def reference(s: bytes) -> bytes:
    return s.decode("utf-8", "replace").encode()


def pins():
    """(input, expected) pairs that do not come from Python: the Unicode standard's example and the issue's counts."""
    return [(UNICODE_EXAMPLE, b"a" + FFFD * 3 + b"b" + FFFD + b"c" + FFFD * 2 + b"d"),
            (bytes.fromhex("F09080"), FFFD), (bytes.fromhex("EDA080"), FFFD * 3), (bytes.fromhex("F4908080"), FFFD * 4),
            (bytes.fromhex("C080"), FFFD * 2)]


def exhaustive_short():
    """Every 1- and 2-byte string (and the empty one)."""
    return [b""] + [bytes([a]) for a in range(256)] + [bytes([a, b]) for a in range(256) for b in range(256)]


def exhaustive_alphabet():
    """Every 3- and 4-byte string over ALPHABET: 24^3 + 24^4 = 345 600."""
    return [bytes(t) for k in (3, 4) for t in itertools.product(ALPHABET, repeat=k)]


def random_strings(count=2000, seed=20260101, max_len=200):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(ALPHABET, np.uint8)
    return [alpha[rng.integers(0, len(alpha), int(rng.integers(0, max_len + 1)))].tobytes() for _ in range(count)]
