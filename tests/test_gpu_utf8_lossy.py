"""GPU: String::from_utf8_lossy on the device (csrc/utf8_lossy.hip.h) through zke_utf8_lossy_batch — every output byte, offset and
flag against Python's decode("utf-8", "replace") (tests/utf8_lossy_cases.py says why that is the reference): the exhaustive sets of
the CPU tier, the lengths around the kernel's 64-byte step, a four-byte sequence across every lane and step edge, strings that end
in a truncated lead in front of a string that starts with a continuation byte, a short output blob, stale bytes of an earlier batch."""
import ctypes as C

import numpy as np
import pytest

import utf8_lossy_cases as U
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

GUARD = 64
E_ARG, E_NOMEM = -1, -3


def call(engine, strings, cap=None, lead=b""):
    """One zke_utf8_lossy_batch: (rc, out_off, out bytes with GUARD bytes of 0xAA behind `cap`, flags, need).  `lead`: bytes in front
    of the first string that belong to nobody (off[0] != 0)."""
    n = len(strings)
    blob, off = A._csr(([lead] if lead else []) + list(strings))
    if lead:
        off = off[1:].copy()
    total = int(off[n] - off[0]) if n else 0
    if cap is None:
        cap = 3 * total
    out_off = np.full(n + 1, 0xAAAAAAAA, np.uint32)
    out = np.full(cap + GUARD, 0xAA, np.uint8)
    flags = np.full(max(n, 1), 0xAA, np.uint8)
    need = C.c_size_t(2 ** 40)
    rcode = engine.lib.zke_utf8_lossy_batch(engine.h, blob.ctypes.data, off.ctypes.data, n, out_off.ctypes.data, out.ctypes.data if cap else None,
                                            cap, C.byref(need), flags.ctypes.data)
    return rcode, out_off, out, flags, need.value, cap


def check(engine, strings, lead=b""):
    ref = [U.reference(s) for s in strings]
    want_off = np.zeros(len(strings) + 1, np.uint64)
    want_off[1:] = np.cumsum([len(r) for r in ref])
    rcode, out_off, out, flags, need, cap = call(engine, strings, lead=lead)
    assert rcode == 0, engine.lib.zke_last_error(None)
    assert need == int(want_off[-1])
    assert (out_off == want_off).all()
    assert out[:need].tobytes() == b"".join(ref)
    assert (out[need:] == 0xAA).all(), "a byte behind the repaired strings was written"
    assert (flags[:len(strings)] == np.array([r != s for r, s in zip(ref, strings)], np.uint8)).all()
    return ref


def test_pins_and_exhaustive_short(engine):
    check(engine, [p[0] for p in U.pins()] + U.exhaustive_short())
    got, changed = engine.utf8_lossy([U.UNICODE_EXAMPLE, b"", b"plain", b"\xf0\x9f\x98\x80"])
    assert got == [U.pins()[0][1], b"", b"plain", b"\xf0\x9f\x98\x80"] and changed.tolist() == [True, False, False, False]
    assert engine.utf8_lossy([])[0] == []


def test_exhaustive_alphabet_and_random(engine):
    check(engine, U.exhaustive_alphabet() + U.random_strings())


def test_lengths_around_the_step(engine):
    strings = []
    for n in (0, 1, 63, 64, 65, 4095, 4096):
        strings += [b"\xff" * n, b"\x80" * n, ("€" * n).encode()[:3 * (n // 3)] + b"a" * (n % 3)]
    ref = check(engine, strings, lead=b"\xe2\x82")       # (the bytes in front of off[0] would complete nothing, and are never read)
    assert len(ref[-3]) == 3 * 4096 and ref[-1] == strings[-1]


def test_sequence_across_every_lane_and_step_edge(engine):
    face = b"\xf0\x9f\x98\x80"
    strings = []
    for k in (0, 1):
        for r in range(64):
            at = 64 * k + r
            strings.append(b"a" * at + face + b"b" * 5)          # whole
            strings.append(b"a" * at + face[:3] + b"b" * 5)      # its last byte removed: one U+FFFD
            strings.append(b"a" * at + face)                     # whole, the string ends with it
            strings.append(b"a" * at + face[:3])                 # cut short by the end of the string
    check(engine, strings)


def test_repair_does_not_read_across_strings(engine):
    strings = []
    for lead, tail in ((b"\xc3", b"\xa9"), (b"\xe2", b"\x82\xac"), (b"\xe2\x82", b"\xac"), (b"\xf0", b"\x9f\x98\x80"), (b"\xf0\x9f", b"\x98\x80"),
                       (b"\xf0\x9f\x98", b"\x80")):
        for pad in (0, 1, 61, 62, 63, 64):
            strings += [b"x" * pad + lead, tail + b"y" * pad]
    ref = check(engine, strings)
    assert ref[0] == U.FFFD and ref[1] == U.FFFD


def test_short_blob_reports_the_need_and_writes_nothing_beyond(engine):
    strings = U.random_strings(300, seed=7) + [b"\xff" * 1000]
    ref = b"".join(U.reference(s) for s in strings)
    for cap in (0, 1, len(ref) // 2, len(ref) - 1):
        rcode, out_off, out, flags, need, _ = call(engine, strings, cap=cap)
        assert rcode == E_NOMEM and need == len(ref)
        assert (out[cap:] == 0xAA).all(), "a byte beyond the capacity was written"
        assert int(out_off[-1]) == len(ref) and out_off[0] == 0
        assert (flags[:len(strings)] <= 1).all()
    rcode, out_off, out, flags, need, _ = call(engine, strings, cap=len(ref))
    assert rcode == 0 and need == len(ref) and out[:need].tobytes() == ref and (out[need:] == 0xAA).all()


def test_stale_bytes_of_an_earlier_batch():
    eng = z.Engine(slots=1)                                       # one slot: both batches run in the same buffers
    long = [b"\xff" * 4096] * 8 + U.random_strings(200, seed=11)
    short = [b"ok", b"\x80", b"", b"caf\xc3\xa9", b"\xe2\x82"]
    for batch in (long, short, long[:3], short):
        check(eng, batch)


def test_argument_refusals(engine):
    off = np.array([0, 4, 2], np.uint64)
    blob = np.zeros(8, np.uint8)
    out_off, flags, need = np.zeros(3, np.uint32), np.zeros(2, np.uint8), C.c_size_t(0)
    args = lambda o, n=2: (engine.h, blob.ctypes.data, o.ctypes.data, n, out_off.ctypes.data, blob.ctypes.data, 8, C.byref(need), flags.ctypes.data)
    assert engine.lib.zke_utf8_lossy_batch(*args(off)) == E_ARG                     # offsets decrease
    big = np.array([0, A.UTF8_LOSSY_MAX_BYTES + 1], np.uint64)
    assert engine.lib.zke_utf8_lossy_batch(*args(big, 1)) == E_ARG                  # refused before a byte is read
    assert engine.lib.zke_utf8_lossy_batch(engine.h, blob.ctypes.data, off.ctypes.data, 2, None, blob.ctypes.data, 8, C.byref(need), flags.ctypes.data) == E_ARG
    assert engine.lib.zke_utf8_lossy_batch(*args(off, 0)) == 0 and out_off[0] == 0 and need.value == 0
