"""CPU (-m "not gpu"): the index-map model of tests/qp_map_model.py — pinned to the oracle's remove_qp, its 64-byte-step ballot
formulations (the compaction of qp_index_kernel, the map-free lookup of capture_origin_kernel) against the sequential reference
function, the properties of the origin flags — and the argument checks of the three entry points, which come before any GPU work."""
import ctypes as C
import random

import numpy as np
import pytest

import qp_map_model as Q
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import engine

E_ARG, E_NOMEM = -1, -3


@pytest.fixture(scope="module")
def bodies():
    return Q.cases()


def test_model_cleaned_equals_the_oracle(oracle, bodies):
    for b in bodies:
        cleaned, im, kept = Q.remove_qp(b)
        assert cleaned == oracle.remove_qp(b), b[:80]
        assert len(im) == len(b) and all(x == Q.NO_INDEX for x in im[kept:]) and cleaned[kept:] == bytes(len(b) - kept)
        assert bytes(b[x] for x in im[:kept]) == cleaned[:kept] and im[:kept] == sorted(set(im[:kept]))


@pytest.mark.parametrize("step", [64, 4, 3])       # 64: the wave; 4 and 3: every short body crosses many step boundaries
def test_ballot_formulations_equal_the_sequential_model(bodies, step):
    rng = random.Random(step)
    for b in bodies:
        if step != 64 and len(b) > 200:
            continue
        ref = Q.remove_qp(b)
        assert Q.ballot_remove_qp(b, step) == ref, (step, b[:80])
        if len(b) <= 4096:
            qs = sorted({0, len(b), max(len(b) - 1, 0), ref[2], max(ref[2] - 1, 0)} | {rng.randrange(len(b) + 1) for _ in range(6)})
            assert Q.ballot_lookup(b, qs, step) == [ref[1][q] if q < len(b) else Q.NO_INDEX for q in qs], (step, b[:80])


def test_origin_flag_properties():
    """No flag => body[start:end] is the capture's bytes; SPLIT <=> a "=\\r\\n" begins inside [start, end)."""
    rng = random.Random(7)
    seen = {0: 0, Q.ORGF_SPLIT: 0, Q.ORGF_PADDING: 0}
    for b in Q.seeded_bodies(3000, 11):
        n = len(b)
        if not n:
            continue
        cleaned, im, kept = Q.remove_qp(b)
        for _ in range(4):
            s = rng.randrange(n + 1)
            e = rng.randrange(s, n + 1)
            start, end, flags = Q.origin(im, n, s, e)
            seen[flags] += 1
            if flags == Q.ORGF_PADDING:
                assert e > kept or s >= kept
                continue
            # ('=' is neither '\r' nor '\n': occurrences of "=\r\n" cannot overlap, each is a break the filter removes; and one that
            # begins inside [start, end) ends inside it, because end - 1 is a kept byte)
            breaks_inside = sum(b[k:k + 3] == Q.SOFT for k in range(start, end))
            assert (flags == Q.ORGF_SPLIT) == (breaks_inside > 0), (b, s, e)
            assert end - start == (e - s) + 3 * breaks_inside, (b, s, e)
            if flags == 0:
                assert b[start:end] == cleaned[s:e], (b, s, e)
    assert all(v > 100 for v in seen.values()), seen
    assert Q.origin([], 0, Q.NO_INDEX, Q.NO_INDEX) == (Q.NO_INDEX, Q.NO_INDEX, 0)


def test_new_entry_points_check_their_arguments_first():
    """zke_qp_clean_batch, zke_extract_captures_mapped[_async]: null and too-small arguments are refused before anything touches a
    GPU; the *_need fields are written (the zke_capture_out convention)."""
    lib = engine.load_library()
    fake = C.c_void_p(0x1000)                     # an "engine" that is never dereferenced: every check below fails in front of it
    off = np.array([0, 4, 2], np.uint64)
    blob = np.zeros(8, np.uint8)
    out8, out32, ln = np.zeros(8, np.uint8), np.zeros(8, np.uint32), np.zeros(2, np.uint32)
    assert lib.zke_qp_clean_batch(None, blob.ctypes.data, off.ctypes.data, 2, out8.ctypes.data, out32.ctypes.data, ln.ctypes.data) == E_ARG
    assert lib.zke_qp_clean_batch(fake, blob.ctypes.data, off.ctypes.data, 2, None, None, None) == E_ARG
    assert lib.zke_qp_clean_batch(fake, blob.ctypes.data, None, 2, out8.ctypes.data, None, None) == E_ARG
    assert lib.zke_qp_clean_batch(fake, blob.ctypes.data, off.ctypes.data, 2, out8.ctypes.data, None, None) == E_ARG       # decreasing offsets
    assert b"non-decreasing" in lib.zke_last_error(None)
    big = np.array([0, 0xFFFFFFFF], np.uint64)
    assert lib.zke_qp_clean_batch(fake, blob.ctypes.data, big.ctypes.data, 1, None, None, ln.ctypes.data) == E_ARG        # a body of 2^32 - 1 bytes
    ok = np.array([3, 3, 7], np.uint64)
    assert lib.zke_qp_clean_batch(fake, None, ok.ctypes.data, 2, out8.ctypes.data, None, None) == E_ARG                   # bytes without a blob
    assert lib.zke_qp_clean_batch(fake, None, None, 0, out8.ctypes.data, None, None) == 0                                 # n == 0: nothing touched
    assert not out8.any()

    refs = A.EmailRefs([A.Email("a.com", b"x", A.PublicKey(b"k"))] * 3)
    g = np.array([0, 1], np.uint32)
    part = (A.zke_capture_part * 1)()
    part[0].dfa_id, part[0].prog_id, part[0].n_groups, part[0].groups = 0, 0, 2, g.ctypes.data
    res = np.zeros(3, dtype=A.RESULT_DTYPE)
    t = C.c_uint64()

    def caps_of(n, P, G):
        bufs = [np.zeros(n * G * 2, np.uint32), np.zeros(n * G, np.uint8), np.zeros(n * P + 1, np.uint32), np.zeros(n * G + 1, np.uint32), np.zeros(64, np.uint8)]
        o = A.zke_capture_out()
        o.spans, o.spans_cap, o.flags, o.flags_cap = bufs[0].ctypes.data, n * G * 2, bufs[1].ctypes.data, n * G
        o.cap_off, o.cap_off_cap, o.cap_str_off, o.cap_str_off_cap = bufs[2].ctypes.data, n * P + 1, bufs[3].ctypes.data, n * G + 1
        o.cap_blob, o.cap_blob_cap = bufs[4].ctypes.data, 64
        return o, bufs

    def org_of(spans_cap, flags_cap, null=False):
        bufs = [np.zeros(max(spans_cap, 1), np.uint32), np.zeros(max(flags_cap, 1), np.uint8)]
        o = A.zke_capture_origin()
        o.spans, o.spans_cap, o.flags, o.flags_cap = (None if null else bufs[0].ctypes.data), spans_cap, bufs[1].ctypes.data, flags_cap
        o.spans_need = o.flags_need = 77
        return o, bufs

    caps, keep1 = caps_of(3, 1, 2)
    org, keep2 = org_of(12, 6)
    sync = lambda e, c, o: lib.zke_extract_captures_mapped(e, refs.arr, 3, None, 0, part, 1, res.ctypes.data, c, o)
    asyn = lambda e, c, o, tk=C.byref(t): lib.zke_extract_captures_mapped_async(e, refs.arr, 3, None, 0, part, 1, res.ctypes.data, c, o, tk)
    for call in (sync, asyn):
        assert call(None, C.byref(caps), C.byref(org)) == E_ARG
        assert call(fake, None, C.byref(org)) == E_ARG
        assert call(fake, C.byref(caps), None) == E_ARG
        small, keep3 = org_of(11, 6)
        assert call(fake, C.byref(caps), C.byref(small)) == E_NOMEM and (small.spans_need, small.flags_need) == (12, 6)
        small, keep3 = org_of(12, 5)
        assert call(fake, C.byref(caps), C.byref(small)) == E_NOMEM and (small.spans_need, small.flags_need) == (12, 6)
        nul, keep3 = org_of(12, 6, null=True)
        assert call(fake, C.byref(caps), C.byref(nul)) == E_ARG and (nul.spans_need, nul.flags_need) == (12, 6)
        tiny, keep4 = caps_of(3, 1, 1)                                    # caps is checked in front of org
        assert call(fake, C.byref(tiny), C.byref(org)) == E_NOMEM and tiny.spans_need == 12
    assert asyn(fake, C.byref(caps), C.byref(org), None) == E_ARG         # null ticket
    assert lib.zke_extract_captures_mapped(fake, refs.arr, 3, None, 1, part, 1, res.ctypes.data, C.byref(caps), C.byref(org)) == E_ARG   # parts without a list
    assert lib.zke_abi_version() == 3
