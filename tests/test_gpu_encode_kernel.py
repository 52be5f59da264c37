"""GPU: encode_outputs_kernel (csrc/encode.hip.h) and the digest launch behind it through zke_encode_outputs, over synthetic
records — random hashes, statuses chosen here — against zkemail_rs_amd.abi_encode.abi_encode and hashlib.sha256, exactly: batch
sizes around the wave count, kinds mixed within a batch, string lengths at every edge of the 16-byte chunk, the 32-byte word and
the 1 024-byte round, lists around one pass of the wave (64 strings) and beyond two, every source residue mod 16 in both blobs,
non-ASCII bytes, non-OK e-mails first and last with every non-OK status, and padding written over stale bytes.

One engine with ONE slot: every batch lands in the same output buffer, which is never cleared.  For every batch the same checks
(check_batch): each encoded place whole, every len / off / kind / digest, len 0 and a zero digest for the non-OK e-mails, whose
places in the caller's bytes stay untouched, and the guard region behind bytes_need."""
import numpy as np
import pytest

import encode_cases as EC
import zkemail_rs_amd as z
from zkemail_rs_amd import _abi as A

pytestmark = pytest.mark.gpu

GUARD, FILL = 96, 0xA5


@pytest.fixture(scope="module")
def eng():
    e = z.Engine(slots=1)
    yield e
    e.close()


def check_batch(eng, outputs, statuses=None, what=""):
    want, total = EC.expected(outputs, statuses)
    tb = A.EncodeTables(outputs, statuses)
    enc = eng.encode_outputs(tb, guard=GUARD, fill=FILL)
    assert (enc.c.infos_need, enc.c.bytes_need) == (len(outputs), total), what
    blob = enc.bytes
    assert (blob[total:] == FILL).all() and len(blob) == max(total + GUARD, 1), (what, "guard region written")
    for i, (off, ln, kind, digest, ref) in enumerate(want):
        f = enc.infos[i]
        assert (int(f["off"]), int(f["len"]), int(f["kind"])) == (off, ln, kind), (what, i)
        assert f["digest"].tobytes() == digest, (what, i, "digest")
        if ln:
            got = blob[off:off + ln].tobytes()
            if got != ref:
                bad = next(k for k in range(ln) if got[k] != ref[k])
                raise AssertionError((what, i, "first differing byte", bad, got[bad & ~31:(bad & ~31) + 32].hex(), ref[bad & ~31:(bad & ~31) + 32].hex()))
        else:
            planned = len(EC.ref_bytes(outputs[i]))
            assert (blob[off:off + planned] == FILL).all(), (what, i, "the place of an e-mail that is not encoded was written")
    return enc


@pytest.mark.parametrize("residue", range(16))
def test_string_lengths_at_every_source_residue(eng, residue):
    """A filler string of `residue` bytes in front of both blobs moves every string's source to another residue mod 16 (the lengths
    themselves add the other shifts); every length of the list appears as an external input and as a match, in both kinds."""
    rng = np.random.default_rng(100 + residue)
    outs = [EC.output(rng, [EC.text(residue)], [EC.text(residue, 1)])]
    for k, n in enumerate(EC.STRING_LENS):
        outs.append(EC.output(rng, [EC.text(n, k), EC.text(1)], [EC.text(n, k + 1)] if k % 2 else None))
        outs.append(EC.output(rng, [EC.text(1, k)], [EC.text(1), EC.text(n, k + 2)] if k % 2 == 0 else None))
    check_batch(eng, outs, what=f"residue {residue}")


def test_list_sizes_around_one_pass_of_the_wave(eng):
    """0, 1, 2, 63, 64, 65 and 130 strings in a list: the scan's carry from pass to pass, in the external inputs and in the matches."""
    rng = np.random.default_rng(5)
    small = [0, 1, 15, 16, 17, 31, 32, 33]
    outs = []
    for k, size in enumerate(EC.LIST_SIZES):
        other = EC.LIST_SIZES[len(EC.LIST_SIZES) - 1 - k]
        outs.append(EC.output(rng, [EC.text(small[(j + k) % 8], j) for j in range(size)], [EC.text(small[(j * 3 + k) % 8], j + 1) for j in range(other)]))
        outs.append(EC.output(rng, [EC.text(small[(j * 5 + k) % 8], j) for j in range(size)], None))
    outs.append(EC.output(rng, [EC.text(70 + j % 60, j) for j in range(130)], [EC.text(1030 + j, j) for j in range(66)]))
    check_batch(eng, outs, what="list sizes")


@pytest.mark.parametrize("n", EC.BATCH_SIZES)
def test_batch_sizes_with_non_ok_first_and_last(eng, n):
    """Kinds mixed, the first and the last e-mail not ZKE_OK, every non-OK status at least once over the batches (each batch takes
    its statuses from a rotating list, n = 1 the whole of it in turn)."""
    outs = EC.random_outputs(900 + n, n)
    st = [A.ZKE_OK] * n
    st[0] = EC.NON_OK[n % len(EC.NON_OK)]
    st[n - 1] = EC.NON_OK[(n + 1) % len(EC.NON_OK)]
    for k in range(3, n - 1, 7):
        st[k] = EC.NON_OK[k % len(EC.NON_OK)]
    check_batch(eng, outs, st, what=f"n={n}")
    if n == 1:
        for s in EC.NON_OK + [A.ZKE_OK]:
            check_batch(eng, outs, [s], what=f"n=1 status {s}")


def test_every_non_ok_status_is_not_encoded(eng):
    outs = EC.random_outputs(31, len(EC.NON_OK) + 2)
    check_batch(eng, outs, [A.ZKE_OK] + EC.NON_OK + [A.ZKE_OK], what="statuses")


def test_padding_is_written_over_stale_bytes(eng):
    """A batch of 4 097-byte strings (never a zero byte), then a batch of 1-byte strings at the same places of the slot's buffer: the
    31 bytes behind each string and every head word's 24 leading bytes must be zeros the kernel wrote."""
    rng = np.random.default_rng(77)
    big = [EC.output(rng, [EC.text(4097, k), EC.text(4097, k + 1)], [EC.text(4097, k + 2)] if k % 2 else None) for k in range(6)]
    check_batch(eng, big, what="stale: long strings")
    tiny = [EC.output(rng, [EC.text(1, k)] * 40, [EC.text(1, k + 1)] * 30 if k % 2 else None) for k in range(6)]
    check_batch(eng, tiny, what="stale: short strings")


def test_sizes_are_exact_and_checked_before_anything_runs(eng):
    """bytes_need / infos_need are the plan's, set by a call that fails with ZKE_E_NOMEM at once; one byte more than needed is fine."""
    import ctypes as C
    outs = EC.random_outputs(12, 9)
    want, total = EC.expected(outs)
    with pytest.raises(z.EngineError, match=r"\(-3\)"):
        eng.encode_outputs(outs, bytes_cap=total - 1)
    tb = A.EncodeTables(outs)
    short = A.EncodedBuffers(len(outs), total)
    short.c.infos_cap = len(outs) - 1
    rc = eng.lib.zke_encode_outputs(eng.h, tb.records.ctypes.data, tb.n, tb.kinds.ctypes.data, tb.ext.off.ctypes.data, tb.ext.str_off.ctypes.data,
                                    tb.ext.blob.ctypes.data, tb.matches.off.ctypes.data, tb.matches.str_off.ctypes.data, tb.matches.blob.ctypes.data,
                                    C.byref(short.c))
    assert rc == -3 and (short.c.infos_need, short.c.bytes_need) == (len(outs), total) and not short.bytes.any()
    enc = eng.encode_outputs(outs, bytes_cap=total + 1)
    assert [e for e, _ in enc.result()] == [w[4] for w in want]
