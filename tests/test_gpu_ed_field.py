"""GPU (-m gpu): the field, scalar, hash and point routines of csrc/ed25519.hip.h, each called directly by the probe program
(tests/cpp/ed_probe.hip) on the cases of tests/ed_field_cases.py — the operands at which a lazily reduced field element wraps
or borrows a second time, scalars around L, every padded message length, and identity / torsion / doubling-by-addition
operands of the complete point formulas, in reduced and unreduced coordinates.  Expectations are Python integers.

The probe runs ONCE per session, as a child process; the tests below assert on slices of its one result file.  After a
non-zero exit or a timeout it is not run again: every test reports that first failure."""
import subprocess

import pytest

import ed_field_cases as F
from zkemail_rs_amd import build

pytestmark = pytest.mark.gpu

_RUN = {}


def results(tmp_path_factory):
    """-> (cases, rows); the probe's single run, remembered whether it worked or not"""
    if not _RUN:
        try:
            cases = F.build_cases()
            exe = build.build_ed_probe()
            d = tmp_path_factory.mktemp("ed_probe")
            (d / "tape.bin").write_bytes(F.pack_tape(cases))
            r = subprocess.run([exe, str(d / "tape.bin"), str(d / "results.bin")], capture_output=True, text=True, timeout=120)
            if r.returncode != 0:
                raise RuntimeError("ed_probe exited with %d: %s" % (r.returncode, r.stderr.strip()[-400:]))
            _RUN["ok"] = (cases, F.unpack_results((d / "results.bin").read_bytes(), len(cases)))
        except Exception as e:                          # a timeout included: nothing more is started on the GPU
            _RUN["error"] = "%s: %s" % (type(e).__name__, e)
    if "error" in _RUN:
        pytest.fail("the probe's one run failed: " + _RUN["error"], pytrace=False)
    return _RUN["ok"]


@pytest.fixture
def probe(tmp_path_factory):
    return results(tmp_path_factory)


def assert_ops(probe, ops):
    cases, rows = probe
    n, bad = 0, []
    for c, row in zip(cases, rows):
        if c.op in ops:
            n += 1
            msg = F.check(c, row)
            if msg:
                bad.append(msg)
    assert n >= len(ops)
    assert {c.op for c in cases if c.op in ops} == set(ops)
    assert not bad, "%d of %d cases wrong; first:\n%s" % (len(bad), n, "\n".join(bad[:5]))


def test_field_binary_ops(probe):
    assert_ops(probe, ("fe_add", "fe_sub", "fe_mul", "fe_mul_i"))


def test_field_squarings(probe):
    assert_ops(probe, ("fe_sq", "fe_sq_i"))


def test_field_unary_ops_and_predicates(probe):
    assert_ops(probe, ("fe_canon", "fe_is_zero", "fe_eq", "fe_is_neg", "fe_neg", "fe_from_bytes"))


def test_field_inversion_and_power_chain(probe):
    assert_ops(probe, ("fe_invert", "fe_pow22523"))


def test_scalars(probe):
    assert_ops(probe, ("sc_lt_L", "sc_reduce512"))


def test_sha512_every_message_length(probe):
    assert_ops(probe, ("sha512_ram",))


def test_decompress_compress_and_order(probe):
    assert_ops(probe, ("ge_decompress", "ge_compress", "ge_is_small_order"))


def test_point_formulas_one_lane(probe):
    assert_ops(probe, ("ge_add", "ge_dbl", "ge_add_cached"))


def test_point_formulas_quad(probe):
    assert_ops(probe, ("q_table", "q_dbl", "q_add"))
