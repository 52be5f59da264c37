"""CPU (-m "not gpu"): the case list of the Ed25519 probe (tests/ed_field_cases.py) is not vacuous and its expectations hold
together — every rare class selects a case, the expectations satisfy the identities they should, the tape packs and unpacks —
and the verify-entry edge vectors (ed_vectors.build_edge_vectors) get the same verdicts from the C oracle as from Python."""
import numpy as np
import pytest

import ed25519_ref as ed
import ed_field_cases as F
import ed_vectors

P = ed.P


@pytest.fixture(scope="module")
def cases():
    return F.build_cases()


@pytest.mark.parametrize("name", list(F.CLASSES))
def test_every_rare_class_selects_a_case(cases, name):
    n = sum(1 for c in cases if F.CLASSES[name](c))
    assert n >= F.CLASS_MIN.get(name, 1), "class '%s' selects %d case(s)" % (name, n)


def test_every_op_has_cases_and_pool_pairs_are_complete(cases):
    by_op = {}
    for c in cases:
        by_op.setdefault(c.op, []).append(c)
    assert set(by_op) == set(F.OPS)
    pool = F.field_pool()
    assert len(pool) >= 60 and all(0 <= v < F.M256 for v in pool)
    for op in ("fe_add", "fe_sub", "fe_mul", "fe_mul_i"):
        assert {(a, b) for a in pool for b in pool} <= {c.ins for c in by_op[op]}
    for op in ("fe_sq", "fe_sq_i", "fe_canon", "fe_is_zero", "fe_is_neg", "fe_neg", "fe_from_bytes"):
        assert set(pool) <= {c.ins[0] for c in by_op[op]}
    inv = {c.ins[0] for c in by_op["fe_invert"]}
    assert len(inv) == 16 and {0, 1, P - 1, P + 1, F.M256 - 1} <= inv and inv == {c.ins[0] for c in by_op["fe_pow22523"]}
    assert {c.aux for c in by_op["sha512_ram"]} == set(range(1, 33))
    assert {1 << i for i in range(512)} <= {c.ins[0] for c in by_op["sc_reduce512"]}
    for c in cases:
        assert all(0 <= v < 1 << (32 * w) for v, w in zip(c.ins, F.OPS[c.op][2]))


def test_second_wrap_constructions_hold():
    pairs = F.mul_second_wrap_pairs()
    assert len(pairs) >= 32 and all(F.is_second_wrap(a, b) and 38 <= a * b % (2 * P) <= 75 for a, b in pairs)
    sq = F.sq_second_wrap_operands()
    assert len(sq) >= 50 and all(F.is_second_wrap(a, a) and a * a % (2 * P) < 200 for a in sq)
    rng = np.random.default_rng(5)
    rnd = [F._rand(rng) for _ in range(2000)]
    assert not any(F.is_second_wrap(a, b) for a, b in zip(rnd[::2], rnd[1::2]))     # random operands never get there


def test_field_expectations_are_self_consistent(cases):
    inv = {c.ins[0]: c.exp for c in cases if c.op == "fe_invert"}
    for a, r in inv.items():
        assert a * r % P == (1 if a % P else 0)
    for c in cases:
        if c.op == "fe_pow22523":                      # a^((p-5)/8): its eighth power times a^3 is the inverse
            assert pow(c.exp, 8, P) * pow(c.ins[0], 3, P) % P == inv[c.ins[0]]
        elif c.op in ("fe_mul", "fe_mul_i"):
            F_, _ = F.mul_terms(*c.ins)
            assert F_ % P == c.exp                     # the folded form the classes are stated on is the same residue
        elif c.op == "fe_neg":
            assert (c.exp + c.ins[0]) % P == 0
        elif c.op == "fe_canon":
            assert 0 <= c.exp < P and (c.exp - c.ins[0]) % P == 0


def test_point_expectations_are_on_the_curve_and_agree_with_the_reference(cases):
    for c in cases:
        if c.op in ("ge_add", "ge_add_cached", "q_add"):
            a, b = c.ins[0:4], c.ins[4:8]
            assert F.on_curve(a) and F.on_curve(b) and F.on_curve(c.exp)
            assert F._same_point(c.exp, ed.add(tuple(v % P for v in a), tuple(v % P for v in b)))
            if c.op == "ge_add_cached":
                assert (c.ins[8] - 2 * ed.D * b[3]) % P == 0
        elif c.op in ("ge_dbl", "q_dbl"):
            assert F.on_curve(c.ins) and F.on_curve(c.exp)
            assert F._same_point(c.exp, ed.mul(2, tuple(v % P for v in c.ins)))
        elif c.op == "ge_is_small_order":
            assert F.on_curve(c.ins) and c.exp == int(ed.is_identity(ed.mul(8, tuple(v % P for v in c.ins))))
        elif c.op == "ge_compress":
            back = ed.decompress(c.exp.to_bytes(32, "little"))
            assert back is not None and F._same_point(back, c.ins)
        elif c.op == "ge_decompress" and c.exp is not None:
            assert F.on_curve(c.exp)
            enc = c.ins[0].to_bytes(32, "little")
            canonical = c.ins[0] % 2 ** 255 < P and not (c.exp[0] == 0 and c.ins[0] >> 255)
            assert (ed.compress(c.exp) == enc) == canonical
    n_bad = sum(1 for c in cases if c.op == "ge_decompress" and c.exp is None)
    assert n_bad >= 10


def test_presentations_keep_the_point():
    rng = np.random.default_rng(9)
    for pt in F.point_singles():
        for mode in F.MODES:
            q = F.present(pt, mode, rng)
            assert F._same_point(q, pt) and F.on_curve(q) and all(0 <= v < F.M256 for v in q)
            assert mode != "lifted" or all(v >= P for v in q)
    ident = F.present(ed.IDENT, "lifted", rng)
    assert ident == (2 * P, 2 * P + 1, 2 * P + 1, 2 * P)      # x + 2p where it fits


def test_tape_round_trips(cases):
    tape = F.pack_tape(cases)
    back, hd = F.unpack_tape(tape)
    assert hd[1] == len(cases) and sum(hd[5:12:2]) == len(cases)
    assert back == [(c.op, tuple(c.ins), c.aux) for c in cases]
    fam = [F.OPS[c.op][1] for c in cases]
    assert fam == sorted(fam)
    for f in range(4):                                         # every family's slice holds that family only
        first, cnt = hd[4 + 2 * f], hd[5 + 2 * f]
        assert cnt > 0 and set(fam[first:first + cnt]) == {f}


def test_check_accepts_the_expected_and_rejects_a_neighbour(cases):
    """the checker itself: a result row made from the expectation passes (on another representative where one exists),
    the same row with one bit flipped does not"""
    seen = set()
    for c in cases:
        if c.op in seen:
            continue
        seen.add(c.op)
        row = np.zeros(F.OUT_WORDS, "<u4")

        def put(k, v):
            row[1 + 8 * k:9 + 8 * k] = np.frombuffer(int(v).to_bytes(32, "little"), "<u4")

        if c.op in ("fe_is_zero", "fe_eq", "fe_is_neg", "sc_lt_L", "ge_is_small_order"):
            row[0] = c.exp
        elif c.op == "sha512_ram":
            row[1:17] = np.frombuffer(c.exp.to_bytes(64, "little"), "<u4")
        elif c.op in ("fe_canon", "sc_reduce512", "ge_compress"):
            put(0, c.exp)
        elif F.OPS[c.op][1] == 0:
            put(0, c.exp + P)
        elif c.op == "ge_decompress":
            row[0] = 1
            for k, v in enumerate((c.exp[0], c.exp[1] + P, 1 + 2 * P, c.exp[3])):
                put(k, v)
        elif c.op == "q_table":
            for k, v in enumerate(c.exp):
                put(k, v + P)
        else:
            for k, v in enumerate(c.exp):
                put(k, v * 7 % P + P)
        assert F.check(c, row) is None, c.op
        row[0 if row[0] or c.op in ("fe_is_zero", "fe_eq", "fe_is_neg", "sc_lt_L", "ge_is_small_order") else 1] ^= 1
        msg = F.check(c, row)
        assert msg is not None and c.op in msg and "0x" in msg
    assert seen == set(F.OPS)


def test_edge_vectors_oracle_agrees_with_python(oracle):
    batches = ed_vectors.build_edge_vectors()
    labels = [l for l, _ in batches]
    assert len(set(labels)) == len(labels)
    assert {len(b) for l, b in batches if l.startswith("n = ")} == {1, 15, 16, 17, 33}
    assert sum(1 for l in labels if l.startswith("msg_len")) == 32 and sum(1 for l in labels if l.startswith("one valid")) == 32
    for label, batch in batches:
        assert len({len(v[1]) for v in batch}) == 1
        for k, m, s, exp in batch:
            py = 0 if not ed.key_decodes(k) else (2 if ed.verify_strict(k, m, s) else 1)
            orc = 0 if not oracle.ed25519_key_decodes(k) else (2 if oracle.ed25519_verify_strict(k, m, s) else 1)
            assert exp == py == orc, (label, k.hex(), s.hex())
