"""Inputs of the mixed-regex tests (zke_verify_emails_mixed): one pool of signed e-mails, a catalogue of regex configs built from
synth.HEADER_PATTERNS / synth.BODY_PATTERNS and a few patterns of test_regex_dfa.PATTERNS, and the expectation: the inputs grouped
by config, every group through the oracle as it runs a single-config batch today (the plain Email list for the e-mails without a
config), the records scattered back.  E-mails are verified in isolation (core/src/circuits.rs:31-68 takes one EmailWithRegex at a
time), so that IS the reference's answer for the mixed list."""
import functools
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import synth
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import regex_compile as rc

FIELDS = [f for f in A.RESULT_DTYPE.names if f != "reserved"]

H_FROM, H_SUBJ = synth.HEADER_PATTERNS
B_ORDER, B_TOKEN = synth.BODY_PATTERNS
H_TO = (r"to:([^\r\n]+)\r\n", [1])                      # the next three: test_regex_dfa.PATTERNS
H_SUBJ_LINE = (r"subject:[^\r\n]+\r\n", [])
H_FROM_DOMAIN = (r"from:[^\r\n]*@example\.com", [])
UNI_ORDER = r"ZKE-ORDER-(\d{8});"                       # compiled in Unicode mode: \d is the Unicode class, the tables are large

# name -> (header parts, body parts), each part (pattern, capture groups)
CONFIGS: Dict[str, Tuple[list, list]] = {
    "A": ([H_FROM, H_SUBJ], []),
    "B": ([H_SUBJ], [B_ORDER, B_TOKEN]),
    "C": ([H_TO], [B_TOKEN, B_ORDER]),
    "D": ([], [B_ORDER]),
    "ONE": ([H_FROM], []),
    "NINE": ([H_FROM, H_SUBJ, H_TO, H_SUBJ_LINE, H_FROM_DOMAIN], [B_ORDER, B_TOKEN, B_ORDER, B_TOKEN]),
    "ORDER_IN_HEADER": ([B_ORDER], []),                 # the pair that "D" uses as a body part, as a header part
    "THREE": ([H_SUBJ, H_FROM], [B_ORDER]),
    "ZERO": ([], []),                                   # verify_email_with_regex with both lists None
}

POOL_N = 24
BODY_LEN = 600


@functools.lru_cache(maxsize=None)
def dfa_of(pattern: str, unicode: bool = False) -> A.DFA:
    return rc.create_dfa(pattern, unicode=unicode)


class PoolMail:
    def __init__(self, email, canon_header, clean_body, kind):
        self.email, self.canon_header, self.clean_body, self.kind = email, canon_header, clean_body, kind


@functools.lru_cache(maxsize=None)
def pool() -> List[PoolMail]:
    """24 signed e-mails with 600-byte bodies: every third one quoted-printable (a marker may straddle a soft break); per eight one
    with a broken signature ("badsig"), one without the TOKEN marker ("notoken"), one with two signed Subject headers ("twosubj") and
    one whose Subject also carries the ORDER marker ("ordersubj": the ORDER pattern then matches once in the header preimage)."""
    rng = np.random.default_rng(20241)
    keys = synth.keys_of(2048, 4)
    out = []
    for i in range(POOL_N):
        kind = {2: "ordersubj", 5: "badsig", 6: "notoken", 7: "twosubj"}.get(i % 8, "plain")
        qp = 0.12 if i % 3 == 0 else 0.0
        order = b"ZKE-ORDER-%08d;" % int(rng.integers(0, 10**8))
        for _ in range(50):          # (a body this short may leave no two free lines for the second marker: draw another)
            try:
                body = synth.ascii_body(rng, BODY_LEN, qp_frac=qp)
                used: set = set()
                body = synth.inject_marker(body, rng, order, split=bool(qp) and i % 2 == 0, used=used)
                if kind != "notoken":
                    body = synth.inject_marker(body, rng, b"ZKE-TOKEN-%012x!" % int(rng.integers(0, 16**12)), split=False, used=used)
                break
            except ValueError:
                continue
        else:
            raise ValueError("no body with room for both markers")
        hs = synth.std_headers(rng, i, "example.com", pad_to=760)
        spec = synth.SignSpec(domain="example.com")
        if kind == "twosubj":
            hs.append((b"Subject", b"second subject line"))
            spec.signed = ("from", "to", "subject", "subject", "date", "message-id")
        if kind == "ordersubj":
            hs = [(n, v + b" " + order if n == b"Subject" else v) for n, v in hs]
        raw, it = synth.sign_email(hs, body, keys[i % len(keys)], spec, corrupt="body" if kind == "badsig" else None)
        em = A.Email("example.com", raw, A.PublicKey(keys[i % len(keys)].pkcs1_der, "rsa"))
        out.append(PoolMail(em, it["canon_header"], it["canon_body"].replace(b"=\r\n", b""), kind))
    return out


def two_signature_mails() -> List[A.Email]:
    """E-mails whose first DKIM-Signature header is not the verified one: the corpus case with a foreign-domain signature in front
    (canonicalize_signed_email succeeds on it), and the same with a first signature whose c= tag canonicalize_signed_email refuses
    (circuits.rs:34-35 panics: a zero-part config reports it, verify_email alone does not)."""
    import cases
    c = [x for x in cases.build_cases() if x.name == "pass_two_signatures"][0]
    k0, k1 = synth.load_keys()["rsa2048_00"], synth.load_keys()["rsa2048_01"]
    hs, body = cases._hdrs(20), cases._body(400, 20)
    raw, _ = synth.sign_email(hs, body, k0, synth.SignSpec())
    raw_other, _ = synth.sign_email(hs, body, k1, synth.SignSpec(domain="other.org", selector="o1", c_tag="nofws/simple"))
    other_sig_hdr = raw_other[:raw_other.find(b"Received:")]
    return [c.email, A.Email("example.com", other_sig_hdr + raw, A.PublicKey(k0.pkcs1_der))]


def parts_for(mail: PoolMail, cfg: Tuple[list, list]):
    """The RegexInfo of one pool e-mail under a config: the captures are what Python's `re` finds (["?"] where it finds nothing)."""
    def side(parts, hay):
        out = []
        for pat, groups in parts:
            m = re.search(pat.encode(), hay)
            out.append(A.CompiledRegex(dfa_of(pat), [m.group(g).decode() for g in groups] if m else ["?"]))
        return out
    return A.RegexInfo(side(cfg[0], mail.canon_header) or None, side(cfg[1], mail.clean_body) or None)


def make_input(pool_ix: int, cfg_name: Optional[str]):
    """An Email (cfg_name None: no config) or an EmailWithRegex of pool e-mail pool_ix."""
    m = pool()[pool_ix % POOL_N]
    return m.email if cfg_name is None else A.EmailWithRegex(m.email, parts_for(m, CONFIGS[cfg_name]))


def workload(assign: Sequence[Optional[str]], start: int = 0, spoil: bool = True):
    """One input per entry of `assign` (a config name or None), pool members in turn.  With `spoil`, the second member of every
    config that has parts gets a capture that its match does not contain (a failure at the regex stage whatever the patterns)."""
    inputs, seen = [], {}
    for k, name in enumerate(assign):
        inp = make_input(start + k, name)
        if name is not None:
            seen[name] = seen.get(name, 0) + 1
            parts = (inp.regex_info.header_parts or []) + (inp.regex_info.body_parts or [])
            if spoil and seen[name] == 2 and parts:
                parts[-1].captures = ["nobody-wrote-this"]
        inputs.append(inp)
    return inputs


def expectation(oracle, inputs, keys: Sequence) -> np.ndarray:
    """keys[i]: what groups input i with the others of its config (None: no config).  Every group through the oracle on its own."""
    exp = np.zeros(len(inputs), dtype=A.RESULT_DTYPE)
    groups: Dict[object, List[int]] = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    for k, idx in groups.items():
        if k is None:
            rec = oracle.verify_batch(A.PackedBatch([inputs[i] for i in idx]), threads=4)
        else:
            rec = oracle.verify_batch(oracle.pack_with_regex([inputs[i] for i in idx]), threads=4)
        for j, i in enumerate(idx):
            exp[i] = rec[j]
    return exp


REGEX_STAGE = (A.ZKE_HEADER_REGEX_FAIL, A.ZKE_BODY_REGEX_FAIL, A.ZKE_DFA_DECODE_FAIL, A.ZKE_CANON_FAIL)


def check_not_vacuous(exp, keys, regex_failures: bool, all_fail: Sequence = ()):
    """On the ORACLE's records, before the engine's are looked at: every populated config has an e-mail that passes (the configs in
    `all_fail` excepted: a junk pair fails all of its e-mails), and with `regex_failures` one that fails at the regex stage."""
    for k in set(keys) - {None}:
        st = [int(exp[i]["status"]) for i in range(len(keys)) if keys[i] == k]
        if k in all_fail:
            assert any(s == A.ZKE_DFA_DECODE_FAIL for s in st), k
            continue
        assert any(s == A.ZKE_OK for s in st), (k, st)
        if regex_failures:
            assert any(s in REGEX_STAGE for s in st), (k, st)


def assert_equal(got, exp, ctx=""):
    assert len(got) == len(exp), ctx
    for i in range(len(exp)):
        for f in FIELDS:
            g, x = got[i][f], exp[i][f]
            same = (g == x).all() if hasattr(g, "all") else g == x
            assert same, f"{ctx} e-mail {i} field {f}: engine={g} oracle={x} [engine status {got[i]['status']}/{got[i]['detail']} " \
                         f"oracle {exp[i]['status']}/{exp[i]['detail']}]"
