"""Helpers of the mixed-extraction tests (zke_extract_captures_mixed) over the pool and the config catalogue of tests/mixed_cases.py.
None of the expectations comes from the entry under test: strings and spans are what Python's `re` finds in the signer's own
canon_header / clean_body, records are the oracle's over inputs built from those `re` captures, origins are tests/qp_map_model.py's
over the oracle's canonical body."""
import ctypes as C
import re
from typing import List, Optional, Sequence

import numpy as np

import mixed_cases as mc
import qp_map_model as Q
from zkemail_rs_amd import _abi as A
from zkemail_rs_amd import regex_compile as rc

NONE = 0xFFFFFFFF
CAP_LDS_STATES = 512            # csrc/capture.hip.h: programs of more states keep their rows in the slot's workspace
CAP_WORK_WAVES = 256            # csrc/pipeline.hip.h: the grid of a capture launch whose rows live there

H_TO_TWO = (r"to:([^\r\n<]*)<([^>\r\n]+)>\r\n", [1, 2])                 # two groups in one part
# the ORDER pattern followed by a large optional bounded repetition: more than CAP_LDS_STATES program states, the same group 1
BIG_ORDER = (r"ZKE-ORDER-([0-9]{8});(?:[a-z =\r\n]{0,300})?", [1])

EXTRA_CONFIGS = {
    "GZERO": ([mc.H_SUBJ_LINE, mc.H_FROM_DOMAIN], []),                     # no requested group at all: G = 0
    "TWO": ([H_TO_TWO], [mc.B_ORDER]),
    "BIGNINE": ([mc.H_FROM, mc.H_SUBJ, mc.H_TO, mc.H_SUBJ_LINE, mc.H_FROM_DOMAIN], [BIG_ORDER, mc.B_TOKEN, mc.B_ORDER, mc.B_TOKEN]),
    "X_MISSING": ([(mc.H_FROM[0], [1, 2]), mc.H_SUBJ], []),                # part 0 asks the from pattern for a group it lacks
    "Y_SUBJ_FIRST": ([mc.H_SUBJ, mc.H_FROM], []),
}


def catalogue(name: str):
    return mc.CONFIGS[name] if name in mc.CONFIGS else EXTRA_CONFIGS[name]


def regex_config(name: Optional[str]) -> Optional[rc.RegexConfig]:
    """The RegexConfig of a catalogue entry (None stays None); a side without parts is None, as mixed_cases.parts_for has it."""
    if name is None:
        return None
    hp, bp = catalogue(name)
    side = lambda parts: [rc.RegexPattern(p, list(g)) for p, g in parts] or None
    return rc.RegexConfig(side(hp), side(bp))


def oracle_input(pool_ix: int, name: Optional[str]):
    """mixed_cases.make_input for a name of either catalogue."""
    m = mc.pool()[pool_ix % mc.POOL_N]
    return m.email if name is None else A.EmailWithRegex(m.email, mc.parts_for(m, catalogue(name)))


def re_captures(mail: mc.PoolMail, name: str):
    """Per part of the config, header parts first: (strings, spans) of the requested groups by `re`, or None where the part does
    not match exactly once."""
    hp, bp = catalogue(name)
    out = []
    for k, (pat, groups) in enumerate(hp + bp):
        hay = mail.canon_header if k < len(hp) else mail.clean_body
        ms = list(re.finditer(pat.encode(), hay))
        out.append(None if len(ms) != 1 else ([ms[0].group(g) for g in groups], [ms[0].span(g) for g in groups]))
    return out


def model_origins(oracle, mail: mc.PoolMail, name: str):
    """Per column of the e-mail (an OK e-mail): (start, end, flags) by the rule of zke_extract_captures_mapped — header columns
    are their spans, body columns go through the index map of the oracle's canonical body."""
    hp, bp = catalogue(name)
    body = mail.email.raw_email.split(b"\r\n\r\n", 1)[1]
    canon = oracle.canon_body(body, True)
    cleaned, im, kept = Q.remove_qp(canon)
    assert cleaned[:kept] == mail.clean_body
    out = []
    for k, part in enumerate(re_captures(mail, name)):
        for s, e in part[1]:
            out.append((s, e, 0) if k < len(hp) else Q.origin(im, len(canon), s, e))
    return out


class Extraction:
    """One synchronous zke_extract_captures_mixed through ctypes with buffers of the sizes the header's formulas give."""

    def __init__(self, eng, emails, names: Sequence[Optional[str]], origins=True, lists=None, blob_bytes=None):
        self.lists = lists if lists is not None else eng.pack_capture_mixed([regex_config(x) for x in names], unicode=False)[0]
        self.refs = A.EmailRefs(emails)
        L = self.lists
        (self.out, self.spans, self.flags, self.cap_off, self.cap_str_off, self.blob, (self.ospans, self.oflags)) = \
            eng._capture_mixed_call(self.refs, L, origins, blob_bytes)
        self.n = self.refs.n

    def strings(self, i: int) -> List[List[bytes]]:
        """Per part of e-mail i its strings."""
        raw, L = self.blob.tobytes(), self.lists
        return [[raw[self.cap_str_off[k]:self.cap_str_off[k + 1]] for k in range(self.cap_off[j], self.cap_off[j + 1])]
                for j in range(int(L.job_off[i]), int(L.job_off[i + 1]))]

    def columns(self, i: int):
        a, b = int(self.lists.col_off[i]), int(self.lists.col_off[i + 1])
        return self.spans[a:b], self.flags[a:b], self.ospans[a:b], self.oflags[a:b]


def check_against_re(x: Extraction, oracle, pool_ix: Sequence[int], names: Sequence[Optional[str]], exp, origins=True, ctx=""):
    """Strings and spans against `re`, flags 0, origins against the model for the e-mails the ORACLE passes; no string, no span
    and identity origins for the others; no job and no column for an e-mail without a config."""
    L = x.lists
    for i, (k, name) in enumerate(zip(pool_ix, names)):
        spans, flags, ospans, oflags = x.columns(i)
        if name is None:
            assert L.job_off[i] == L.job_off[i + 1] and L.col_off[i] == L.col_off[i + 1], (ctx, i)
            continue
        if int(exp[i]["status"]) != A.ZKE_OK:
            assert all(s == [] for s in x.strings(i)) and (spans == NONE).all() and not flags.any(), (ctx, i, name)
            if origins:
                assert (ospans == NONE).all() and not oflags.any(), (ctx, i, name)
            continue
        mail = mc.pool()[k % mc.POOL_N]
        want = re_captures(mail, name)
        assert all(w is not None for w in want), (ctx, i, name)
        assert x.strings(i) == [w[0] for w in want], (ctx, i, name, x.strings(i))
        assert [tuple(int(v) for v in s) for s in spans] == [sp for w in want for sp in w[1]], (ctx, i, name)
        assert not flags.any(), (ctx, i, name)
        if origins:
            got = [(int(o[0]), int(o[1]), int(f)) for o, f in zip(ospans, oflags)]
            assert got == model_origins(oracle, mail, name), (ctx, i, name)


def verify_mixed_lists(x: Extraction) -> A.MixedLists:
    """The zke_regex_mixed that hands an extraction's tables VERBATIM to zke_verify_emails_mixed: the configs' DFA ids, config_of,
    and cap_off / cap_str_off / cap_blob as delivered."""
    L = x.lists
    ml = A.MixedLists([([d for d, _, _ in h], [d for d, _, _ in b]) for h, b in L.configs], [int(c) for c in L.config_of[:L.n]], None)
    ml.keep = (x.cap_off, x.cap_str_off, np.concatenate([x.blob, np.zeros(1, np.uint8)]))
    ml.c.cap_off, ml.c.cap_str_off, ml.c.cap_blob = (a.ctypes.data for a in ml.keep)
    return ml
