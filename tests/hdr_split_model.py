"""The mailparse header split of csrc/hdrsplit.hip.h, stated twice on the CPU — test infrastructure.

`serial`       scan_headers (the serial walk: the fallback of round 0, the only path of later signature rounds and of the
               MIME sub-part walk) as plain Python over bytes.
`lines`        split_headers_lines (the line-parallel path every ordinary e-mail takes) restated ON ITS OWN DATA LAYOUT:
               64-byte chunks with the 64-bit ballots Lm / Cm / Bm, the first ':' of each line from the addition
               ca + cb + cin, the lfpos / colpos tables capped at LINE_CAP, 64 lines per step with continuation decided by
               a + b + vcarry, the error order from the `bad` ballot, the value end written by the lane of a header's last
               line.  A byte beyond `staged` = min(len, 3568) reads as OOB.  It returns None exactly where the kernel
               returns false, and records in `census` (a Counter) which of its branches an input met, so that
               test_hdr_split_model.py can certify what each population of hdr_split_cases.py reaches.
`body_offset`  find_body: the first CRLFCRLF that starts at or after hdr_end - 2, else len.
`route`        which of the two splits answers in round 0.

Results are ("ok", [(key_start, key_end, val_start, val_end), ...], hdr_end) or (cause, None, None) with cause one of
"lead" (ZKE_D_HDR_LEADING_SPACE), "lonecr" (ZKE_D_HDR_LONE_CR), "many" (ZKE_D_U_TOO_MANY_HEADERS); hdr_end is the offset of
the empty line (len when there is none).
"""
from __future__ import annotations

from collections import Counter
from typing import Optional

import numpy as np

ZKE_MAX_HEADERS = 256
PARSE_STAGE_BYTES = 3568
LINE_CAP = 512
HDR_LDS_ENTRIES = 64
OOB = 0x100
M64 = (1 << 64) - 1
LF, CR, SP, HT, COLON = 10, 13, 32, 9, 58
NOCOL = 0xFFFF


# ------------------------------------------------------------------ the serial walk
def serial(raw: bytes, max_headers: int = ZKE_MAX_HEADERS):
    n = len(raw)
    ix = 0
    spans = []
    while ix < n:
        c0 = raw[ix]
        if c0 == LF:
            break
        if c0 == CR:
            if ix + 1 < n and raw[ix + 1] == LF:
                break
            return ("lonecr", None, None)
        if c0 == SP:
            return ("lead", None, None)
        p = ix
        while p < n and raw[p] != COLON and raw[p] != LF:
            p += 1
        if p >= n:
            key_end = vs = ve = nxt = n
        elif raw[p] == LF:
            key_end = vs = ve = p
            nxt = p + 1
        else:
            key_end = p
            vs = p + 1
            while vs < n and raw[vs] == SP:
                vs += 1
            q = vs
            while True:
                q = raw.find(b"\n", q)
                if q < 0:
                    q = n
                    break
                if q + 1 < n and raw[q + 1] in (SP, HT):
                    q += 1
                    continue
                break
            nxt = q + 1 if q < n else n
            ve = min(q, n)
            while ve > vs and raw[ve - 1] in (CR, LF):
                ve -= 1
        if len(spans) >= max_headers:
            return ("many", None, None)
        spans.append((ix, key_end, vs, ve))
        ix = nxt
    return ("ok", spans, ix)


# ------------------------------------------------------------------ the line-parallel split
def _ballots(data: bytes, byte: int) -> int:
    """Bit p set where data[p] == byte: every chunk's ballot at once (chunk `base` is bits base .. base + 63)."""
    if not data:
        return 0
    hit = np.frombuffer(data, np.uint8) == byte
    return int.from_bytes(np.packbits(hit, bitorder="little").tobytes(), "little")


def _below(k: int) -> int:
    return (1 << k) - 1


def _ctz(x: int) -> int:
    return (x & -x).bit_length() - 1


_pop = int.bit_count if hasattr(int, "bit_count") else (lambda x: bin(x).count("1"))


def _bits(x: int):
    while x:
        b = x & -x
        yield b.bit_length() - 1
        x ^= b


def lines(raw: bytes, census: Optional[Counter] = None):
    cz = census if census is not None else Counter()
    n = len(raw)
    staged = min(n, PARSE_STAGE_BYTES)
    stage = raw[:staged]

    def sb(pos):
        return stage[pos] if pos < staged else OOB

    if n == 0:
        cz["empty input"] += 1
        return ("ok", [], 0)
    if sb(0) == LF or (sb(0) == CR and sb(1) == LF):
        cz["empty list"] += 1
        return ("ok", [], 0)
    # ---- pass A: 64 bytes per step.  The look-ahead bytes n1 / n2 of lane l are bytes l + 1 / l + 2 of the staged part, so
    # a lane's "LF followed by LF or CRLF" is the LF ballot ANDed with the shifted ballots; beyond `staged` every ballot is 0.
    all_lf, all_col, all_cr = _ballots(stage, LF), _ballots(stage, COLON), _ballots(stage, CR)
    all_blank = all_lf & ((all_lf >> 1) | ((all_cr >> 1) & (all_lf >> 2)))
    lfpos = [None] * LINE_CAP
    colpos = [None] * LINE_CAP
    colpos[0] = NOCOL
    n_lines, cut, colon_seen = 0, None, False
    for base in range(0, staged, 64):
        Lm, Cm, Bm = (all_lf >> base) & M64, (all_col >> base) & M64, (all_blank >> base) & M64
        cutbit = 64
        if Bm:
            cutbit = _ctz(Bm)
            Lm &= _below(cutbit + 1)
            Cm &= _below(cutbit)
        for lane in _bits(Lm):
            line = n_lines + _pop(Lm & _below(lane))
            if line < LINE_CAP:
                lfpos[line] = base + lane
            if line + 1 < LINE_CAP:
                colpos[line + 1] = NOCOL
        ca, cb, cin = ~Cm & M64, Lm, 0 if colon_seen else 1
        total = (ca + cb + cin) & M64
        F = Cm & (total ^ ca ^ cb)
        for lane in _bits(F):
            line = n_lines + _pop(Lm & _below(lane))
            if line < LINE_CAP:
                colpos[line] = base + lane
        colon_seen = ((((ca & cb) | ((ca | cb) & ~total)) >> 63) & 1) == 0
        n_lines += _pop(Lm)
        if Bm:
            cut = base + cutbit
            cz[("cut lane", cutbit)] += 1
            break
        if base + 64 < staged and not (Lm >> 63) & 1:
            cz[("colon_seen at a chunk edge inside a line", colon_seen)] += 1
    if cut is None:
        cz[("fallback", "no empty line in the staged part")] += 1
        return None
    if n_lines > LINE_CAP:
        cz[("fallback", "more than LINE_CAP lines")] += 1
        return None
    # ---- pass B: 64 lines per step, one lane per line
    hdr = [[None] * 4 for _ in range(ZKE_MAX_HEADERS)]
    start_group = [None] * ZKE_MAX_HEADERS
    nh, vcarry = 0, 0
    for G in range(0, n_lines, 64):
        lanes = range(min(64, n_lines - G))
        VM = _below(len(lanes))
        s, e, c0, c1, col, nx = ([0] * 64 for _ in range(6))
        Wm = Cm = Em = 0
        for lane in lanes:
            g = G + lane
            s[lane] = lfpos[g - 1] + 1 if g else 0
            e[lane] = lfpos[g]
            assert e[lane] + 1 < staged                  # pass A read it: it is staged
            c0[lane], c1[lane] = stage[s[lane]], stage[s[lane] + 1]
            col[lane] = colpos[g]
            nx[lane] = stage[e[lane] + 1]
            if c0[lane] in (SP, HT):
                Wm |= 1 << lane
            if col[lane] != NOCOL:
                Cm |= 1 << lane
            if c0[lane] == SP or (c0[lane] == CR and c1[lane] != LF):
                Em |= 1 << lane
        a, b = Wm | Cm, Cm
        Vprev = ((a + b + vcarry) ^ a ^ b) & M64
        cont = Wm & Vprev
        HS = VM & ~cont
        too_many = 0
        if nh + _pop(HS) > ZKE_MAX_HEADERS:                # (else no lane's header number reaches the limit)
            for lane in _bits(HS):
                if nh + _pop(HS & _below(lane)) >= ZKE_MAX_HEADERS:
                    too_many |= 1 << lane
        bad = (HS & Em) | too_many
        if bad:
            f = _ctz(bad)
            fc = c0[f]
            cause = "lead" if fc == SP else "lonecr" if fc == CR else "many"
            rest = bad & ~(1 << f)
            others = set()
            for lane in _bits(rest):
                if (HS & Em) >> lane & 1:
                    others.add("lead" if c0[lane] == SP else "lonecr")
                else:
                    others.add("many")
            cz[("bad first", cause, "another cause behind" if others - {cause} else "alone")] += 1
            return (cause, None, None)
        for lane in lanes:
            hs = (HS >> lane) & 1
            C = (Cm >> lane) & 1
            if hs:
                hr = nh + _pop(HS & _below(lane))
                ke = vs = e[lane]
                if C:
                    ke = col[lane]
                    vs = col[lane] + 1
                    while stage[vs] == SP:
                        vs += 1
                hdr[hr][0:3] = [s[lane], ke, vs]
                start_group[hr] = G
                if not C:
                    hdr[hr][3] = e[lane]
            inval = C if hs else 1
            if inval and nx[lane] not in (SP, HT):
                q = e[lane]
                while q > s[lane] and stage[q - 1] in (CR, LF):
                    q -= 1
                h = nh + _pop(HS & _below(lane + 1)) - 1
                hdr[h][3] = q
                cz[("value end", "LDS" if h < HDR_LDS_ENTRIES else "overflow",
                    "same group" if start_group[h] == G else "a later group than the header start")] += 1
        nh += _pop(HS)
        vcarry = ((Cm >> 63) & 1) | (((Wm >> 63) & 1) & ((Vprev >> 63) & 1))
        if G + 64 < n_lines:
            cz[("vcarry at a group edge", vcarry)] += 1
    cz[("header table", "LDS only" if nh <= HDR_LDS_ENTRIES else "LDS and overflow")] += 1
    spans = [tuple(hdr[h]) for h in range(nh)]
    assert all(x is not None for sp in spans for x in sp)
    return ("ok", spans, cut + 1)


# ------------------------------------------------------------------ the body and the route
def body_offset(raw: bytes, hdr_end: int) -> int:
    i = raw.find(b"\r\n\r\n", max(hdr_end - 2, 0))
    return i + 4 if i >= 0 else len(raw)


def route(raw: bytes) -> str:
    return "serial" if lines(raw) is None else "lines"
