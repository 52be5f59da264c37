"""A plain-Python interpreter of the capture-program BLOB (zkemail_rs_amd.regex_compile.create_capture_program; layout in
DESIGN.md §3): decode the bytes with the checks the engine's host reader makes, then a leftmost-first Pike simulation with
capture slots.  It shares no code with the compiler's NFA classes: what it knows about a program it has read from the blob."""
import struct

MAGIC, VERSION, HEADER_WORDS = 0x50434B5A, 1, 8
FAIL, MATCH, RANGE, SPARSE, LOOK, UNION, CAPTURE = range(7)
LOOKS = (1, 2, 4, 8, 64, 128)                # Look::{Start, End, StartLF, EndLF, WordAscii, WordAsciiNegate}
MAX_STATES, MAX_PROGRAM_GROUPS = 8192, 32    # ZKE_CAP_MAX_STATES, ZKE_CAP_MAX_PROGRAM_GROUPS
D_U_CAPTURE_STATES, D_U_CAPTURE_PROGRAM = 91, 94


class BadProgram(ValueError):
    def __init__(self, detail):
        super().__init__(f"capture program refused (detail {detail})")
        self.detail = detail


class Program:
    def __init__(self, blob: bytes):
        bad = BadProgram(D_U_CAPTURE_PROGRAM)
        if len(blob) < 4 * HEADER_WORDS or len(blob) % 4:
            raise bad
        w = struct.unpack(f"<{len(blob) // 4}I", blob)
        magic, version, self.n_states, self.n_groups, self.start, flags, n_words, zero = w[:8]
        if magic != MAGIC or version != VERSION or zero or flags > 1 or not self.n_states or not self.n_groups or self.start >= self.n_states:
            raise bad
        if HEADER_WORDS + self.n_states + 1 + n_words != len(w):
            raise bad
        if self.n_states > MAX_STATES or self.n_groups > MAX_PROGRAM_GROUPS:
            raise BadProgram(D_U_CAPTURE_STATES)
        self.unicode = bool(flags)
        N = self.n_states
        off = w[8:8 + N + 1]
        st = w[8 + N + 1:]
        if off[0] != 0 or off[N] != n_words:
            raise bad
        self.states = []
        for q in range(N):
            if off[q + 1] <= off[q] or off[q + 1] > n_words:
                raise bad
            o, ln = off[q], off[q + 1] - off[q]
            kind, cnt = st[o] & 0xFF, st[o] >> 8
            if kind in (FAIL, MATCH):
                if cnt or ln != 1:
                    raise bad
                self.states.append((kind,))
            elif kind in (RANGE, SPARSE):
                if cnt == 0 or cnt > 256 or (kind == RANGE and cnt != 1) or ln != 1 + 2 * cnt:
                    raise bad
                trans, floor = [], 0
                for k in range(cnt):
                    r, nxt = st[o + 1 + 2 * k], st[o + 2 + 2 * k]
                    lo, hi = r & 0xFF, (r >> 8) & 0xFF
                    if r >> 16 or lo > hi or lo < floor or nxt >= N:
                        raise bad
                    floor = hi + 1
                    trans.append((lo, hi, nxt))
                self.states.append((kind, trans))
            elif kind == LOOK:
                if cnt or ln != 3 or st[o + 1] not in LOOKS or st[o + 2] >= N:
                    raise bad
                self.states.append((kind, st[o + 1], st[o + 2]))
            elif kind == UNION:
                if ln != 1 + cnt or any(x >= N for x in st[o + 1:o + 1 + cnt]):
                    raise bad
                self.states.append((kind, list(st[o + 1:o + 1 + cnt])))
            elif kind == CAPTURE:
                if cnt or ln != 3 or st[o + 1] >= 2 * self.n_groups or st[o + 2] >= N:
                    raise bad
                self.states.append((kind, st[o + 1], st[o + 2]))
            else:
                raise bad


def _word(b):
    return b == 0x5F or 0x30 <= b <= 0x39 or 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A


def look_holds(look, hay, pos):
    if look == 1:
        return pos == 0
    if look == 2:
        return pos == len(hay)
    if look == 4:
        return pos == 0 or hay[pos - 1] == 0x0A
    if look == 8:
        return pos == len(hay) or hay[pos] == 0x0A
    left = pos > 0 and _word(hay[pos - 1])
    right = pos < len(hay) and _word(hay[pos])
    return (left != right) if look == 64 else (left == right)


def captures_at(prog: Program, hay: bytes, start: int):
    """The leftmost-first match of the program anchored at `start`: its slots [s0, e0, s1, e1, ...] (None = the group took no
    part), or None when nothing matches there.  Pike's algorithm: a priority-ordered thread list, slots per thread."""
    S = prog.states

    def add(lst, seen, q, slots, pos):
        stack = [(q, slots)]
        while stack:
            q, slots = stack.pop()
            if q in seen:
                continue
            seen.add(q)
            t = S[q]
            if t[0] == UNION:
                for x in reversed(t[1]):
                    stack.append((x, slots))
            elif t[0] == LOOK:
                if look_holds(t[1], hay, pos):
                    stack.append((t[2], slots))
            elif t[0] == CAPTURE:
                s2 = list(slots)
                s2[t[1]] = pos
                stack.append((t[2], tuple(s2)))
            else:
                lst.append((q, slots))

    cur = []
    add(cur, set(), prog.start, (None,) * (2 * prog.n_groups), start)
    best = None
    pos = start
    while cur:
        nxt, seen = [], set()
        for q, slots in cur:
            t = S[q]
            if t[0] == MATCH:
                best = list(slots)
                break                                  # leftmost-first: the threads behind this one are cut
            if t[0] in (RANGE, SPARSE) and pos < len(hay):
                for lo, hi, to in t[1]:
                    if lo <= hay[pos] <= hi:
                        add(nxt, seen, to, slots, pos + 1)
                        break
        cur = nxt
        pos += 1
    return best
