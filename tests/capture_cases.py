"""The semantics corpus of the capture extraction, shared by the CPU tier (tests/capture_model.py over the blob) and the GPU
tier (zke_capture_batch): patterns, seeded haystacks and what Python's `re` / `regex` say about them.

Pattern rule, so that Python and regex-automata agree by construction: no capture group under a * / + / {n,} whose body can
match empty, no empty-matching loop body, and no pattern that matches the empty string."""
import random
import re

# byte mode ((?-u) throughout): the four bench patterns first, then alternation priority, lazy / greedy pairs, optional and
# repeated groups, anchors, the ASCII word boundary
BYTE_PATTERNS = [
    r"from:[^\r\n]*<([a-z]+)@example\.com>\r\n", r"subject:([^\r\n]+)\r\n", r"ZKE-ORDER-([0-9]{8});", r"ZKE-TOKEN-([a-f0-9]{12})!",
    r"from:[^\r\n]*<([a-z]+)@([a-z.]+)>", r"(a|ab)(c|bcd)(d*)", r"(a+?)(a*)b", r"(a+)(a*?)b", r"x(ab|a)(bc|c)?y?", r"(foo|foobar)(bar)?",
    r"([a-z]+)=([0-9]*);?", r"(?:k(\d)+,)+z", r"to:(.*?)<(.+?)>", r"(a|b)*c", r"((a)|(b))+c", r"^(h)ello|(w)orld$", r"\b(\w+)@(\w+)\b",
    r"(?i)Subject:\s*(re:|fwd:)?\s*(.*)\r\n", r"a{2,4}?(a*)", r"(x?)(x?)(x?)xx", r"(?m)^id: (\S+)$", r"(a*)b|(a*)c", r"([^;]*);([^;]*)",
    r"(\d{1,3})\.(\d{1,3})", r"<(?:([a-z]+)\.)?([a-z]+)>",
    r"\A(h)(e)?", r"(o)\z", r"(?s)<(.+)>", r"(?-u:\B)(cd)", r"(ab){2,3}(c)?",
]
# Unicode mode (regex-automata's default): \w \d . and negated classes over scalar values, as UTF-8 automata
UNICODE_PATTERNS = [
    r"(\w+)@(\w+)", r"(\d+)-(\d+)", r"<(.+?)>", r"from:[^\r\n]*<(\w+)@([\w.]+)>", r"([^@\s]+)@", r"(é+)(\w*)", r"(?i)(straße|STRASSE)\s(\d+)",
    r"id=(.)(.)?;",
]

_ALPH = b"abcdxyz019;=<>@. \r\n:kfowrheltHWSubjectRE-,ZKEORDTN!"
_INSERTS = [b"", b"from: Bob <bob@example.com>\r\n", b"subject: hi there\r\n", b"aaab", b"abcd", b"xabcy", b"foobar", b"k1,k22,z", b"hello world",
            b"ZKE-ORDER-12345678;", b"ZKE-TOKEN-0123456789ab!", b"to: A <a@b> <c>", b"id: 77\n", b"aac", b"abbac", b"10.0.12.3", b"<ab.cd>", b"<cd>",
            b"Subject: Re: yo\r\n", b"xxx", b"u@v", b"ababab", b"ababc", b"<a\nb>", b"hello", b"ho", b"abcd cd", b"v 10.5 ", b"\nid: 9\n", b"abab", b"xaxx", b"world"]
_UNI_ALPH = "abz09 @<>-.;=\n\r:éßñ日本語٣٤σΣж"
_UNI_INSERTS = ["", "héllo@wörld", "٣٤-٥٦", "12-34", "<日本語>", "from: Ünï <jürgen@exämple.org>", "ab@", "ééé日本", "Straße 12", "STRASSE 7",
                "id=日;", "id=ab;", "a@b"]


def byte_haystacks(count: int, seed: int):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        base = bytes(rng.choice(_ALPH) for _ in range(rng.randint(0, 60)))
        k = rng.randint(0, len(base))
        out.append(base[:k] + rng.choice(_INSERTS) + base[k:])
    return out


def unicode_haystacks(count: int, seed: int):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        base = "".join(rng.choice(_UNI_ALPH) for _ in range(rng.randint(0, 40)))
        k = rng.randint(0, len(base))
        out.append(base[:k] + rng.choice(_UNI_INSERTS) + base[k:])
    return out


def python_spelling(pattern: str) -> str:
    """The same pattern as Python spells it: \\z is \\Z, a `$` outside (?m) is \\Z too (Python's also matches in front of a final
    line feed, regex-syntax's does not), and (?-u:\\B) is a plain \\B of a bytes pattern."""
    p = pattern.replace(r"\z", r"\Z").replace(r"(?-u:\B)", r"\B").replace(r"(?-u:\b)", r"\b")
    return p if "(?m)" in p else p.replace("$", r"\Z")


def byte_matches(pattern: str, hay: bytes):
    """[(span, [group spans or None ...])] of every match of re.finditer over the bytes."""
    rx = re.compile(python_spelling(pattern).encode())
    out = []
    for m in rx.finditer(hay):
        out.append((m.span(), [None if m.span(g)[0] < 0 else m.span(g) for g in range(1, rx.groups + 1)]))
    return out


def unicode_matches(pattern: str, text: str):
    """The same from the `regex` module over the decoded text, character offsets converted to UTF-8 byte offsets."""
    import regex
    rx = regex.compile(pattern)
    at = [0]
    for ch in text:
        at.append(at[-1] + len(ch.encode("utf-8")))
    conv = lambda sp: None if sp[0] < 0 else (at[sp[0]], at[sp[1]])   # noqa: E731
    return [(conv(m.span()), [conv(m.span(g)) for g in range(1, rx.groups + 1)]) for m in rx.finditer(text)]


def group_count(pattern: str, unicode: bool) -> int:
    if unicode:
        import regex
        return regex.compile(pattern).groups
    return re.compile(python_spelling(pattern).encode()).groups
