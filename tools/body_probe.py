"""Time body_extract_kernel against the same build's parse_kernel on one batch (not bench.py: nothing here is a threshold).

The batch has the shape of BASELINE configs[1] — 1 024 DKIM-signed e-mails, 4 KB of body text each, 16 RSA-2048 keys — with every
e-mail wrapped as a two-part multipart/alternative: a text/plain part, then the text/html part that holds the body under a
Content-Transfer-Encoding.  Three legs, one per encoding of that part:

  (b) base64            (q) quoted-printable            (i) identity (7bit)

Per leg: zke_extract_bodies — the device time of body_extract_kernel from the engine's HIP events (zke_set_timing;
zke_timings.front_end_us is the launch) and the host clock around the synchronous C call — and zke_verify_emails over the SAME bytes,
whose front_end_us is parse_kernel (the wrapping changes the body, so the signatures no longer verify; the front end's work — header
split, MIME walk, tag lists, canonicalisation — does not depend on that).  Every extraction is compared with tests/body_model.py first.

The expectation on record: the decode is one pass over at most the e-mail's bytes with no hashing, so it should cost no more than the
front end.  If it costs more, the quoted-printable carries are the first suspect.

    python tools/body_probe.py --out profiles/body_probe.txt
"""
import argparse
import base64
import ctypes as C
import os
import quopri
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[-(len(xs) // 10) - 1]


def fmt(t):
    return f"{t[0]:9.1f} us [{t[1]:.1f} .. {t[2]:.1f}]"


def wrap(raw: bytes, k: int, leg: str) -> bytes:
    """The signed e-mail `raw` as a multipart/alternative: its header block plus a Content-Type header, its body as the text/html part."""
    head, body = raw.split(b"\r\n\r\n", 1)
    # the workload's own (unsigned) MIME headers make way for the multipart's
    head = b"\r\n".join(ln for ln in head.split(b"\r\n") if not ln.lower().startswith((b"mime-version:", b"content-type:", b"content-transfer-encoding:")))
    bound = b"=_probe_%04d" % k
    if leg == "b":
        cte, text = b"base64", base64.encodebytes(body).replace(b"\n", b"\r\n")
    elif leg == "q":
        cte, text = b"quoted-printable", quopri.encodestring(body.replace(b"\r\n", b"\n")).replace(b"\n", b"\r\n")
    else:
        cte, text = b"7bit", body
    if not text.endswith(b"\r\n"):
        text += b"\r\n"
    return (head + b"\r\nMIME-Version: 1.0\r\nContent-Type: multipart/alternative;\r\n boundary=\"" + bound + b"\"\r\n\r\n"
            b"--" + bound + b"\r\nContent-Type: text/plain; charset=utf-8\r\n\r\nsee the html part\r\n"
            b"--" + bound + b"\r\nContent-Type: text/html; charset=utf-8\r\nContent-Transfer-Encoding: " + cte + b"\r\n\r\n" + text +
            b"--" + bound + b"--\r\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--body", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import body_model as M
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A
    from zkemail_rs_amd.engine import _BodyBuffers

    eng = z.Engine()
    eng.set_timing(True)

    def timed(call, fields):
        wall, dev = [], {f: [] for f in fields}
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e6
            if k >= args.warmup:
                wall.append(dt)
                t = eng.timings()
                for f in fields:
                    dev[f].append(t[f])
        return med(wall), {f: med(v) for f, v in dev.items()}

    wl = synth.make_workload("c2", args.n, args.body, rsa_bits=2048, n_keys=16, seed=4242)
    lines = [f"body_probe: steps={args.steps} warmup={args.warmup}",
             f"batch: n={args.n} e-mails of the configs[1] shape ({args.body} B of body text, RSA-2048), each wrapped as multipart/alternative "
             "{text/plain, text/html under the leg's Content-Transfer-Encoding}"]
    for leg, name in (("b", "base64"), ("q", "quoted-printable"), ("i", "identity")):
        raws = [wrap(e.raw_email, k, leg) for k, e in enumerate(wl.emails)]
        emails = [A.Email(e.from_domain, r, e.public_key) for e, r in zip(wl.emails, raws)]
        got = eng.extract_bodies(raws)
        for g, raw in zip(got[:64], raws[:64]):
            want = M.extract(raw)
            assert (g.status, g.part, g.encoding, g.body) == (0, want.part, want.encoding, want.data), "the engine and the model agree on the probe's batch"
        assert all(g.status == 0 and g.part == (2 | A.BODY_PART_HTML) for g in got)
        b = _BodyBuffers(raws)

        def extract():
            rc = eng.lib.zke_extract_bodies(eng.h, b.arr, b.n, 0, C.byref(b.c))
            assert rc == 0, rc
        w, d = timed(extract, ("front_end_us", "h2d_us", "d2h_us"))
        refs = A.EmailRefs(emails)
        out = eng.verify_emails(refs)
        wv, dv = timed(lambda: eng.verify_emails(refs), ("front_end_us", "total_us"))
        total = sum(len(r) for r in raws)
        lines.append(f"  ({leg}) {name}: {total / len(raws):.0f} B per e-mail, {sum(len(g.body) for g in got) / len(got):.0f} B per decoded body")
        lines.append(f"      body_extract_kernel (front_end_us)   {fmt(d['front_end_us'])}   h2d {fmt(d['h2d_us'])}   d2h {fmt(d['d2h_us'])}")
        lines.append(f"      zke_extract_bodies, the C call       {fmt(w)}   host clock")
        lines.append(f"      parse_kernel on the same bytes       {fmt(dv['front_end_us'])}   (zke_verify_emails: launches first to last {fmt(dv['total_us'])}, host clock {fmt(wv)}; "
                     f"{int((out['status'] == 0).sum())} of {len(out)} verify — the wrapping changed the signed body)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
