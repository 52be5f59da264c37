"""Time zke_verify_emails_encoded against the plain entry and against the host loop it replaces (not bench.py: nothing here is a
threshold).  Two batches:

  c2   BASELINE configs[1]'s shape: 1 024 DKIM-signed e-mails, 4 KB of body, RSA-2048, TWO external inputs each; verify_email (kind 0)
  c3   configs[2]'s shape: 4 096 e-mails, 2 header parts with one capture each; verify_email_with_regex (kind 1)

Per batch, three calls, interleaved round by round after a warm-up, each synchronous (the device is idle when the clock stops), the
median over the rounds:

  (a) zke_verify_emails_encoded                  records + encodings + digests, one call
  (b) the plain entry of the same batch          zke_verify_emails / zke_verify_emails_with_regex: records only
  (c) the way to the same product without (a)    (b), then ONE thread walks the records: zke_abi_encode per e-mail (the pointer tables
                                                 of its strings are built once, outside the clock) and hashlib.sha256 of the bytes

Every round of (a) is compared with (c)'s product first.  `--trace` runs (a) alone `--steps` times and prints nothing else: the run to
put under `rocprofv3 --kernel-trace --stats` (tools/kernel_medians.py reads the trace: encode_outputs_kernel and the sha256 kernel
behind it, which in this run hashes nothing else).

    python tools/encode_probe.py --out profiles/encode_probe.txt
"""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[-(len(xs) // 10) - 1]


def fmt(t):
    return f"{t[0]:9.1f} us [{t[1]:.1f} .. {t[2]:.1f}]"


class HostLoop:
    """(c)'s second half: per e-mail the pointer tables zke_abi_encode takes, built once; run(records) encodes and hashes every
    ZKE_OK record on the calling thread."""

    def __init__(self, lib, strings, matches):
        self.lib = lib
        self.items = []
        for ext, m in zip(strings, matches):
            self.items.append((self._table(ext), self._table(m or []), 0 if m is None else 1))
        self.buf = np.zeros(1 << 16, np.uint8)
        self.need = C.c_size_t()

    @staticmethod
    def _table(strs):
        bs = [s.encode("utf-8") for s in strs]
        bufs = [np.frombuffer(b or b"\0", np.uint8) for b in bs]
        return (bufs, (C.c_void_p * max(len(bs), 1))(*[x.ctypes.data for x in bufs]), (C.c_size_t * max(len(bs), 1))(*[len(b) for b in bs]), len(bs))

    def run(self, records):
        out = []
        base, step = records.ctypes.data, records.dtype.itemsize
        fd, pk = records.dtype.fields["from_domain_hash"][1], records.dtype.fields["public_key_hash"][1]
        status = records["status"]
        for i, ((_, p1, l1, n1), (_, p2, l2, n2), wm) in enumerate(self.items):
            if status[i]:
                out.append((b"", b"\0" * 32))
                continue
            rc = self.lib.zke_abi_encode(base + i * step + fd, base + i * step + pk, p1, l1, n1, wm, p2, l2, n2, self.buf.ctypes.data, self.buf.size, C.byref(self.need))
            assert rc == 0, rc
            b = self.buf[:self.need.value].tobytes()
            out.append((b, hashlib.sha256(b).digest()))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="c2,c3")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A
    from zkemail_rs_amd.engine import regex_matches_of

    eng = z.Engine()
    lines = [f"encode_probe: steps={args.steps} warmup={args.warmup} (one engine, one slot; medians [10th .. 90th percentile]; host clock around synchronous calls)"]
    for shape in args.shape.split(","):
        if shape == "c2":
            wl = synth.make_workload("c2", 1024, 4096, rsa_bits=2048, n_keys=16, seed=4242)
            inputs = wl.emails
            for i, e in enumerate(inputs):
                e.external_inputs = [A.ExternalInput("address", "0x%040x" % (i * 104729)), A.ExternalInput("nonce", "%d" % (i * 7919))]
            form, what = "plain", "1 024 e-mails, 4 KB bodies, RSA-2048, two external inputs each; verify_email, kind 0"
        else:
            inputs, _, _ = synth.make_regex_workload("c3", 4096, 4096, rsa_bits=2048, n_keys=16, seed=4243, n_header_parts=2, n_body_parts=0)
            form, what = "lists", "4 096 e-mails, 4 KB bodies, RSA-2048, 2 header parts with one capture each; verify_email_with_regex, kind 1"
        emails = [i if isinstance(i, A.Email) else i.email for i in inputs]
        n = len(inputs)
        call = eng._encoded_call(inputs, form, None, None)
        plain_out = np.zeros(n, A.RESULT_DTYPE)

        def run_a():
            rc = eng.lib.zke_verify_emails_encoded(eng.h, call.refs.arr, n, C.byref(call.c), call.out.ctypes.data, C.byref(call.enc.c))
            assert rc == 0, rc

        def run_b():
            if form == "plain":
                rc = eng.lib.zke_verify_emails(eng.h, call.refs.arr, n, plain_out.ctypes.data)
            else:
                rc = eng.lib.zke_verify_emails_with_regex(eng.h, call.refs.arr, n, call.c.lists, plain_out.ctypes.data)
            assert rc == 0, rc

        if args.trace:
            for _ in range(args.steps):
                run_a()
            continue
        loop = HostLoop(eng.lib, [A.flat_external_inputs(e.external_inputs) for e in emails],
                        [None if form == "plain" else regex_matches_of(i) for i in inputs])
        ta, tb, tc = [], [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter(); run_a(); t1 = time.perf_counter()
            run_b(); t2 = time.perf_counter()
            run_b(); product = loop.run(plain_out); t3 = time.perf_counter()
            assert call.records.tobytes() == plain_out.tobytes() and call.enc.result() == product, "(a) and (c) give the same product"
            if k >= args.warmup:
                ta.append((t1 - t0) * 1e6); tb.append((t2 - t1) * 1e6); tc.append((t3 - t2) * 1e6)
        ok = int((plain_out["status"] == 0).sum())
        ret = (n * 48 + int(call.enc.c.bytes_need)) / n
        lines += [f"{shape}: {what}",
                  f"    {ok} of {n} encoded; {int(call.enc.c.bytes_need) / n:.0f} B of encoding + 48 B of info = {ret:.0f} B returned per e-mail beside its 192-byte record",
                  f"    (a) zke_verify_emails_encoded               {fmt(med(ta))}",
                  f"    (b) the plain entry                         {fmt(med(tb))}",
                  f"    (c) (b) + zke_abi_encode + hashlib.sha256   {fmt(med(tc))}   (one thread, a Python loop over ctypes: {(med(tc)[0] - med(tb)[0]) / n:.2f} us per e-mail on top of (b))",
                  f"    (a) - (b) = {med(ta)[0] - med(tb)[0]:.1f} us for the batch; (c) / (a) = {med(tc)[0] / med(ta)[0]:.2f}"]
    if args.trace:
        return
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
