"""Time the key-record decode and the selection from records against the route they replace (not bench.py: nothing here is a
threshold).  The batch is the two-signature workload of tools/sigscan_probe.py's leg (e): 1 024 e-mails, a foreign signature
first, 16 RSA-2048 keys; every candidate's key is answered as the TXT record a resolver returns ("v=DKIM1; k=rsa; p=<base64 of the
SubjectPublicKeyInfo>", 410 characters).

  (k) keyrec_kernel alone           — zke_decode_key_records over the batch's candidate records; device time from the engine's HIP
                                      events (zke_set_timing; zke_timings.front_end_us is the decode launch), and the host clock
                                      around the synchronous C call
  (r) zke_select_keys_from_records  — host clock around the synchronous call: records in, selection out; front_end_us is then the
                                      verify front end, total_us the batch's launches with the three key-record launches in front
  (p) the parent's route            — decode on the host, then zke_select_keys: host clock around both.  The host decode is
                                      tests/keyrec_model.py, one core: the only statement of that step this repository has, Python,
                                      a lower bound on nothing; the zke_select_keys part is given on its own beside it
Medians and [10th .. 90th percentile] over --steps batches after --warmup.

    python tools/keyrec_probe.py --out profiles/keyrec_probe.txt
"""
import argparse
import ctypes as C
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import keyrec_cases as K
    import keyrec_model as KM
    import sigscan_inputs as I
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A
    from zkemail_rs_amd.engine import _KeyrecBuffers

    eng = z.Engine()
    eng.set_timing(True)

    def timed(call, fields=()):
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

    doms, raws, resolver, unsigned = I.chain_workload(n=args.n)
    records = {k: b"v=DKIM1; k=rsa; p=" + K.b64(K.spki_wrap(v.key)) for k, v in resolver.items()}
    scans = eng.scan_signatures(raws, doms, 8)
    rec_rows = [[records.get((d, s.selector)) for s in sc.sigs if s.code == 0] for d, sc in zip(doms, scans)]
    flat = [r for row in rec_rows for r in row]
    probe = A.EmailRefs([A.Email(d, r, A.PublicKey(b"")) for d, r in zip(doms, raws)])
    lines = [f"keyrec_probe: steps={args.steps} warmup={args.warmup}",
             f"chain: n={len(raws)} e-mails, two DKIM-Signature headers each (the first from another domain), {len(unsigned)} unsigned, "
             f"{len(flat)} candidate records of {len(flat[0])} bytes (RSA-2048 SubjectPublicKeyInfo)"]

    # (k) the decode alone
    b = _KeyrecBuffers(flat)

    def decode():
        rc = eng.lib.zke_decode_key_records(eng.h, b.arr, b.m, A.KEYREC_DNS, C.byref(b.c))
        assert rc == 0, rc
    decode()
    assert all(int(c) == 0 for c in b.infos["code"][:b.m]), "every record of the workload decodes"
    w, d = timed(decode, ("front_end_us", "h2d_us", "d2h_us"))
    lines.append(f"  (k) keyrec_kernel (front_end_us)        {fmt(d['front_end_us'])}   h2d {fmt(d['h2d_us'])}   d2h {fmt(d['d2h_us'])}")
    lines.append(f"      zke_decode_key_records, the C call  {fmt(w)}   host clock")

    # (r) selection from records
    got = eng.select_keys_from_records(probe, rec_rows, A.KEYREC_DNS)
    w, d = timed(lambda: eng.select_keys_from_records(probe, rec_rows, A.KEYREC_DNS), ("front_end_us", "total_us"))
    lines.append(f"  (r) zke_select_keys_from_records        {fmt(w)}   host clock; launches first to last {fmt(d['total_us'])}, of which parse_kernel {fmt(d['front_end_us'])}")

    # (p) the parent's route: the host decodes, then zke_select_keys
    def parent():
        rows = [[KM.public_key(KM.decode(r, KM.DNS)) if r else None for r in row] for row in rec_rows]
        return eng.select_keys(probe, rows)
    want = parent()
    assert got[0].tobytes() == want[0].tobytes() and list(got[1]) == list(want[1]), "both routes select alike"
    key_rows = [[KM.public_key(KM.decode(r, KM.DNS)) if r else None for r in row] for row in rec_rows]
    w_sel, d_sel = timed(lambda: eng.select_keys(probe, key_rows), ("front_end_us", "total_us"))
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        [[KM.decode(r, KM.DNS) for r in row if r] for row in rec_rows]
        dt = (time.perf_counter() - t0) * 1e6
        best = dt if best is None else min(best, dt)
    lines.append(f"  (p) zke_select_keys, keys decoded       {fmt(w_sel)}   host clock; launches first to last {fmt(d_sel['total_us'])}, of which parse_kernel {fmt(d_sel['front_end_us'])}")
    lines.append(f"      + the host decode in front of it    {best:9.1f} us wall, one core (best of 3; the Python model: the only statement of that step here, a lower bound on nothing)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
