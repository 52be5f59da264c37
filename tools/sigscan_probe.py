"""Time the DKIM-Signature scan and the key selection against the front end they are built from and the host loop they replace
(not bench.py: nothing here is a threshold).

  (s) sigscan_kernel alone         — zke_scan_signatures over the configs[1] shape (1 024 e-mails, 4 KB body) and c3's 4 096; device
                                     time from the engine's HIP events (zke_set_timing; zke_timings.front_end_us is the scan launch)
  (f) the verify front end         — zke_verify_emails over the SAME seeded batch, front_end_us (parse_kernel).  `--only f` runs
                                     from a checkout of the parent commit too: that is the figure to put beside (s)
  (e) end to end, the two-signature workload of the chain test (1 024 e-mails, a foreign signature first, 16 keys), host clock
      around the synchronous calls, e-mails in pageable memory:
        zke_scan_signatures per batch; zke_select_keys per batch; zke_verify_emails over the same (e-mail, key) entries;
        the host loop the scan replaces — tests/sigscan_model.py, one core: the only statement of that loop this repository has,
        Python, a lower bound on nothing.
Medians and [10th .. 90th percentile] over --steps batches after --warmup.

    python tools/sigscan_probe.py --out profiles/sigscan_probe.txt
"""
import argparse
import os
import pickle
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"c2": dict(n=1024, body_len=4096, rsa_bits=2048, n_keys=16), "c3": dict(n=4096, body_len=4096, rsa_bits=2048, n_keys=16)}


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[-(len(xs) // 10) - 1]


def fmt(t):
    return f"{t[0]:9.1f} us [{t[1]:.1f} .. {t[2]:.1f}]"


def cached(cache, name, make):
    """Pickled workloads (signing thousands of e-mails takes minutes).  Pickles are code: point --cache only at a directory this
    tool itself has filled."""
    pkl = os.path.join(cache, name + ".pkl") if cache else None
    if pkl and os.path.exists(pkl):
        with open(pkl, "rb") as f:
            return pickle.load(f)
    v = make()
    if pkl:
        os.makedirs(cache, exist_ok=True)
        with open(pkl, "wb") as f:
            pickle.dump(v, f)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="sfe", help='legs to run; "" fills the workload cache without a GPU')
    ap.add_argument("--out", default=None)
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A
    lines = [f"sigscan_probe: steps={args.steps} warmup={args.warmup} only={args.only}"]
    eng = z.Engine() if args.only else None
    if eng:
        eng.set_timing(True)

    def device(call, field="front_end_us"):
        xs = []
        for k in range(args.warmup + args.steps):
            call()
            if k >= args.warmup:
                xs.append(eng.timings()[field])
        return med(xs)

    def wall(call):
        xs = []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            call()
            if k >= args.warmup:
                xs.append((time.perf_counter() - t0) * 1e6)
        return med(xs)

    for name, cfg in SHAPES.items():
        emails = cached(args.cache, f"sigscan_{name}", lambda: synth.make_workload(name, seed=2, **cfg).emails)
        if not eng:
            continue
        raw_total = sum(len(e.raw_email) for e in emails)
        eng.reserve(cfg["n"], raw_total, 1, 0)
        eng.reserve_host(cfg["n"], raw_total + 1024 * cfg["n"])
        lines.append(f"{name}: n={cfg['n']} raw={raw_total} bytes, one DKIM-Signature per e-mail")
        if "s" in args.only:
            refs = eng._scan_refs([e.raw_email for e in emails], [e.from_domain for e in emails])
            from zkemail_rs_amd.engine import _ScanBuffers
            import ctypes as C
            b = _ScanBuffers(refs.n, 8, 32 * refs.n * 8)

            def scan():
                rc = eng.lib.zke_scan_signatures(eng.h, refs.arr, refs.n, 8, C.byref(b.c))
                assert rc == 0, rc
            scan()
            assert int(b.status[:, 3].sum()) == cfg["n"], "every e-mail of the workload has one candidate"
            lines.append(f"  (s) sigscan_kernel (max_sigs 8)   {fmt(device(scan))}   d2h {fmt(device(scan, 'd2h_us'))}")
        if "f" in args.only:
            refs = A.EmailRefs(emails)
            lines.append(f"  (f) parse_kernel (front_end_us)   {fmt(device(lambda: eng.verify_emails(refs)))}")
    if "e" in args.only or not eng:
        import sigscan_inputs as I
        doms, raws, resolver, unsigned = cached(args.cache, "sigscan_chain", lambda: I.chain_workload())
        if eng:
            import sigscan_model as M
            scans = eng.scan_signatures(raws, doms, 8)
            cands = [[resolver.get((d, s.selector)) for s in sc.sigs if s.code == 0] for d, sc in zip(doms, scans)]
            probe = A.EmailRefs([A.Email(d, r, A.PublicKey(b"")) for d, r in zip(doms, raws)])
            pairs = A.EmailRefs([A.Email(d, r, k) for d, r, ks in zip(doms, raws, cands) for k in ks])
            lines.append(f"chain: n={len(raws)} e-mails, two DKIM-Signature headers each (the first from another domain), {len(unsigned)} unsigned, "
                         f"{pairs.n} (e-mail, key) entries; host clock around the synchronous call")
            lines.append(f"  (e) zke_scan_signatures           {fmt(wall(lambda: eng.scan_signatures(raws, doms, 8)))}   (with the Python wrapper's packing and unpacking)")
            refs = eng._scan_refs(raws, doms)
            from zkemail_rs_amd.engine import _ScanBuffers
            import ctypes as C
            b = _ScanBuffers(refs.n, 8, 32 * refs.n * 8)
            lines.append(f"      ... the C call alone            {fmt(wall(lambda: eng.lib.zke_scan_signatures(eng.h, refs.arr, refs.n, 8, C.byref(b.c))))}")
            lines.append(f"  (e) zke_select_keys               {fmt(wall(lambda: eng.select_keys(probe, cands)))}")
            lines.append(f"  (e) zke_verify_emails, same pairs {fmt(wall(lambda: eng.verify_emails(pairs)))}")
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                M.scan(raws, doms, 8)
                dt = (time.perf_counter() - t0) * 1e6
                best = dt if best is None else min(best, dt)
            lines.append(f"  (e) host loop: the Python scan model   {best:9.1f} us wall, one core (best of 3; the only statement of that loop here, a lower bound on nothing)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
