"""Time the capture extraction against the verification it feeds and the host loop it replaces (not bench.py: nothing here
is a threshold).

For the c3 shape (4 096 e-mails, 2 header parts) and the c5re shape (2 048 e-mails, RSA-4096, QP soft breaks, 2 + 2 parts):
  (a) zke_extract_captures per batch               — raw e-mails + keys + patterns in, RegexInfo tables out
  (b) zke_verify_emails_with_regex per batch       — the same e-mails with synth's capture strings
  (c) the host loop (a) replaces                   — re.search over the signer's canonical header / cleaned body per
                                                     e-mail, one core (the canonicalisation itself is NOT counted: the
                                                     signer already had it, so this is a lower bound)
(a) and (b) are device time from the engine's HIP events (zke_set_timing: first launch to last launch, copies excluded), median
and spread over --steps batches after --warmup; (c) is wall time.  `--only b` measures (b) alone — run that way from a
checkout of the parent commit to compare the existing path before and after.

    python tools/capture_probe.py --out profiles/captures_probe.txt
"""
import argparse
import os
import pickle
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {
    "c3": dict(n=4096, body_len=4096, rsa_bits=2048, n_keys=16, n_header_parts=2, n_body_parts=0),
    "c5re": dict(n=2048, body_len=4096, rsa_bits=4096, n_keys=16, n_header_parts=2, n_body_parts=2, qp_frac=0.05),
}


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[-(len(xs) // 10) - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (a quick look: 0.125)")
    ap.add_argument("--only", default="abc")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cache", default=None, help="directory of pickled workloads (written when missing): signing 6 144 e-mails takes minutes.  Pickles are code: "
                         "point this only at a directory this tool itself has filled")
    args = ap.parse_args()
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import regex_compile as rc
    lines = [f"capture_probe: {z.Engine.__module__} steps={args.steps} warmup={args.warmup} scale={args.scale} only={args.only}"]
    eng = z.Engine() if args.only else None          # --only "": fill the workload cache, no GPU
    if eng:
        eng.set_timing(True)
    for name, cfg in SHAPES.items():
        cfg = dict(cfg, n=max(16, int(cfg["n"] * args.scale)))
        pkl = os.path.join(args.cache, f"{name}_{cfg['n']}.pkl") if args.cache else None
        if pkl and os.path.exists(pkl):
            with open(pkl, "rb") as f:
                inputs, wl = pickle.load(f)
        else:
            inputs, wl, _ = synth.make_regex_workload(name, seed=1000, **cfg)
            if pkl:
                os.makedirs(args.cache, exist_ok=True)
                with open(pkl, "wb") as f:
                    pickle.dump((inputs, wl), f)
        if args.only == "":
            continue
        emails = [i.email for i in inputs]
        raw_total = sum(len(e.raw_email) for e in emails)
        P = cfg["n_header_parts"] + cfg["n_body_parts"]
        eng.reserve(cfg["n"], raw_total, 1, P)
        eng.reserve_host(cfg["n"], raw_total + 1024 * cfg["n"])
        lines.append(f"{name}: n={cfg['n']} parts={cfg['n_header_parts']}+{cfg['n_body_parts']} raw={raw_total} bytes")

        def timed(call):
            tot, dfa = [], []
            for k in range(args.warmup + args.steps):
                call()
                t = eng.timings()
                if k >= args.warmup:
                    tot.append(t["total_us"]); dfa.append(t["regex_prep_us"] + t["dfa_us"])
            return med(tot), med(dfa)

        if "a" in args.only:
            rcfg = rc.RegexConfig([rc.RegexPattern(p, ci) for p, ci in synth.HEADER_PATTERNS[:cfg["n_header_parts"]]] or None,
                                  [rc.RegexPattern(p, ci) for p, ci in synth.BODY_PATTERNS[:cfg["n_body_parts"]]] or None)
            refs = z._abi.EmailRefs(emails)
            records, infos = eng.extract_captures(refs, rcfg, unicode=False)
            ok = int((records["status"] == 0).sum())
            (t, lo, hi), (d, dlo, dhi) = timed(lambda: eng.extract_captures(refs, rcfg, unicode=False))
            lines.append(f"  (a) zke_extract_captures          total {t:9.1f} us [{lo:.1f} .. {hi:.1f}]   regex stage + capture {d:8.1f} us [{dlo:.1f} .. {dhi:.1f}]   "
                         f"({ok} of {cfg['n']} e-mails OK, {cfg['n'] / t:.2f} M e-mails/s)")
        if "b" in args.only:
            (t, lo, hi), (d, dlo, dhi) = timed(lambda: eng.verify_emails_with_regex(inputs))
            lines.append(f"  (b) zke_verify_emails_with_regex  total {t:9.1f} us [{lo:.1f} .. {hi:.1f}]   regex stage           {d:8.1f} us [{dlo:.1f} .. {dhi:.1f}]")
        if "c" in args.only:
            hrx = [re.compile(p.encode()) for p, _ in synth.HEADER_PATTERNS[:cfg["n_header_parts"]]]
            brx = [re.compile(p.encode()) for p, _ in synth.BODY_PATTERNS[:cfg["n_body_parts"]]]
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                for it in wl.inter:
                    for rx in hrx:
                        m = rx.search(it["canon_header"])
                        _ = m and m.groups()
                    for rx in brx:
                        m = rx.search(it["clean_body"])
                        _ = m and m.groups()
                dt = (time.perf_counter() - t0) * 1e6
                best = dt if best is None else min(best, dt)
            lines.append(f"  (c) host loop, re.search per e-mail     {best:9.1f} us wall, one core (best of 3; canonicalisation not counted)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
