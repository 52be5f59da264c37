"""Time the mapped capture extraction against the plain one, and the plain one against the parent commit's (not bench.py: nothing
here is a threshold).

On the c5re shape (2 048 e-mails, RSA-4096, QP soft breaks, 2 + 2 parts), interleaved step by step in ONE process on one GPU:
  (m) zke_extract_captures_mapped of this build     — the extraction plus capture_origin_kernel and its copy back
  (p) zke_extract_captures of this build            — must run the kernels it ran before
  (q) zke_extract_captures of --parent-lib          — a libzkemail_amd.so built from the parent commit (python -m zkemail_rs_amd.build
                                                      in a checkout of it); left out when the option is absent
Device time from the engine's HIP events (zke_set_timing: first launch to last launch, copies excluded), median and 10th / 90th
percentile over --steps rounds after --warmup.  The origin launch's own time is the median over the rounds of (m) - (p) of the
regex stage + capture mark (it is the only launch the two differ by), shown beside regex_prep_kernel's (the QP pass it should
cost on the order of).

    python tools/qp_origin_probe.py --parent-lib ../parent/zkemail.rs_amd/libzkemail_amd.so --out profiles/qp_origin_probe.txt
"""
import argparse
import ctypes as C
import os
import pickle
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = dict(n=2048, body_len=4096, rsa_bits=4096, n_keys=16, n_header_parts=2, n_body_parts=2, qp_frac=0.05)


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[len(xs) // 10], xs[-(len(xs) // 10) - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="batch size multiplier (a quick look: 0.125)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cache", default=None, help="directory of pickled workloads (written when missing; as tools/capture_probe.py: point it only at a "
                                                  "directory this tool or that one has filled)")
    ap.add_argument("--fill-cache", action="store_true", help="sign the workload into --cache and stop: no GPU needed")
    args = ap.parse_args()
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A
    from zkemail_rs_amd import engine as E
    from zkemail_rs_amd import regex_compile as rc

    cfg = dict(SHAPE, n=max(16, int(SHAPE["n"] * args.scale)))
    pkl = os.path.join(args.cache, f"c5re_{cfg['n']}.pkl") if args.cache else None
    if pkl and os.path.exists(pkl):
        with open(pkl, "rb") as f:
            inputs, wl = pickle.load(f)
    else:
        inputs, wl, _ = synth.make_regex_workload("c5re", seed=1000, **cfg)
        if pkl:
            os.makedirs(args.cache, exist_ok=True)
            with open(pkl, "wb") as f:
                pickle.dump((inputs, wl), f)
    if args.fill_cache:
        return
    emails = [i.email for i in inputs]
    raw_total = sum(len(e.raw_email) for e in emails)
    refs = A.EmailRefs(emails)
    rcfg = rc.RegexConfig([rc.RegexPattern(p, ci) for p, ci in synth.HEADER_PATTERNS[:2]], [rc.RegexPattern(p, ci) for p, ci in synth.BODY_PATTERNS[:2]])

    class LibEngine(z.Engine):
        """An engine of another build of the library, loaded beside this tree's."""
        def __init__(self, path):
            self.lib = E.load_library(path)
            opt = A.zke_options()
            opt.device = -1
            self.options, self.h = opt, C.c_void_p()
            self._check(self.lib.zke_engine_create(C.byref(opt), C.byref(self.h)), "zke_engine_create")
            self._dfa_cache, self._capture_cache, self._pattern_cache = {}, {}, {}

    engines = {"child": z.Engine()}
    if args.parent_lib:
        engines["parent"] = LibEngine(os.path.abspath(args.parent_lib))
    for eng in engines.values():
        eng.set_timing(True)
        eng.reserve(cfg["n"], raw_total, 1, 4)
        eng.reserve_host(cfg["n"], raw_total + 1024 * cfg["n"])
    legs = [("m", "child", True), ("p", "child", False)] + ([("q", "parent", False)] if args.parent_lib else [])
    rec = {k: dict(total=[], stage=[], prep=[]) for k, _, _ in legs}
    first = {}
    for step in range(args.warmup + args.steps):
        for k, who, mapped in legs:
            eng = engines[who]
            res = eng.extract_captures(refs, rcfg, unicode=False, origins=True) if mapped else eng.extract_captures(refs, rcfg, unicode=False)
            t = eng.timings()
            if step == 0:
                first[k] = res
            if step >= args.warmup:
                rec[k]["total"].append(t["total_us"]); rec[k]["stage"].append(t["regex_prep_us"] + t["dfa_us"]); rec[k]["prep"].append(t["regex_prep_us"])
    # faster and different is not faster: the three legs deliver the same records and strings
    for k in first:
        assert first[k][0].tobytes() == first["p"][0].tobytes() and first[k][1] == first["p"][1], k
    ok = int((first["p"][0]["status"] == 0).sum())
    flags = first["m"][2][1]
    names = {"m": "zke_extract_captures_mapped (this build)", "p": "zke_extract_captures        (this build)", "q": "zke_extract_captures        (parent)    "}
    lines = [f"qp_origin_probe: c5re n={cfg['n']} parts=2+2 raw={raw_total} bytes steps={args.steps} warmup={args.warmup} ({ok} e-mails OK; "
             f"origins: {int((flags == A.ORGF_SPLIT).sum())} SPLIT, {int((flags == A.ORGF_PADDING).sum())} PADDING of {flags.size})"]
    for k, _, _ in legs:
        (t, lo, hi), (d, dlo, dhi) = med(rec[k]["total"]), med(rec[k]["stage"])
        lines.append(f"  ({k}) {names[k]}  total {t:9.1f} us [{lo:.1f} .. {hi:.1f}]   regex stage + capture {d:8.1f} us [{dlo:.1f} .. {dhi:.1f}]")
    own = med([a - b for a, b in zip(rec["m"]["stage"], rec["p"]["stage"])])
    prep = med(rec["p"]["prep"])
    lines.append(f"  origin launch, (m) - (p) per round          {own[0]:9.1f} us [{own[1]:.1f} .. {own[2]:.1f}]   regex_prep_kernel (p) {prep[0]:8.1f} us [{prep[1]:.1f} .. {prep[2]:.1f}]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
