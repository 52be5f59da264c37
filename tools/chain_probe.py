#!/usr/bin/env python
"""chain_probe.py [--body N] [--reps K]: the two dependency chains of the hash / modexp launch, each where the other cannot mask it.

Run under `rocprofv3 --kernel-trace --stats` (a run of its own); the kernel summary then holds
  * sha256_pair_kernel: 1 024 messages of --body bytes through zke_sha256_batch (16 groups, nothing else in the launch): the SHA-256
    chain alone, (body + 9 + 63) / 64 blocks;
  * hash_modexp_kernel: 1 024 RSA-2048 e-mails with --body byte bodies through the device entry, one slot, one batch at a time.  With
    --body 64 the SHA-256 chain is 2 blocks (the header preimage is the longer message, some 14 blocks) and the launch lasts as
    long as the RSA chain: 18 Montgomery products; with --body 4096 it is the launch of the benchmark, alone.
The RSA role is the engine's choice, or ZKE_RSA_OCT9=0 / 1 in the environment; ZKE_LIB picks the build (tools/build_variant.sh).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--body", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sha-only", action="store_true", help="the zke_sha256_batch launches only")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")
    import bench
    import synth
    import zkemail_rs_amd as z
    from zkemail_rs_amd import _abi as A

    eng = z.Engine(device=0, slots=1)
    rng = np.random.default_rng(1)
    msgs = [rng.integers(0, 256, args.body, dtype=np.uint8).tobytes() for _ in range(1024)]
    for _ in range(args.reps):
        eng.sha256_batch(msgs)
    if args.sha_only:
        print(f"chain_probe: body {args.body}, {args.reps} reps, SHA-256 only")
        eng.close()
        return
    wl = synth.make_workload("probe", 1024, args.body, rsa_bits=2048, n_keys=16, seed=11)
    packed = A.PackedBatch(wl.emails)
    dev = torch.device("cuda", 0)
    cb, keep, totals = bench.device_batch(torch, packed, dev)
    eng.reserve(packed.n, totals[0], 1, 0)
    out = torch.zeros(packed.n * 192, dtype=torch.uint8, device=dev)
    for _ in range(args.reps + 2):                     # the first batch fills the key cache: the one-signature-per-wave routine
        eng.verify_batch_device(cb, totals[0], totals[1], totals[2], out.data_ptr(), 0)
        eng.sync()
    rec = out.cpu().numpy().view(A.RESULT_DTYPE)
    ok = int((rec["status"] == 0).sum())
    print(f"chain_probe: body {args.body}, {args.reps} reps, {ok} of {packed.n} verified")
    eng.close()
    if ok != packed.n:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
