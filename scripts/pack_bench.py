#!/usr/bin/env python3
"""Times the LWE -> TLWE packing key switch (tfhe_amd_pack_dev) in one process.

  python scripts/pack_bench.py [--out profiles/pack.jsonl] [--runs 7]

Configurations (T outputs of P inputs each, device-resident arrays of random words):
  (1, 1024)        one output, its key rows split over the most workgroups
  (16, 1024)       split form, 2 x compute units workgroups in all
  (256, 1024)      split in two on a 256-CU device
  (1, 16)          a small pack: the cost does not depend on P beyond the digit pass
  (CUs + 1, 1024)  the first T in the unsplit form: every workgroup runs one output's 750 group steps
                   in series, which is what T = 1 would cost without the split
After two warm-up calls per configuration the configurations alternate, `runs` rounds; each figure
is the wall time around a stream synchronize.  One JSON line per configuration: median, min, max
in ms, the kernels the call launched, group steps (750 per output) and the median per group step.
The first output of every configuration is checked against tests/pack_oracle.py once."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-gpu-tfhe_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import tfhe_amd as T  # noqa: E402

N, n_lwe = 1024, 500
GROUPS = 750


def main():
    import torch
    import pack_oracle as PO
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pack.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()

    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    rng = np.random.default_rng(37)
    words = rng.integers(-2**31, 2**31, (n_lwe, 6, 2, N), dtype=np.int64).astype(np.int32)
    pkey = ctx.pack_key_import(words)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)

    configs = []
    for T_, P in ((1, N), (16, N), (256, N), (1, 16), (cus + 1, N)):
        in_a = torch.randint(-2**31, 2**31 - 1, (T_, P, n_lwe), dtype=torch.int32, device="cuda")
        in_b = torch.randint(-2**31, 2**31 - 1, (T_, P), dtype=torch.int32, device="cuda")
        out = torch.zeros((T_, 2, N), dtype=torch.int32, device="cuda")

        def run(in_a=in_a, in_b=in_b, out=out):
            ctx.pack_dev(pkey, in_a, in_b, out)
            ctx.sync()
        configs.append(dict(T=T_, P=P, run=run, in_a=in_a, in_b=in_b, out=out))
    torch.cuda.synchronize()

    for c in configs:
        c["run"]()
        c["run"]()
        c["kernels"] = ctx.last_kernels()
        want = PO.pack_rows(words, c["in_a"][:1].cpu().numpy(), c["in_b"][:1].cpu().numpy())
        assert np.array_equal(c["out"][:1].cpu().numpy(), want), (c["T"], c["P"])
    times = {id(c): [] for c in configs}
    for _ in range(args.runs):
        for c in configs:
            t0 = time.perf_counter()
            c["run"]()
            times[id(c)].append((time.perf_counter() - t0) * 1e3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for c in configs:
            t = sorted(times[id(c)])
            med = t[len(t) // 2]
            rec = dict(T=c["T"], P=c["P"], runs=len(t), median_ms=round(med, 4), min_ms=round(t[0], 4),
                       max_ms=round(t[-1], 4), kernels=c["kernels"], group_steps=GROUPS * c["T"],
                       us_per_group_step=round(med * 1e3 / (GROUPS * c["T"]), 4),
                       us_per_output=round(med * 1e3 / c["T"], 2), compute_units=cus, version=T.version())
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))
    pkey.close()
    ctx.close()
    K.close()


if __name__ == "__main__":
    main()
