#!/usr/bin/env python3
"""Times the p-way selection (tfhe_amd_select_batch_dev) in one process.

  python scripts/select_bench.py [--out profiles/select.jsonl] [--runs 7]

Configurations (device-resident arrays; candidates and pack key of random words, fresh selectors):
  select (B, p) = (1, 4), (256, 4), (1024, 4)   pack + box fill + rotation + key switch
  acc    B = 1024    the bootstrap from encrypted accumulators alone (rotation + key switch)
  lut    B = 1024    one ordinary LUT bootstrap batch (rotation + key switch), for comparison: the
                     selection replaces what bootsMUX does for bits with two such rotation batches
After two warm-up calls per configuration the configurations alternate, `runs` rounds; each figure
is the wall time around a stream synchronize.  One JSON line per configuration: median, min, max in
ms, the kernels the call launched and the median per query.  Query 0 of every configuration is
checked against the oracles of tests/ once."""
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


def main():
    import torch
    import acc_oracle as AO
    import lut_oracle as LO
    import oracle_ctypes as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "select.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()

    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    okey = O.OracleKey(K.bk, K.ksk, use_ntt=True)
    rng = np.random.default_rng(38)
    words = rng.integers(-2**31, 2**31, (n_lwe, 6, 2, N), dtype=np.int64).astype(np.int32)
    pkey = ctx.pack_key_import(words)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    rand = lambda *shape: torch.randint(-2**31, 2**31 - 1, shape, dtype=torch.int32, device="cuda")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    host = lambda t: t.cpu().numpy()

    configs = []
    for B, p in ((1, 4), (256, 4), (1024, 4)):
        cand_a, cand_b = rand(p, B, n_lwe), rand(p, B)
        y = [dev(v) for v in K.encrypt_digits(rng.integers(0, p, B), p, rng)]
        res = (torch.zeros((B, n_lwe), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"))

        def run(cand_a=cand_a, cand_b=cand_b, y=y, res=res):
            ctx.select_dev(pkey, cand_a, cand_b, y[0], y[1], res[0], res[1])
            ctx.sync()

        def want(cand_a=cand_a, cand_b=cand_b, y=y):
            return AO.select(okey, words, host(cand_a[:, :1]), host(cand_b[:, :1]), 0, 1, host(y[0][:1]), host(y[1][:1]))
        configs.append(dict(what="select", B=B, p=p, run=run, res=res, want=want))
    B = 1024
    acc = rand(B, 2, N)
    x = [dev(v) for v in K.encrypt_digits(rng.integers(0, 4, B), 4, rng)]
    res = (torch.zeros((B, n_lwe), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"))

    def run_acc():
        ctx.acc_bootstrap_dev(acc, res[0], res[1], x[0], x[1])
        ctx.sync()
    configs.append(dict(what="acc", B=B, p=None, run=run_acc, res=res,
                        want=lambda: AO.bootstrap_batch(okey, host(acc[:1]), host(x[0][:1]), host(x[1][:1]))))
    tv = rand(1, N)
    res_l = (torch.zeros((B, n_lwe), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"))

    def run_lut():
        ctx.lut_bootstrap_dev(tv, res_l[0], res_l[1], x[0], x[1])
        ctx.sync()
    configs.append(dict(what="lut", B=B, p=None, run=run_lut, res=res_l,
                        want=lambda: LO.bootstrap_batch(okey, host(tv), host(x[0][:1]), host(x[1][:1]))))
    torch.cuda.synchronize()

    for c in configs:
        c["run"]()
        c["run"]()
        c["kernels"] = ctx.last_kernels()
        w = c["want"]()
        assert np.array_equal(host(c["res"][0][:1]), w[0]) and np.array_equal(host(c["res"][1][:1]), w[1]), (c["what"], c["B"])
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
            rec = dict(what=c["what"], B=c["B"], p=c["p"], runs=len(t), median_ms=round(med, 4), min_ms=round(t[0], 4),
                       max_ms=round(t[-1], 4), kernels=c["kernels"], us_per_query=round(med * 1e3 / c["B"], 2),
                       compute_units=cus, version=T.version())
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))
    pkey.close()
    ctx.close()
    K.close()


if __name__ == "__main__":
    main()
