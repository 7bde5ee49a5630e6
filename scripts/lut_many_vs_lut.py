"""Many-LUT against single-table blind rotation and bootstrap.

One process, one context.  At each batch size it warms the single-table forms
(tfhe_amd_bootstrap_lut_woks_batch_dev / _batch_dev, a random table) and the many-LUT forms
(theta = 1, n_out = 2, a random table), then alternates timed launches:
  1. blind rotation: the `lut-many` launch against the `lut` launch, each launch's blind-rotation
     time (the fp64 kernel and the guard's launch, HIP events on the stream) through
     tfhe_amd_profile_read; the yardstick is the single-table series' own spread;
  2. end to end: ONE key-switched many-LUT call (two functions) against TWO key-switched
     single-table calls, wall time around a stream synchronisation.
Prints per batch size all series, their medians and the ratios.

    python scripts/lut_many_vs_lut.py [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-gpu-tfhe_amd"))

THETA, N_OUT = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tfhe_amd as T

    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    rng = np.random.default_rng(43)
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def r4(v):
        return [round(x, 4) for x in v]

    emit({"what": "lut_many_vs_lut", "version": T.version(), "device": torch.cuda.get_device_name(0),
          "reps": args.reps, "theta": THETA, "n_out": N_OUT})
    for B in args.batches:
        x_a = torch.from_numpy(rng.integers(-2**31, 2**31, (B, T.n_lwe), dtype=np.int64).astype(np.int32)).cuda()
        x_b = torch.from_numpy(rng.integers(-2**31, 2**31, B, dtype=np.int64).astype(np.int32)).cuda()
        tv = torch.from_numpy(rng.integers(-2**31, 2**31, (1, T.N), dtype=np.int64).astype(np.int32)).cuda()
        u_a = torch.zeros((N_OUT, B, T.N), dtype=torch.int32, device="cuda")
        u_b = torch.zeros((N_OUT, B), dtype=torch.int32, device="cuda")
        r_a = torch.zeros((N_OUT, B, T.n_lwe), dtype=torch.int32, device="cuda")
        r_b = torch.zeros((N_OUT, B), dtype=torch.int32, device="cuda")

        def lut():
            ctx.lut_woks_dev(tv, u_a[0], u_b[0], x_a, x_b)
            return ctx.last_kernels()

        def many():
            ctx.lut_many_woks_dev(tv, THETA, N_OUT, u_a, u_b, x_a, x_b)
            return ctx.last_kernels()

        def lut_twice():
            for f in range(N_OUT):
                ctx.lut_bootstrap_dev(tv, r_a[f], r_b[f], x_a, x_b)

        def many_once():
            ctx.lut_many_bootstrap_dev(tv, THETA, N_OUT, r_a, r_b, x_a, x_b)

        def br_ms(fn):
            ctx.profile_enable(True)
            fn()
            ctx.sync()
            ms = ctx.profile_read()["br_ms"]
            ctx.profile_enable(False)
            return ms

        def wall_ms(fn):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3

        kern = {}
        for _ in range(2):
            kern["lut"] = lut()
            kern["many"] = many()
            lut_twice()
            many_once()
        ctx.sync()
        br = {"lut": [], "many": []}
        for _ in range(args.reps):
            br["lut"].append(br_ms(lut))
            br["many"].append(br_ms(many))
        e2e = {"lut_x2": [], "many": []}
        for _ in range(args.reps):
            e2e["lut_x2"].append(wall_ms(lut_twice))
            e2e["many"].append(wall_ms(many_once))
        mb = {k: float(np.median(v)) for k, v in br.items()}
        me = {k: float(np.median(v)) for k, v in e2e.items()}
        emit({"B": B, "kernels": kern, "br_lut_ms": r4(br["lut"]), "br_many_ms": r4(br["many"]),
              "br_lut_median_ms": round(mb["lut"], 4), "br_many_median_ms": round(mb["many"], 4),
              "br_many_over_lut": round(mb["many"] / mb["lut"], 4),
              "br_lut_spread": [round(min(br["lut"]) / mb["lut"], 4), round(max(br["lut"]) / mb["lut"], 4)],
              "e2e_lut_x2_ms": r4(e2e["lut_x2"]), "e2e_many_ms": r4(e2e["many"]),
              "e2e_lut_x2_median_ms": round(me["lut_x2"], 4), "e2e_many_median_ms": round(me["many"], 4),
              "e2e_many_over_lut_x2": round(me["many"] / me["lut_x2"], 4)})
    ctx.close()
    K.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
