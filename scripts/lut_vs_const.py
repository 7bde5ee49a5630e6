"""LUT against constant blind rotation, kernel time.

One process, one context: warms tfhe_amd_bootstrap_woks_batch_dev (the constant test vector) and
tfhe_amd_bootstrap_lut_woks_batch_dev (a random table) at each batch size, then alternates timed
launches of the two and reads each launch's blind-rotation time (the fp64 kernel and the guard's
launch, HIP events on the stream) through tfhe_amd_profile_read.  Prints per batch size both
series, their medians, the LUT / constant ratio and the constant series' own spread.

    python scripts/lut_vs_const.py [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-gpu-tfhe_amd"))


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
    rng = np.random.default_rng(42)
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit({"what": "lut_vs_const", "version": T.version(), "device": torch.cuda.get_device_name(0), "reps": args.reps})
    for B in args.batches:
        x_a = torch.from_numpy(rng.integers(-2**31, 2**31, (B, T.n_lwe), dtype=np.int64).astype(np.int32)).cuda()
        x_b = torch.from_numpy(rng.integers(-2**31, 2**31, B, dtype=np.int64).astype(np.int32)).cuda()
        tv = torch.from_numpy(rng.integers(-2**31, 2**31, (1, T.N), dtype=np.int64).astype(np.int32)).cuda()
        u_a = torch.zeros((B, T.N), dtype=torch.int32, device="cuda")
        u_b = torch.zeros(B, dtype=torch.int32, device="cuda")

        def const():
            T._check(T.lib.tfhe_amd_bootstrap_woks_batch_dev(ctx.h, B, T.MU, x_a.data_ptr(), x_b.data_ptr(),
                                                             u_a.data_ptr(), u_b.data_ptr(), None), "woks_dev")
            return ctx.last_kernels()

        def lut():
            ctx.lut_woks_dev(tv, u_a, u_b, x_a, x_b)
            return ctx.last_kernels()

        def timed(fn):
            ctx.profile_enable(True)
            fn()
            ctx.sync()
            ms = ctx.profile_read()["br_ms"]
            ctx.profile_enable(False)
            return ms

        kern = {}
        for _ in range(2):
            kern["const"] = const()
            kern["lut"] = lut()
        ctx.sync()
        series = {"const": [], "lut": []}
        for _ in range(args.reps):
            series["const"].append(timed(const))
            series["lut"].append(timed(lut))
        med = {k: float(np.median(v)) for k, v in series.items()}
        cmin, cmax = min(series["const"]), max(series["const"])
        emit({"B": B, "kernels": kern, "const_ms": [round(v, 4) for v in series["const"]],
              "lut_ms": [round(v, 4) for v in series["lut"]], "const_median_ms": round(med["const"], 4),
              "lut_median_ms": round(med["lut"], 4), "lut_over_const": round(med["lut"] / med["const"], 4),
              "const_spread": [round(cmin / med["const"], 4), round(cmax / med["const"], 4)]})
    ctx.close()
    K.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
