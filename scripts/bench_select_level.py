#!/usr/bin/env python3
"""What a select row costs inside a circuit level, against the batch call.

A circuit of ONE select node over p + 1 input wires, run at B instances through
tfhe_amd_circuit_run_pk_dev, against tfhe_amd_select_batch_dev on the same words (function-major
candidates [p][B][500]), on one device, alternating, `reps` timed calls each after a warm-up of both at
every shape.  A call is timed with the host clock from before the call to after the context's stream
has drained.  The two give the same words (checked).  One JSON line per (B, p) on stdout.

    python scripts/bench_select_level.py [--shapes 256:4,1024:4] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-gpu-tfhe_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256:4,1024:4", help="B:p, comma separated")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import tfhe_amd as T
    if not torch.cuda.is_available():
        sys.exit("bench_select_level: no GPU (there is no CPU fallback)")
    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    rng = np.random.default_rng(39)
    r32 = lambda shape: rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)
    pkey = ctx.pack_key_import(r32((500, 6, 2, 1024)))
    for shape in args.shapes.split(","):
        B, p = (int(x) for x in shape.split(":"))
        cand_a, cand_b = torch.from_numpy(r32((p, B, 500))).cuda(), torch.from_numpy(r32((p, B))).cuda()
        y_a, y_b = torch.from_numpy(r32((B, 500))).cuda(), torch.from_numpy(r32(B)).cuda()
        C = T.Circuit()
        ins = C.inputs(p + 1)
        out = C.select(ins[:p], ins[p])
        wa = torch.zeros((p + 2, B, 500), dtype=torch.int32, device="cuda")
        wb = torch.zeros((p + 2, B), dtype=torch.int32, device="cuda")
        wa[:p], wb[:p], wa[p], wb[p] = cand_a, cand_b, y_a, y_b
        r_a = torch.zeros((B, 500), dtype=torch.int32, device="cuda")
        r_b = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def level():
            C.run_dev(ctx, B, wa, wb, pack_key=pkey)

        def batch():
            ctx.select_dev(pkey, cand_a, cand_b, y_a, y_b, r_a, r_b)

        def timed(fn):
            t = time.perf_counter()
            fn()
            ctx.sync()
            return (time.perf_counter() - t) * 1e3
        kernels = {}
        for name, fn in (("level", level), ("batch", batch)):       # warm-up, and the launch lists
            for _ in range(2):
                timed(fn)
            kernels[name] = ctx.last_kernels()
        assert torch.equal(wa[out], r_a) and torch.equal(wb[out], r_b), "the level and the batch call differ"
        ms = {"level": [], "batch": []}
        for _ in range(args.reps):
            for name, fn in (("batch", batch), ("level", level)):   # alternating
                ms[name].append(timed(fn))
        line = {"B": B, "p": p, "reps": args.reps}
        for name in ("batch", "level"):
            line[name + "_ms_median"] = round(statistics.median(ms[name]), 4)
            line[name + "_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
            line[name + "_ms"] = [round(x, 4) for x in ms[name]]
            line[name + "_kernels"] = kernels[name]
        line["level_over_batch"] = round(line["level_ms_median"] / line["batch_ms_median"], 4)
        print(json.dumps(line), flush=True)
        C.close()
    pkey.close()
    ctx.close()
    K.close()


if __name__ == "__main__":
    main()
