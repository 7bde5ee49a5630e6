"""One-rotation adder cells against the gate builders.

One process, one context.  For each workload the gate circuit (`Circuit.mul` / `Circuit.dot`) and
the one-rotation circuit (`Circuit.mul_fa` / `Circuit.dot_fa`) are built over the same operands,
run once to warm up (compile, table upload, scratch), checked by decryption against integer
arithmetic, and then timed alternately: wall time of `Circuit.run_dev` around a device
synchronisation.  Workloads:
  mul: 16 x 16 bits over 256 instances;
  dot: one 64-term 16-bit dot product (the matrix-vector row of bench_matvec.py) over 64 instances,
       bench_matvec.py's rows per GPU.
Prints bootstraps, depth, every timing, the medians and the time ratio beside the bootstrap ratio.

    python scripts/fa_vs_gates.py [--reps 7] [--out FILE] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-gpu-tfhe_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    import torch
    import tfhe_amd as T
    import matvec

    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    emit({"what": "fa_vs_gates", "version": T.version(), "device": torch.cuda.get_device_name(0), "reps": args.reps})

    def build_mul(nbits, fa):
        C = T.Circuit()
        a, b = C.inputs(nbits), C.inputs(nbits)
        return C, a, b, (C.mul_fa if fa else C.mul)(a, b)

    def staged(C, planes, B):
        """the wire arrays with the inputs encrypted (the same ciphertexts for both circuits)"""
        n_w = C.info()["wires"]
        wa = torch.zeros((n_w, B, T.n_lwe), dtype=torch.int32, device="cuda")
        wb = torch.zeros((n_w, B), dtype=torch.int32, device="cuda")
        for w, (ea, eb) in planes.items():
            wa[w] = torch.from_numpy(ea).cuda()
            wb[w] = torch.from_numpy(eb).cuda()
        return wa, wb

    def decrypt(wa, wb, wires):
        return T.int_of([K.decrypt(wa[w].cpu().numpy(), wb[w].cpu().numpy()) for w in wires])

    def measure(name, B, circuits, want, shape):
        """circuits: {"gates": (C, enc planes, out wires), "fa": ...}"""
        state, res = {}, {}
        for k, (C, planes, outs) in circuits.items():
            wa, wb = staged(C, planes, B)
            C.run_dev(ctx, B, wa, wb)       # warm-up: compile, table upload, scratch
            ctx.sync()
            kern = ctx.last_kernels()
            ok = bool(np.array_equal(decrypt(wa, wb, outs), want))
            state[k] = (C, wa, wb)
            res[k] = {"info": C.info(), "correct": ok, "kernels": kern, "ms": []}
        for _ in range(args.reps):
            for k in ("gates", "fa"):
                C, wa, wb = state[k]
                ctx.sync()
                t0 = time.perf_counter()
                C.run_dev(ctx, B, wa, wb)
                ctx.sync()
                res[k]["ms"].append((time.perf_counter() - t0) * 1e3)
        for k, (C, planes, outs) in circuits.items():   # still right after the timed runs
            res[k]["correct"] = res[k]["correct"] and bool(np.array_equal(decrypt(*state[k][1:], outs), want))
        med = {k: float(np.median(res[k]["ms"])) for k in res}
        out = {"workload": name, "shape": shape, "B": B}
        for k in ("gates", "fa"):
            i = res[k]["info"]
            out[k] = {"bootstraps": i["bootstraps"], "depth": i["depth"], "wires": i["wires"],
                      "correct": res[k]["correct"], "median_ms": round(med[k], 3),
                      "min_ms": round(min(res[k]["ms"]), 3), "max_ms": round(max(res[k]["ms"]), 3),
                      "ms": [round(x, 3) for x in res[k]["ms"]],
                      "bootstraps_per_s": round(i["bootstraps"] * B / (med[k] * 1e-3))}
        out["kernels_fa"] = [k for k in res["fa"]["kernels"] if "blind_rotate" in k]
        out["bootstrap_ratio"] = round(res["fa"]["info"]["bootstraps"] / res["gates"]["info"]["bootstraps"], 4)
        out["time_ratio"] = round(med["fa"] / med["gates"], 4)
        out["gates_spread"] = [round(min(res["gates"]["ms"]) / med["gates"], 4),
                               round(max(res["gates"]["ms"]) / med["gates"], 4)]
        emit(out)
        for k in state:
            state[k][0].close()

    # 1. multiply
    nbits, B = (4, 8) if args.small else (16, 256)
    rng = np.random.default_rng(51)
    x, y = rng.integers(0, 2**nbits, B), rng.integers(0, 2**nbits, B)
    enc = [K.encrypt(p, rng) for p in T.bits_of(x, nbits) + T.bits_of(y, nbits)]
    circuits = {}
    for k, fa in (("gates", False), ("fa", True)):
        C, a, b, prod = build_mul(nbits, fa)
        circuits[k] = (C, dict(zip(a + b, enc)), prod)
    measure("mul", B, circuits, x * y, f"{nbits} x {nbits} bits")

    # 2. the matrix-vector row
    cols, nbits, B = (3, 4, 5) if args.small else (64, 16, 64)
    rng = np.random.default_rng(52)
    A, xv = rng.integers(0, 2**nbits, (B, cols)), rng.integers(0, 2**nbits, cols)
    ob = matvec.out_bits(cols, nbits)
    want = (A @ xv) % (1 << ob)   # < 2^38: exact in int64
    circuits = {}
    enc = None
    for k, fa in (("gates", False), ("fa", True)):
        C, a_w, x_w, y_w = matvec.build(T, cols, nbits, fa=fa)
        bits = matvec.instance_inputs(T, a_w, x_w, A, xv, nbits)
        if enc is None:   # both builders number their input wires alike
            enc = {w: K.encrypt(p, rng) for w, p in bits.items()}
        assert sorted(bits) == sorted(enc)
        circuits[k] = (C, enc, y_w)
    measure("dot", B, circuits, want, f"{cols} terms x {nbits} bits -> {ob} bits")

    ctx.close()
    K.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
