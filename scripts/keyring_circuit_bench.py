#!/usr/bin/env python3
"""Mixed-key circuits against what a caller does without them.

BASELINE config 3's 32-bit ripple add and the 8 x 8 mul_fa, B = 256 instances whose ciphertexts
belong to G in {1, 4, 32} cloud keys, evenly interleaved (instance i under key i mod G), three ways:
  (a) ring      one KeyRing.circuit_dev call over all 256;
  (b) per_key   G Circuit.run_dev calls of 256 / G instances, one per member context, each on its
                context's own stream, issued back to back and then all waited for;
  (c) single    the single-key B = 256 run on member 0.
One process; a warm-up of every configuration, then the configurations alternating in a fresh
seeded order per run, RUNS runs each; a run is one call timed by the host clock around the stream
synchronisation that ends it.  Reported per configuration: median (min .. max) milliseconds per
call.  Before timing, (a) and (b) are compared word for word on every wire.  The profiler is off
while timing; afterwards one profiled ring call per configuration gives the key switch's share of
the device time from the profile counters (tfhe_amd_profile_read).

--only ring restricts a process to (a): for alternating two builds of the library (TFHE_AMD_LIB),
e.g. the per-group key switch forced by -DTFHE_AMD_RING_KS_PER_GROUP; --label names the build in
the output lines.

Distinct keys as in scripts/keyring_bench.py: member g's bootstrapping key is the session key with
its 500 key indices rotated by g; nothing is decrypted.

    python scripts/keyring_circuit_bench.py [--out profiles/keyring_circuit.jsonl] [--keys 1,4,32]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-gpu-tfhe_amd"))

B, N_LWE = 256, 500


def circuits(T):
    C = T.Circuit()
    a, b = C.inputs(32), C.inputs(32)
    C.add(a, b)
    M = T.Circuit()
    x, y = M.inputs(8), M.inputs(8)
    M.mul_fa(x, y)
    return {"add32": (C, a + b), "mul_fa8": (M, x + y)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="1,4,32")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="ring: time configuration (a) alone")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tfhe_amd as T
    if not torch.cuda.is_available():
        sys.exit("keyring_circuit_bench: no GPU (there is no CPU path to time)")
    groups = [int(x) for x in args.keys.split(",")]
    K = T.SecretKeyset()
    ctxs = [T.Context(np.roll(K.bk, g, axis=0), K.ksk, device=0) for g in range(max(groups))]
    rng = np.random.default_rng(256)
    words = lambda shape: torch.from_numpy(rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)).cuda()

    configs = {}   # name -> (call, wait, G, way, workload)
    rings = {G: T.KeyRing(ctxs[:G]) for G in groups}
    info = {}
    for wl, (C, ins) in circuits(T).items():
        n_w = C.info()["wires"]
        info[wl] = dict(C.info(), levels=sum(1 for r in C.level_sizes() if r > 0))
        wa, wb = torch.zeros((n_w, B, N_LWE), dtype=torch.int32, device="cuda"), torch.zeros((n_w, B), dtype=torch.int32, device="cuda")
        for w in ins:
            wa[w], wb[w] = words((B, N_LWE)), words(B)
        torch.cuda.synchronize()
        for G in groups:
            ring, key_of, n = rings[G], np.arange(B) % G, B // G
            sub = [(wa[:, g::G].contiguous(), wb[:, g::G].contiguous()) for g in range(G)]
            torch.cuda.synchronize()

            def ring_call(ring=ring, C=C, key_of=key_of, wa=wa, wb=wb):
                ring.circuit_dev(C, key_of, wa, wb)

            def per_key_call(G=G, C=C, sub=sub, n=n):
                for g in range(G):
                    C.run_dev(ctxs[g], n, sub[g][0], sub[g][1])

            def per_key_wait(G=G):
                for g in range(G):
                    ctxs[g].sync()

            # (a) == (b), word for word on every wire
            ring_call(); ctxs[0].sync()
            per_key_call(); per_key_wait()
            for g in range(G):
                assert torch.equal(wa[:, g::G], sub[g][0]) and torch.equal(wb[:, g::G], sub[g][1]), (wl, G, g)
            configs[f"{wl}_ring_G{G}"] = (ring_call, ctxs[0].sync, G, "ring", wl)
            if args.only != "ring":
                configs[f"{wl}_per_key_G{G}"] = (per_key_call, per_key_wait, G, "per_key", wl)
        if args.only != "ring":
            configs[f"{wl}_single_B{B}"] = (lambda C=C, wa=wa, wb=wb: C.run_dev(ctxs[0], B, wa, wb), ctxs[0].sync, 1,
                                            "single", wl)

    def run(call, wait):
        t0 = time.perf_counter()
        call()
        wait()
        return (time.perf_counter() - t0) * 1e3

    for call, wait, _, _, _ in configs.values():
        for _ in range(args.warmup):
            run(call, wait)
    times = {name: [] for name in configs}
    names = list(configs)
    for r in range(args.runs):   # a fresh seeded order per run: no configuration always follows the same one
        for k in np.random.default_rng(r).permutation(len(names)):
            times[names[k]].append(run(configs[names[k]][0], configs[names[k]][1]))
    # the key switch's share of a ring call, from the profile counters (after the timing: profiler off there)
    share = {}
    ctxs[0].profile_enable(True)
    for name, (call, wait, G, way, wl) in configs.items():
        if way != "ring":
            continue
        p0 = ctxs[0].profile_read()   # the counters accumulate: one call's part is the difference
        call(); wait()
        p1 = ctxs[0].profile_read()
        p = {k: p1[k] - p0[k] for k in p1}
        share[name] = {"br_ms": round(p["br_ms"], 4), "ks_ms": round(p["ks_ms"], 4),
                       "ks_share": round(p["ks_ms"] / max(p["br_ms"] + p["ks_ms"], 1e-9), 4),
                       "ring_kernels": ctxs[0].last_kernels()[:6]}
    ctxs[0].profile_enable(False)
    lines = []
    for name, (_, _, G, way, wl) in configs.items():
        t = times[name]
        ln = {"bench": "keyring_circuit", "build": args.label, "config": name, "workload": wl, "way": way, "keys": G,
              "instances": B, "ms_per_call_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
              "ms_max": round(max(t), 4), "runs": args.runs, **{k: info[wl][k] for k in ("bootstraps", "levels")},
              "device": torch.cuda.get_device_name(0), "version": T.version()}
        ln.update(share.get(name, {}))
        lines.append(ln)
    lines[0]["recomputed_by_guard"] = sum(c.guard_stats()[1] for c in ctxs)
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out:
        with open(args.out, "a" if args.only else "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    for ring in rings.values():
        ring.close()
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
