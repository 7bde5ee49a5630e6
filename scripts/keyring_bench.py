#!/usr/bin/env python3
"""Mixed-key batches against what a caller does without them.

1 024 NAND gates whose ciphertexts belong to G in {1, 4, 32} cloud keys, evenly interleaved
(ciphertext i under key i mod G), three ways:
  (a) ring      one KeyRing.gate_dev call over all 1 024;
  (b) per_key   G tfhe_amd_gate_batch_dev calls of 1 024 / G gates, one per member context, each on
                its context's own stream, issued back to back and then all waited for;
  (c) single    the single-key B = 1 024 call on member 0 (the headline's launch).
One process; warm-up calls of every configuration, then the configurations alternating in a fresh
seeded order per run, RUNS runs each; a run is one untimed lead-in call, then INNER calls issued back
to back and timed by the host clock around the stream synchronisation that ends them (without the
lead-in the configuration that follows the 32-context one measured 0.45 ms per call slower than the
same call elsewhere in the order).  Reported per configuration: median (min .. max) milliseconds per
call.  Before timing, (a) and (b) are compared word for word.

Distinct keys: member g's bootstrapping key is the session key with its 500 key indices rotated by
g (np.roll): distinct device memory and distinct words of a real key's magnitudes; the timing does
not depend on the key's validity and nothing is decrypted.  Key traffic of a launch, from shapes:
every CMux step of a row reads one 64 KB slice of its key (4 rows x 2 polynomials x 512 complex
doubles), so 1 024 rows x 500 steps x 64 KB = 33.6 GB per launch, from G x 32.8 MB of distinct key.

    python scripts/keyring_bench.py [--out profiles/keyring.jsonl] [--keys 1,4,32]
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

B, N_LWE = 1024, 500
KEY_SLICE_BYTES = 4 * 2 * 512 * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="1,4,32")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tfhe_amd as T
    if not torch.cuda.is_available():
        sys.exit("keyring_bench: no GPU (there is no CPU path to time)")
    groups = [int(x) for x in args.keys.split(",")]
    K = T.SecretKeyset()
    ctxs = [T.Context(np.roll(K.bk, g, axis=0), K.ksk, device=0) for g in range(max(groups))]
    rng = np.random.default_rng(1024)
    words = lambda shape: torch.from_numpy(rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)).cuda()
    ins = [words((B, N_LWE)), words(B), words((B, N_LWE)), words(B)]
    res = [torch.zeros((B, N_LWE), dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()

    configs = {}   # name -> (call, wait)
    rings = []
    for G in groups:
        ring = T.KeyRing(ctxs[:G])
        rings.append(ring)
        key_of = np.arange(B) % G
        gates = np.full(B, T.GATES["NAND"], np.int32)
        n = B // G
        sub_in = [[x[g::G].contiguous() for x in ins] for g in range(G)]
        sub_res = [[torch.zeros((n, N_LWE), dtype=torch.int32, device="cuda"),
                    torch.zeros(n, dtype=torch.int32, device="cuda")] for g in range(G)]
        torch.cuda.synchronize()

        def ring_call(ring=ring, key_of=key_of, gates=gates):
            ring.gate_dev(gates, key_of, res[0], res[1], *ins)

        def per_key_call(G=G, sub_in=sub_in, sub_res=sub_res):
            for g in range(G):
                ctxs[g].gate_dev("NAND", sub_res[g][0], sub_res[g][1], *sub_in[g])

        def per_key_wait(G=G):
            for g in range(G):
                ctxs[g].sync()

        # (a) == (b), word for word
        ring_call(); ctxs[0].sync()
        kern = ctxs[0].last_kernels()
        per_key_call(); per_key_wait()
        for g in range(G):
            assert torch.equal(res[0][g::G], sub_res[g][0]) and torch.equal(res[1][g::G], sub_res[g][1]), (G, g)
        configs[f"ring_G{G}"] = (ring_call, ctxs[0].sync, G, "ring")
        configs[f"per_key_G{G}"] = (per_key_call, per_key_wait, G, "per_key")
    configs["single_B1024"] = (lambda: ctxs[0].gate_dev("NAND", res[0], res[1], *ins), ctxs[0].sync, 1, "single")

    def run(call, wait):
        call()   # untimed lead-in: the first call after another configuration's streams measured slower
        wait()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            call()
        wait()
        return (time.perf_counter() - t0) * 1e3 / args.inner

    for call, wait, _, _ in configs.values():
        for _ in range(args.warmup):
            run(call, wait)
    times = {name: [] for name in configs}
    names = list(configs)
    for r in range(args.runs):   # a fresh seeded order per run: no configuration always follows the same one
        for k in np.random.default_rng(r).permutation(len(names)):
            times[names[k]].append(run(configs[names[k]][0], configs[names[k]][1]))
    lines = []
    for name, (_, _, G, way) in configs.items():
        t = times[name]
        lines.append({"bench": "keyring", "config": name, "way": way, "keys": G, "gates": B,
                      "ms_per_call_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
                      "ms_max": round(max(t), 4), "runs": args.runs, "calls_per_run": args.inner,
                      "gates_per_s": round(B / statistics.median(t) * 1e3),
                      "key_bytes_read_per_call": B * 500 * KEY_SLICE_BYTES,
                      "distinct_key_bytes": G * 500 * KEY_SLICE_BYTES,
                      "device": torch.cuda.get_device_name(0), "version": T.version()})
    lines[0]["ring_kernels"] = kern
    lines[0]["recomputed_by_guard"] = sum(c.guard_stats()[1] for c in ctxs)   # 0: no run paid for an exact recomputation
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    for ring in rings:
        ring.close()
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
