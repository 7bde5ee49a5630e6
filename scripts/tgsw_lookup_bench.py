#!/usr/bin/env python3
"""Times the leveled table lookup (tfhe_amd_tgsw_lookup_dev) beside the same lookup
built as a MUX-tree circuit on the bootstrapping engine, in one process.

  python scripts/tgsw_lookup_bench.py [--out profiles/tgsw_lookup.jsonl] [--runs 7]

Key-switched lookups on device-resident arrays at B = 1 and B = 1024:
  d10     d_h = 10, stride 1: one entry of a 1024-entry table
  d7x8    d_h = 7, stride 8, n_out = 8: one 8-word entry of a 128-entry table
  d6      d_h = 6, stride 1: one entry of a 64-entry table, the size of the circuit below
  mux64   the 64-entry table as a tree of 63 MUX gates over 6 LWE address bits, one circuit run
After a warm-up the configurations alternate, `runs` rounds; each figure is the wall time around
a stream synchronize.  One JSON line per configuration: median, min, max in ms, the bootstraps or
CMux steps per query, and the bytes of TGSW samples a query reads (64 KB per step)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-gpu-tfhe_amd"))

import tfhe_amd as T  # noqa: E402

N, n_lwe = 1024, 500
SAMPLE_BYTES = 2 * 2 * 4 * N * 4   # two primes x (a, b) x 4 rows x N words


def mux_tree(entries):
    """entries[addr] in {0, 1} -> (circuit, address input wires, output wire)"""
    C = T.Circuit()
    bits = C.inputs(6)
    level = [C.gate("CONST", int(v)) for v in entries]
    for i in range(6):
        level = [C.gate("MUX", bits[i], level[2 * j + 1], level[2 * j]) for j in range(len(level) // 2)]
    return C, list(bits), level[0]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tgsw_lookup.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()

    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    rng = np.random.default_rng(64)
    count = 24
    bits = rng.integers(0, 2, count).astype(np.int32)
    bits[:2] = (0, 1)
    tset = ctx.tgsw_import(K.tgsw_encrypt(bits))
    table = ((rng.integers(0, 2, N) * 2 - 1) << 29).astype(np.int32)
    d_tab = torch.from_numpy(table.reshape(1, 1, 1, N)).cuda()

    def pick(want):
        return np.array([rng.choice(np.flatnonzero(bits == w)) for w in want.reshape(-1)], np.int32).reshape(want.shape)

    configs = []
    checks = []
    for name, d_h, ls, n_out in (("d10", 10, 0, 1), ("d7x8", 7, 3, 8), ("d6", 6, 0, 1)):
        for B in (1, 1024):
            addr = rng.integers(0, 1 << d_h, B)
            sel = torch.from_numpy(pick((addr[:, None] >> np.arange(d_h)) & 1)).cuda()
            r_a = torch.zeros((n_out, B, n_lwe), dtype=torch.int32, device="cuda")
            r_b = torch.zeros((n_out, B), dtype=torch.int32, device="cuda")

            def run(sel=sel, r_a=r_a, r_b=r_b, ls=ls, n_out=n_out):
                ctx.tgsw_lookup_dev(tset, sel, d_tab, r_a, r_b, None, ls, n_out)
                ctx.sync()
            want = np.stack([table[(addr << ls) + f] > 0 for f in range(n_out)]).astype(np.int32)
            checks.append((name, B, r_a, r_b, want))
            configs.append(dict(name=name, B=B, run=run, steps=d_h, bootstraps=0, tgsw_bytes=d_h * SAMPLE_BYTES))

    C, ins, out = mux_tree(table[:64] > 0)
    info = C.info()
    for B in (1, 1024):
        addr = rng.integers(0, 64, B)
        wa = torch.zeros((info["wires"], B, n_lwe), dtype=torch.int32, device="cuda")
        wb = torch.zeros((info["wires"], B), dtype=torch.int32, device="cuda")
        for i, w in enumerate(ins):
            a, b = K.encrypt((addr >> i) & 1, rng)
            wa[w] = torch.from_numpy(a).cuda()
            wb[w] = torch.from_numpy(b).cuda()

        def run(B=B, wa=wa, wb=wb):
            C.run_dev(ctx, B, wa, wb)
            ctx.sync()
        checks.append(("mux64", B, wa[out:out + 1], wb[out:out + 1], (table[addr] > 0).astype(np.int32)[None]))
        configs.append(dict(name="mux64", B=B, run=run, steps=0, bootstraps=info["bootstraps"], tgsw_bytes=0))
    torch.cuda.synchronize()

    for c in configs:   # warm-up (scratch growth, circuit tables), then every result is checked once
        c["run"]()
        c["run"]()
    for name, B, r_a, r_b, want in checks:
        got = K.decrypt(r_a.cpu().numpy().reshape(-1, n_lwe), r_b.cpu().numpy().reshape(-1))
        assert np.array_equal(got, want.reshape(-1)), (name, B)
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
            rec = dict(config=c["name"], B=c["B"], runs=len(t), median_ms=round(t[len(t) // 2], 4),
                       min_ms=round(t[0], 4), max_ms=round(t[-1], 4), cmux_steps_per_query=c["steps"],
                       bootstraps_per_query=c["bootstraps"], tgsw_bytes_per_query=c["tgsw_bytes"],
                       version=T.version())
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))
    tset.close()
    ctx.close()
    K.close()


if __name__ == "__main__":
    main()
