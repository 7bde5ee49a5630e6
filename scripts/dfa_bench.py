#!/usr/bin/env python3
"""Times the 32-bit comparison as a leveled automaton (tfhe_amd_dfa_run_dev) beside
the same comparison as a gate circuit (tfhe_amd_circuit_compare) on LWE inputs, in one process.

  python scripts/dfa_bench.py [--out profiles/dfa_bench.jsonl] [--runs 7]

Key-switched device forms on device-resident arrays at B = 1 and B = 1024:
  dfa_lt      x < y over 64 TGSW-encrypted bits (len = 64), n_out = 1
  dfa_lt_eq_gt  the same word, the three outputs (x < y, x = y, x > y), n_out = 3
  circuit_lt  x < y as tfhe_amd_circuit_compare over 2 x 32 LWE-encrypted bits, one circuit run
After a warm-up the configurations alternate, `runs` rounds; each figure is the wall time around
a stream synchronize.  One JSON line per configuration: median, min, max in ms, the CMux products
and the bootstraps per query."""
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
D = 32


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dfa_bench.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()

    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    rng = np.random.default_rng(3232)
    count = 24
    bits = rng.integers(0, 2, count).astype(np.int32)
    bits[:2] = (0, 1)
    tset = ctx.tgsw_import(K.tgsw_encrypt(bits))
    nxt, start, cls = T.dfa_compare()
    vals = np.array([[1 << 29 if c == k else -(1 << 29) for k in (T.DFA_LT, T.DFA_EQ, T.DFA_GT)] for c in cls], np.int32)
    d_fin = torch.from_numpy(T.dfa_fin(vals)).cuda()
    dfa = ctx.dfa_create(nxt, start, 2 * D)
    products = sum(int(nxt[s][0] != nxt[s][1]) for i in range(2 * D) for s in dfa.live(i))

    def pick(want):
        return np.array([rng.choice(np.flatnonzero(bits == w)) for w in want.reshape(-1)], np.int32).reshape(want.shape)

    def operands(B):
        """x, y [B] uint32 as [B][32] bit arrays, most significant bit first; a third of the pairs equal"""
        x = rng.integers(0, 2, (B, D))
        y = np.where(rng.integers(0, 3, (B, 1)) == 0, x, rng.integers(0, 2, (B, D)))
        lt = np.array([tuple(a) < tuple(b) for a, b in zip(x, y)])
        eq = (x == y).all(axis=1)
        return x, y, np.stack([lt, eq, ~lt & ~eq]).astype(np.int32)

    configs = []
    checks = []
    for B in (1, 1024):
        x, y, truth = operands(B)
        sel = torch.from_numpy(pick(np.stack([x, y], axis=2).reshape(B, 2 * D))).cuda()
        for name, n_out in (("dfa_lt", 1), ("dfa_lt_eq_gt", 3)):
            r_a = torch.zeros((n_out, B, n_lwe), dtype=torch.int32, device="cuda")
            r_b = torch.zeros((n_out, B), dtype=torch.int32, device="cuda")

            def run(sel=sel, r_a=r_a, r_b=r_b, n_out=n_out):
                ctx.dfa_run_dev(tset, dfa, sel, d_fin, r_a, r_b, None, n_out)
                ctx.sync()
            checks.append((name, B, r_a, r_b, truth[:n_out]))
            configs.append(dict(name=name, B=B, run=run, products=products, bootstraps=0))

    C = T.Circuit()
    xa, ya = C.inputs(D), C.inputs(D)            # little-endian wires
    out = C.compare(list(xa), list(ya), "LT")
    info = C.info()
    for B in (1, 1024):
        x, y, truth = operands(B)
        wa = torch.zeros((info["wires"], B, n_lwe), dtype=torch.int32, device="cuda")
        wb = torch.zeros((info["wires"], B), dtype=torch.int32, device="cuda")
        for wires, v in ((xa, x), (ya, y)):
            for i, w in enumerate(wires):
                a, b = K.encrypt(v[:, D - 1 - i], rng)
                wa[w] = torch.from_numpy(a).cuda()
                wb[w] = torch.from_numpy(b).cuda()

        def run(B=B, wa=wa, wb=wb):
            C.run_dev(ctx, B, wa, wb)
            ctx.sync()
        checks.append(("circuit_lt", B, wa[out:out + 1], wb[out:out + 1], truth[:1]))
        configs.append(dict(name="circuit_lt", B=B, run=run, products=0, bootstraps=info["bootstraps"]))
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
                       min_ms=round(t[0], 4), max_ms=round(t[-1], 4), cmux_products_per_query=c["products"],
                       bootstraps_per_query=c["bootstraps"], version=T.version())
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec))
    dfa.close()
    tset.close()
    ctx.close()
    K.close()


if __name__ == "__main__":
    main()
