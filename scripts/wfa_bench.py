#!/usr/bin/env python3
"""Times the maximum of two 32-bit integers as a weighted leveled automaton (tfhe_amd_wfa_run_dev,
DESIGN.md §3.12) beside the same maximum as a gate circuit (tfhe_amd_circuit_minmax) on LWE inputs,
in one process.

  python scripts/wfa_bench.py [--out profiles/wfa_bench.jsonl] [--runs 7]

Key-switched device forms on device-resident arrays at B = 1 and B = 1024:
  wfa_max      all 32 bits of max(x, y) over 64 TGSW-encrypted bits (len = 64), n_out = 32
  circuit_max  max(x, y) as tfhe_amd_circuit_minmax over 2 x 32 LWE-encrypted bits, one circuit run
The two forms take different inputs (TGSW samples of the client's bits against LWE samples): the
table prices the input layer, as in §3.10.  After a warm-up the configurations alternate, `runs`
rounds; each figure is the wall time around a stream synchronize.  One JSON line per configuration:
median, min, max in ms, the CMux products and the bootstraps per query."""
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wfa_bench.jsonl"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()

    K = T.SecretKeyset()
    ctx = T.Context(K.bk, K.ksk, device=0)
    rng = np.random.default_rng(3264)
    count = 24
    bits = rng.integers(0, 2, count).astype(np.int32)
    bits[:2] = (0, 1)
    tset = ctx.tgsw_import(K.tgsw_encrypt(bits))
    nxt, start, (w_val, w_pos), fin = T.wfa_max(D)
    d_fin = torch.from_numpy(fin).cuda()
    d_w = (torch.from_numpy(w_val).cuda(), torch.from_numpy(w_pos).cuda())
    dfa = ctx.dfa_create(nxt, start, 2 * D)
    products = sum(int(nxt[s][0] != nxt[s][1] or w_val[s][0] != w_val[s][1]) for i in range(2 * D) for s in dfa.live(i))

    def pick(want):
        return np.array([rng.choice(np.flatnonzero(bits == w)) for w in want.reshape(-1)], np.int32).reshape(want.shape)

    def operands(B):
        """x, y [B] as [B][32] bit arrays, most significant bit first; a third of the pairs equal ->
        (x, y, the bits of max(x, y) [32][B], bit 0 first)"""
        x = rng.integers(0, 2, (B, D))
        y = np.where(rng.integers(0, 3, (B, 1)) == 0, x, rng.integers(0, 2, (B, D)))
        gt = np.array([tuple(a) > tuple(b) for a, b in zip(x, y)])
        m = np.where(gt[:, None], x, y)
        return x, y, np.ascontiguousarray(m[:, ::-1].T).astype(np.int32)

    configs = []
    checks = []
    for B in (1, 1024):
        x, y, truth = operands(B)
        sel = torch.from_numpy(pick(np.stack([x, y], axis=2).reshape(B, 2 * D))).cuda()
        r_a = torch.zeros((D, B, n_lwe), dtype=torch.int32, device="cuda")
        r_b = torch.zeros((D, B), dtype=torch.int32, device="cuda")

        def run(sel=sel, r_a=r_a, r_b=r_b):
            ctx.dfa_run_dev(tset, dfa, sel, d_fin, r_a, r_b, None, D, weights=d_w)
            ctx.sync()
        checks.append(("wfa_max", B, r_a, r_b, truth))
        configs.append(dict(name="wfa_max", B=B, run=run, products=products, bootstraps=0))

    C = T.Circuit()
    xa, ya = C.inputs(D), C.inputs(D)            # little-endian wires
    out = C.minmax(list(xa), list(ya), want_max=True)
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
        idx = torch.tensor(out, device="cuda")
        checks.append(("circuit_max", B, (wa, idx), (wb, idx), truth))
        configs.append(dict(name="circuit_max", B=B, run=run, products=0, bootstraps=info["bootstraps"]))
    torch.cuda.synchronize()

    for c in configs:   # warm-up (scratch growth, circuit tables), then every result is checked once
        c["run"]()
        c["run"]()
    for name, B, r_a, r_b, want in checks:
        if isinstance(r_a, tuple):
            r_a, r_b = r_a[0][r_a[1]], r_b[0][r_b[1]]
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
