"""The leveled automaton composed from the CPU oracle's own functions (TEST
INFRASTRUCTURE: the expected values of tests/test_dfa.py and tests/test_dfa_gpu.py), as
tests/tgsw_oracle.py composes the table lookup.

The caller's TGSW samples take the place of the first entries of a bootstrapping key (tgsw_oracle.key).
For one query with the selectors sel [len] (bit 0 first) and the final weights fin [Q][rows][N]:
  1. ACC_len[s] = fin[s] (a plaintext polynomial is the trivial sample (0, fin[s]));
  2. for j = len .. 1 and every state s reachable from the start state after j - 1 bits:
     ACC_{j-1}[s] = d0 + external_product(wrap(d1 - d0 + 2048), sel[j - 1]) with
     d_b = ACC_j[next[s][b]]; a state with next0 == next1 takes d0 as it is (its product is exactly
     zero, test_dfa.py pins that), and so does a selector outside [0, count) (the device forms' rule);
  3. sample extraction of ACC_0[start] at f = 0 .. n_out - 1 (many_lut_oracle.extract);
  4. keyswitch_batch over the n_out B samples, function-major (many_lut_oracle.keyswitch).
rounding=False leaves the 2048 out: the truncating composition of the diagnostic in test_dfa.py.
Reachability and simulation are plain Python."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import many_lut_oracle as MO
import oracle_ctypes as O
import tgsw_oracle as TO

N, n_lwe = O.N, O.n_lwe
THREADS = MO.THREADS
wrap = MO.wrap
ROUND = 1 << 11


def reach(next, start, steps):
    """[R_0, ..., R_steps]: the states reachable from start after i bits, each sorted"""
    next = np.asarray(next)
    out = [[int(start)]]
    for _ in range(steps):
        out.append(sorted({int(next[s][b]) for s in out[-1] for b in (0, 1)}))
    return out


def simulate(next, start, bits):
    s = int(start)
    for b in np.asarray(bits).reshape(-1):
        s = int(next[s][int(b)])
    return s


def step(okey, i, d1, d0, rounding=True):
    """d0 + C_i (x) (d1 - d0 + 2^11 on every word); a bad index: d0"""
    d0 = np.asarray(d0).reshape(2, N)
    if i < 0 or i >= okey.count:
        return d0.astype(np.int32)
    diff = wrap(np.asarray(d1).reshape(2, N).astype(np.int64) - d0.astype(np.int64) + (ROUND if rounding else 0))
    return wrap(okey.external_product(diff, i).astype(np.int64) + d0.astype(np.int64))


def run_acc(okey, next, start, sel, fin, rounding=True):
    """ACC_0[start] [2][N] of one query; sel [len], fin [Q][rows][N]"""
    next = np.asarray(next)
    length = len(sel)
    live = reach(next, start, length)
    acc = {s: TO._tlwe(fin[s]) for s in live[length]}
    for j in range(length, 0, -1):
        new = {}
        for s in live[j - 1]:
            n0, n1 = int(next[s][0]), int(next[s][1])
            new[s] = acc[n0] if n0 == n1 else step(okey, int(sel[j - 1]), acc[n1], acc[n0], rounding)
        acc = new
    return acc[int(start)]


def run_woks(okey, next, start, sel, fin, fin_index=None, n_out=1, rounding=True):
    """sel [B][len], fin [n_fin][Q][rows][N] -> (u_a [n_out][B][N], u_b [n_out][B])"""
    sel = np.asarray(sel)
    fin = O.i32(fin)
    B = sel.shape[0]
    idx = np.zeros(B, np.int64) if fin_index is None else np.clip(np.asarray(fin_index, dtype=np.int64), 0,
                                                                  fin.shape[0] - 1)

    def one(q):
        acc = run_acc(okey, next, start, sel[q], fin[idx[q]], rounding)
        out = [MO.extract(acc[0], acc[1], f) for f in range(n_out)]
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)

    with ThreadPoolExecutor(THREADS) as pool:
        res = list(pool.map(one, range(B)))
    u_a = np.stack([r[0] for r in res], axis=1)
    u_b = np.stack([r[1] for r in res], axis=1)
    return np.ascontiguousarray(u_a), np.ascontiguousarray(u_b)


def run(okey, next, start, sel, fin, fin_index=None, n_out=1):
    """the key-switched form -> (r_a [n_out][B][500], r_b [n_out][B])"""
    return MO.keyswitch(okey, run_woks(okey, next, start, sel, fin, fin_index, n_out))
