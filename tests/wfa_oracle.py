"""The weighted leveled automaton composed from the CPU oracle's own functions
(TEST INFRASTRUCTURE: the expected values of tests/test_wfa.py and tests/test_wfa_gpu.py), as
tests/dfa_oracle.py composes the unweighted one.  It shares no code with the library: the weights
are added in numpy, the CMux step is dfa_oracle.step and the plain simulation is Python.

For one query with the selectors sel [len] (bit 0 first), the final weights fin [Q][rows][N] and the
transition weights w_val [Q][2], w_pos [len]:
  1. ACC_len[s] = fin[s];
  2. for j = len .. 1, i = j - 1, p = w_pos[i] and every state s reachable after i bits:
       d_b = ACC_j[next[s][b]] + (0, w_val[s][b] X^p)      (coefficient p of the b polynomial alone)
       ACC_i[s] = step(sel[i], d1, d0) = d0 + C (x) (d1 - d0 + 2048)
     a state with next0 == next1 AND w0 == w1 takes d0 as it is (with the weight in it); a selector
     outside [0, count) gives d0 too (dfa_oracle.step's own rule); a p outside [0, N) makes the step
     weightless (both weights count as 0: the device forms' rule);
  3. sample extraction of ACC_0[start] at f = 0 .. n_out - 1 (many_lut_oracle.extract);
  4. keyswitch_batch over the n_out B samples, function-major (many_lut_oracle.keyswitch)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import dfa_oracle as DO
import many_lut_oracle as MO
import oracle_ctypes as O
import tgsw_oracle as TO

N, n_lwe = O.N, O.n_lwe
wrap = MO.wrap


def _weighted(d, w, p):
    """d + (0, w X^p)"""
    out = np.asarray(d).reshape(2, N).astype(np.int64)
    out[1, p] += int(w)
    return wrap(out)


def run_acc(okey, next, start, sel, fin, w_val, w_pos):
    """ACC_0[start] [2][N] of one query"""
    next, w_val = np.asarray(next), np.asarray(w_val)
    length = len(sel)
    live = DO.reach(next, start, length)
    acc = {s: TO._tlwe(fin[s]) for s in live[length]}
    for j in range(length, 0, -1):
        p = int(w_pos[j - 1])
        ok = 0 <= p < N
        new = {}
        for s in live[j - 1]:
            n0, n1 = int(next[s][0]), int(next[s][1])
            w0, w1 = (int(w_val[s][0]), int(w_val[s][1])) if ok else (0, 0)
            d0 = _weighted(acc[n0], w0, p if ok else 0)
            if n0 == n1 and w0 == w1:
                new[s] = d0
            else:
                new[s] = DO.step(okey, int(sel[j - 1]), _weighted(acc[n1], w1, p if ok else 0), d0)
        acc = new
    return acc[int(start)]


def run_woks(okey, next, start, sel, fin, w_val, w_pos, fin_index=None, n_out=1):
    """sel [B][len], fin [n_fin][Q][rows][N] -> (u_a [n_out][B][N], u_b [n_out][B])"""
    sel = np.asarray(sel)
    fin = O.i32(fin)
    B = sel.shape[0]
    idx = np.zeros(B, np.int64) if fin_index is None else np.clip(np.asarray(fin_index, dtype=np.int64), 0,
                                                                  fin.shape[0] - 1)

    def one(q):
        acc = run_acc(okey, next, start, sel[q], fin[idx[q]], w_val, w_pos)
        out = [MO.extract(acc[0], acc[1], f) for f in range(n_out)]
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)

    with ThreadPoolExecutor(MO.THREADS) as pool:
        res = list(pool.map(one, range(B)))
    u_a = np.stack([r[0] for r in res], axis=1)
    u_b = np.stack([r[1] for r in res], axis=1)
    return np.ascontiguousarray(u_a), np.ascontiguousarray(u_b)


def run(okey, next, start, sel, fin, w_val, w_pos, fin_index=None, n_out=1):
    """the key-switched form -> (r_a [n_out][B][500], r_b [n_out][B])"""
    return MO.keyswitch(okey, run_woks(okey, next, start, sel, fin, w_val, w_pos, fin_index, n_out))


def simulate(next, start, w_val, w_pos, bits):
    """(final state, poly [N] int32 = the sum of the weights along the path)"""
    poly = np.zeros(N, np.int64)
    s = int(start)
    for i, b in enumerate(np.asarray(bits).reshape(-1)):
        poly[int(w_pos[i])] += int(w_val[s][int(b)])
        s = int(next[s][int(b)])
    return s, wrap(poly)


def max_word(x, y, d):
    """the word of the max / min automaton: x_{d-1}, y_{d-1}, ..., x_0, y_0"""
    return [(v >> k) & 1 for k in range(d - 1, -1, -1) for v in (x, y)]
