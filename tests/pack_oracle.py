"""The LWE -> TLWE packing key switch in numpy and the CPU oracle's polynomial
product (TEST INFRASTRUCTURE: the expected values of tests/test_pack.py and tests/test_pack_gpu.py).

    OUT = (0, sum_p b_p X^pos[p]) - sum_{i < 500, j = 1..6} D_ij (*) K_ij
    D_ij = sum_p d_j(a_p[i]) X^pos[p],  d_j(a) = (((a + 0x88888880) >> (32 - 4 j)) & 15) - 8

Two independent routes to OUT:
  pack_rows    row by row: the oracle's exact negacyclic product orc_negacyclic_addmul_ntt of D_ij
               and each polynomial of K_ij, 6 000 calls per output, then negated;
  pack_inputs  input by input: sum_ij d_j(a_p[i]) K_ij as an integer matrix product (no polynomial
               arithmetic at all), then one negacyclic shift by pos[p] per input.
A pos entry outside [0, 1024) drops its input (the device form's rule; the host form refuses it)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import many_lut_oracle as MO
import oracle_ctypes as O

N, n_lwe = O.N, O.n_lwe
BASEBIT, T_DIG = 4, 6
OFFSET = 0x88888880
SIGMA_BK = 7.180961047225788e-09
THREADS = MO.THREADS
wrap = MO.wrap


def digits(a):
    """mask words (any shape) -> balanced digits [..., 6] in [-8, 7], digit j = 1 first"""
    u = (np.asarray(a).astype(np.int64) + OFFSET) & 0xFFFFFFFF
    return np.stack([((u >> (32 - BASEBIT * j)) & 15) - 8 for j in range(1, T_DIG + 1)], axis=-1)


def sigma_pack(P):
    """predicted standard deviation (torus units) of the noise the pack adds to every coefficient"""
    return np.sqrt(n_lwe * T_DIG * 21.5 * P) * SIGMA_BK


def _positions(P, pos):
    pos = np.arange(P) if pos is None else np.asarray(pos).astype(np.int64)
    return pos, (pos >= 0) & (pos < N)


def _body(in_b, pos, live):
    b = np.zeros(N, np.int64)
    b[pos[live]] = np.asarray(in_b).astype(np.int64)[live]
    return b


def pack_rows(key, in_a, in_b, pos=None):
    """route (a).  key [500][6][2][1024], in_a [T][P][500], in_b [T][P] -> [T][2][1024] int32"""
    key = O.i32(key).reshape(n_lwe * T_DIG, 2, N)
    in_a = np.asarray(in_a)
    T, P, _ = in_a.shape
    pos, live = _positions(P, pos)
    f = O.lib().orc_negacyclic_addmul_ntt
    out = np.zeros((T, 2, N), np.int32)
    for t in range(T):
        dig = digits(in_a[t])                                  # [P][500][6]
        D = np.zeros((n_lwe * T_DIG, N), np.int32)
        D[:, pos[live]] = dig[live].reshape(-1, n_lwe * T_DIG).T
        rows = np.flatnonzero(D.any(axis=1))

        def part(chunk):
            res = np.zeros((2, N), np.int32)
            for r in chunk:
                for c in range(2):
                    f(O._p(res[c]), O._p(D[r]), O._p(key[r, c]))
            return res.astype(np.int64)

        with ThreadPoolExecutor(THREADS) as pool:
            total = sum(pool.map(part, np.array_split(rows, THREADS)), np.zeros((2, N), np.int64))
        total = -total
        total[1] += _body(in_b[t], pos, live)
        out[t] = wrap(total)
    return out


def _shift(x, k):
    """X^k x over Z[X]/(X^N + 1), x [..., N]"""
    return np.concatenate([-x[..., N - k:], x[..., :N - k]], axis=-1) if k else x


def pack_inputs(key, in_a, in_b, pos=None):
    """route (b), meant for small P.  sum_ij d_ij K_ij in float64 BLAS on the two 16-bit halves of
    the key words: |sum| <= 3000 * 8 * 2^16 < 2^31, exact."""
    key = O.i32(key).reshape(n_lwe * T_DIG, 2 * N).astype(np.int64)
    lo = (key & 0xFFFF).astype(np.float64)
    hi = (key >> 16).astype(np.float64)
    in_a = np.asarray(in_a)
    T, P, _ = in_a.shape
    pos, live = _positions(P, pos)
    d = digits(in_a).reshape(T * P, n_lwe * T_DIG).astype(np.float64)
    M = ((d @ hi).astype(np.int64) << 16) + (d @ lo).astype(np.int64)
    M = M.reshape(T, P, 2, N)
    out = np.zeros((T, 2, N), np.int64)
    for t in range(T):
        for p in np.flatnonzero(live):
            out[t] -= _shift(M[t, p], int(pos[p]))
        out[t, 1] += _body(in_b[t], pos, live)
    return wrap(out)
