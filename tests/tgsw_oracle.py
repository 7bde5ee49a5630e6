"""The leveled table lookup composed from the CPU oracle's own functions (TEST
INFRASTRUCTURE: the expected values of tests/test_tgsw.py and tests/test_tgsw_gpu.py).

The caller's TGSW samples take the place of the first entries of a bootstrapping key, so the
oracle's orc_mux_rotate / orc_external_product run on them unchanged:
  1. key(samples, ksk): OracleKey over a pool [500][4][2][1024] whose first entries are the samples;
  2. CMux tree of the vertical packing: level l pairs the polynomials (2 j, 2 j + 1) with address
     bit d_h + l, out = d0 + external_product(d1 - d0, sel);
  3. ACC = the tree's result (or the table itself, a = 0 for a plaintext table), then for
     i = 0 .. d_h - 1: mux_rotate(ACC, sel[i], 2N - 2^(i + log_stride));
  4. sample extraction at f = 0 .. n_out - 1 in numpy (many_lut_oracle.extract);
  5. keyswitch_batch over the n_out B samples, function-major.
A selector outside [0, count) skips its rotation step and leaves d0 in the tree (the device
forms' rule; the host forms refuse it)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import many_lut_oracle as MO
import oracle_ctypes as O

N, n_lwe = O.N, O.n_lwe
THREADS = MO.THREADS
wrap = MO.wrap


def key(samples, ksk, use_ntt=True):
    """OracleKey whose bootstrapping key starts with the samples [count][4][2][1024]"""
    samples = O.i32(samples).reshape(-1, 4, 2, N)
    assert samples.shape[0] <= n_lwe
    pool = np.zeros((n_lwe, 4, 2, N), np.int32)
    pool[:samples.shape[0]] = samples
    k = O.OracleKey(pool, ksk, use_ntt=use_ntt)
    k.count = samples.shape[0]
    return k


def _tlwe(poly):
    """[rows][N] -> (a, b) [2][N]: a plaintext polynomial is the trivial sample (0, poly)"""
    poly = np.asarray(poly)
    if poly.shape[0] == 2:
        return poly.astype(np.int32)
    return np.stack([np.zeros(N, np.int32), poly[0].astype(np.int32)])


def cmux(okey, i, d1, d0=None):
    """d0 + C_i (x) (d1 - d0); d0 = None: the external product of d1; a bad index: d0"""
    d1 = np.asarray(d1).reshape(2, N)
    z = np.zeros((2, N), np.int32) if d0 is None else np.asarray(d0).reshape(2, N)
    if i < 0 or i >= okey.count:
        return z.astype(np.int32)
    diff = wrap(d1.astype(np.int64) - z.astype(np.int64))
    return wrap(okey.external_product(diff, i).astype(np.int64) + z.astype(np.int64))


def lookup_acc(okey, sel, table, log_stride):
    """the accumulator of one query after the tree and the d_h rotation steps; table [n_poly][rows][N]"""
    n_poly = table.shape[0]
    levels = n_poly.bit_length() - 1
    d_h = len(sel) - levels
    polys = [_tlwe(p) for p in table]
    for l in range(levels):
        polys = [cmux(okey, int(sel[d_h + l]), polys[2 * j + 1], polys[2 * j]) for j in range(len(polys) // 2)]
    acc = polys[0]
    for i in range(d_h):
        if 0 <= int(sel[i]) < okey.count:
            acc = okey.mux_rotate(acc, int(sel[i]), 2 * N - (1 << (i + log_stride)))
    return acc


def lookup_woks(okey, sel, tab, tab_index=None, log_stride=0, n_out=1):
    """sel [B][d], tab [n_tab][n_poly][rows][N] -> (u_a [n_out][B][N], u_b [n_out][B])"""
    sel = np.asarray(sel)
    tab = O.i32(tab)
    B = sel.shape[0]
    idx = np.zeros(B, np.int64) if tab_index is None else np.clip(np.asarray(tab_index, dtype=np.int64), 0,
                                                                  tab.shape[0] - 1)

    def one(q):
        acc = lookup_acc(okey, sel[q], tab[idx[q]], log_stride)
        out = [MO.extract(acc[0], acc[1], f) for f in range(n_out)]
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)

    with ThreadPoolExecutor(THREADS) as pool:
        res = list(pool.map(one, range(B)))
    u_a = np.stack([r[0] for r in res], axis=1)
    u_b = np.stack([r[1] for r in res], axis=1)
    return np.ascontiguousarray(u_a), np.ascontiguousarray(u_b)


def lookup(okey, sel, tab, tab_index=None, log_stride=0, n_out=1):
    """the key-switched form -> (r_a [n_out][B][500], r_b [n_out][B])"""
    return MO.keyswitch(okey, lookup_woks(okey, sel, tab, tab_index, log_stride, n_out))


def tlwe_phase(tlwe_key, a, b):
    """b - a s over Z[X]/(X^N + 1) mod 2^32 for a binary key s [N] -> int32 [N]"""
    a = np.asarray(a).astype(np.int64)
    acc = np.asarray(b).astype(np.int64).copy()
    for k in np.flatnonzero(np.asarray(tlwe_key)):
        acc[k:] -= a[:N - k]          # X^k a, negacyclic
        acc[:k] += a[N - k:]
    return wrap(acc)


def pick(rng, bits, want):
    """for each wanted bit, the index of a random pool sample that encrypts it"""
    bits = np.asarray(bits)
    return np.array([rng.choice(np.flatnonzero(bits == w)) for w in np.asarray(want).reshape(-1)],
                    np.int32).reshape(np.asarray(want).shape)
