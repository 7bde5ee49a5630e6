"""The programmable bootstrap composed from the CPU oracle's own functions (TEST INFRASTRUCTURE:
the expected values of tests/test_lut.py and tests/test_lut_gpu.py).

The oracle (oracle/tfhe_oracle.c, tests/oracle_ctypes.py) has no LUT bootstrap of its own; it has
every piece of one.  For an input sample x (n = 500) and a test vector tv (N = 1024):
  1. barb, bara_i = modSwitchFromTorus32(x_b / x_a[i], 2N) = ((x + 2^20) >> 21) & 2047;
  2. acc = (0, X^{2N - barb} tv)                            (orc_mul_by_xai);
  3. orc_blind_rotate(acc, key, bara, 500);
  4. sample extraction at index 0: u_a[0] = acc_a[0], u_a[j] = -acc_a[N - j], u_b = acc_b[0];
  5. orc_keyswitch for the key-switched forms.
With tv = (mu, ..., mu) this is orc_bootstrap_woKS word for word (test_lut.py checks it).
ctypes releases the GIL, so batches run over a pool of at most 16 threads."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_ctypes as O

N, n_lwe = O.N, O.n_lwe
E8 = 1 << 29
LUT_GATE = -2
THREADS = min(16, os.cpu_count() or 4)


def wrap(x):
    return ((np.asarray(x, dtype=np.int64) + 2**31) % 2**32 - 2**31).astype(np.int32)


def modswitch_2n(x):
    """modSwitchFromTorus32(x, 2N), vectorised"""
    return ((((np.asarray(x).astype(np.int64) & 0xFFFFFFFF) + (1 << 20)) >> 21) & (2 * N - 1)).astype(np.int32)


def lin(c, terms, B):
    """(0, c) + sum_k s_k X_k over samples (a [B][500], b [B]), mod 2^32"""
    a = np.zeros((B, n_lwe), np.int64)
    b = np.full(B, int(c), np.int64)
    for s, (xa, xb) in terms:
        a += np.int64(s) * np.asarray(xa).astype(np.int64)
        b += np.int64(s) * np.asarray(xb).astype(np.int64)
    return wrap(a), wrap(b)


def woks_one(okey, tv, x_a, x_b):
    """steps 1-4 for one sample -> (u_a [N], u_b)"""
    L = O.lib()
    bara = np.ascontiguousarray(modswitch_2n(x_a))
    barb = int(modswitch_2n(np.int64(x_b)))
    acc = np.zeros((2, N), np.int32)
    acc[1] = O.mul_by_xai((2 * N - barb) % (2 * N), tv)
    L.orc_blind_rotate(O._p(acc.reshape(2 * N)), ctypes.c_void_p(okey.h), O._p(bara), n_lwe)
    u_a = np.empty(N, np.int32)
    u_a[0] = acc[0, 0]
    u_a[1:] = wrap(-acc[0, :0:-1].astype(np.int64))
    return u_a, int(acc[1, 0])


def woks_batch(okey, tvs, x_a, x_b, lut_index=None):
    """B samples through their tables: tvs [n_lut][N] (or one [N]); lut_index [B] or None (table 0)"""
    tvs = O.i32(tvs).reshape(-1, N)
    x_a, x_b = O.i32(x_a), O.i32(x_b)
    B = x_a.shape[0]
    idx = np.zeros(B, np.int64) if lut_index is None else np.asarray(lut_index, dtype=np.int64)
    with ThreadPoolExecutor(THREADS) as pool:
        out = list(pool.map(lambda i: woks_one(okey, tvs[idx[i]], x_a[i], x_b[i]), range(B)))
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def bootstrap_batch(okey, tvs, x_a, x_b, lut_index=None):
    """steps 1-5 -> (r_a [B][500], r_b [B])"""
    u_a, u_b = woks_batch(okey, tvs, x_a, x_b, lut_index)
    return okey.keyswitch_batch(u_a, u_b, nthreads=THREADS)


_decode_cache = {}


def decode_case(keyset, p, B=48):
    """B fresh encryptions of random messages in [0, p) at the key-switch noise (the parameter
    set's key-switch standard deviation, encrypt_digits' default) and a random table f encoded at
    (2 f(m) + 1) / (4p): shared by the CPU and the GPU decode tests, fixed seed.
    -> (msgs, f, tv, x_a, x_b)"""
    import tfhe_amd as T
    if p not in _decode_cache:
        rng = np.random.default_rng(1000 + p)
        msgs = rng.integers(0, p, B)
        f = rng.integers(0, p, p)
        tv = T.lut_table(p, T.lut_encode(f, p))
        x_a, x_b = keyset.encrypt_digits(msgs, p, rng)
        _decode_cache[p] = [msgs, f, tv, x_a, x_b, None]
    return tuple(_decode_cache[p][:5])


def decode_expected(keyset, okey, p):
    """the oracle's key-switched results for decode_case (computed once per process)"""
    _, _, tv, x_a, x_b = decode_case(keyset, p)
    if _decode_cache[p][5] is None:
        _decode_cache[p][5] = bootstrap_batch(okey, tv, x_a, x_b)
    return _decode_cache[p][5]


def eval_circuit(C, okey, inputs, B):
    """Node-by-node evaluation of a circuit with LUT nodes (and gate / lincomb / NOT / COPY / CONST
    nodes, as tests/circuit_oracle.py; no MUX): every wire an LWE sample, nothing folded.
    inputs: {wire: (a [B][500], b [B])}; returns {wire: (a, b)} for every wire."""
    n_w = C.info()["wires"]
    W = {}
    for w in range(n_w):
        kind, gate, c0, s, ins = C.node(w)
        if kind == 0:
            W[w] = tuple(np.asarray(v, dtype=np.int32) for v in inputs[w])
        elif kind == 2:
            if gate == 15:
                W[w] = (np.zeros((B, n_lwe), np.int32), np.full(B, c0, np.int32))
            else:
                sg = -1 if gate == 13 else 1
                W[w] = lin(0, [(sg, W[ins[0]])], B)
        else:
            assert gate != 10, "MUX: use circuit_oracle.eval_circuit"
            if gate == LUT_GATE:
                table, c0 = C.lut_node(w)
                tv = C.lut_table_get(table)
            else:
                tv = np.full(N, E8, np.int32)
            x = lin(c0, [(s[k], W[ins[k]]) for k in range(3) if ins[k] >= 0 and s[k] != 0], B)
            W[w] = bootstrap_batch(okey, tv, x[0], x[1])
    return W
