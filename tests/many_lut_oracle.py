"""The many-LUT bootstrap composed from the CPU oracle's own functions (TEST
INFRASTRUCTURE: the expected values of tests/test_lut_many.py and tests/test_lut_many_gpu.py), as
tests/lut_oracle.py composes the single-table one.

For an input sample x (n = 500), a test vector tv (N = 1024), theta = log_nu and n_out <= 2^theta:
  1. barb, bara_i = bar_theta(x_b / x_a[i]) = ((((x + 2^(20+theta)) >> (21+theta)) << theta) & 2047,
     numpy; pinned to nu * modSwitchFromTorus32(x, 2N / nu) of the oracle by test_lut_many.py;
  2. acc = (0, X^{2N - barb} tv)                            (orc_mul_by_xai);
  3. orc_blind_rotate(acc, key, bara, 500), ONCE per sample;
  4. sample extraction at index f = 0 .. n_out - 1 in numpy: u_f.a[j] = acc_a[f - j] for j <= f,
     -acc_a[N + f - j] for j > f, u_f.b = acc_b[f]; pinned to the index-0 extraction of
     X^{2N - f} acc by test_lut_many.py;
  5. orc_keyswitch of every extracted sample for the key-switched forms.
Outputs are function-major: [n_out][B][...]."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import lut_oracle as LO
import oracle_ctypes as O

N, n_lwe = O.N, O.n_lwe
LUT_MANY_GATE = -3
THREADS = LO.THREADS
wrap = LO.wrap


def bar(x, theta):
    """the modulus switch to a multiple of nu = 2^theta, vectorised"""
    x = np.asarray(x).astype(np.int64) & 0xFFFFFFFF
    return ((((x + (1 << (20 + theta))) >> (21 + theta)) << theta) & (2 * N - 1)).astype(np.int32)


def extract(acc_a, acc_b, f):
    """sample extraction at index f of the accumulator (acc_a [N], acc_b [N]) -> (u_a [N], u_b)"""
    j = np.arange(N)
    a = np.asarray(acc_a).astype(np.int64)
    u_a = np.where(j <= f, a[(f - j) % N], -a[(N + f - j) % N])
    return wrap(u_a), int(np.asarray(acc_b)[f])


def woks_one(okey, tv, x_a, x_b, theta, n_out):
    """steps 1-4 for one sample -> (u_a [n_out][N], u_b [n_out])"""
    L = O.lib()
    bara = np.ascontiguousarray(bar(x_a, theta))
    barb = int(bar(np.int64(x_b), theta))
    acc = np.zeros((2, N), np.int32)
    acc[1] = O.mul_by_xai((2 * N - barb) % (2 * N), tv)
    L.orc_blind_rotate(O._p(acc.reshape(2 * N)), ctypes.c_void_p(okey.h), O._p(bara), n_lwe)
    out = [extract(acc[0], acc[1], f) for f in range(n_out)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def woks_batch(okey, tvs, x_a, x_b, theta, n_out, lut_index=None):
    """B samples through their tables -> (u_a [n_out][B][N], u_b [n_out][B])"""
    tvs = O.i32(tvs).reshape(-1, N)
    x_a, x_b = O.i32(x_a), O.i32(x_b)
    B = x_a.shape[0]
    idx = np.zeros(B, np.int64) if lut_index is None else np.asarray(lut_index, dtype=np.int64)
    with ThreadPoolExecutor(THREADS) as pool:
        out = list(pool.map(lambda i: woks_one(okey, tvs[idx[i]], x_a[i], x_b[i], theta, n_out), range(B)))
    u_a = np.stack([o[0] for o in out], axis=1)
    u_b = np.stack([o[1] for o in out], axis=1)
    return np.ascontiguousarray(u_a), np.ascontiguousarray(u_b)


def keyswitch(okey, u):
    """step 5 over function-major extracted samples -> (r_a [n_out][B][500], r_b [n_out][B])"""
    n_out, B = u[1].shape
    r_a, r_b = okey.keyswitch_batch(u[0].reshape(n_out * B, N), u[1].reshape(n_out * B), nthreads=THREADS)
    return r_a.reshape(n_out, B, n_lwe), r_b.reshape(n_out, B)


def bootstrap_batch(okey, tvs, x_a, x_b, theta, n_out, lut_index=None):
    return keyswitch(okey, woks_batch(okey, tvs, x_a, x_b, theta, n_out, lut_index))


# ---- the seeded decode cases (p, theta, n_out): DESIGN.md §3.3's noise budget
DECODE_CASES = [(4, 1, 2), (8, 1, 2), (4, 2, 4)]
_decode_cache = {}


def decode_case(keyset, p, theta, n_out, B=48):
    """B fresh encryptions of random messages in [0, p) and n_out random functions f_r: [0, p) ->
    [0, p), each encoded at (2 f_r(m) + 1) / (4p), interleaved in one test vector; fixed seed.
    -> (msgs, f [n_out][p], tv, x_a, x_b)"""
    import tfhe_amd as T
    key = (p, theta, n_out)
    if key not in _decode_cache:
        rng = np.random.default_rng(3000 + 100 * p + 10 * theta + n_out)
        msgs = rng.integers(0, p, B)
        f = rng.integers(0, p, (n_out, p))
        tv = T.lut_table_many(p, T.lut_encode(f, p), theta)
        x_a, x_b = keyset.encrypt_digits(msgs, p, rng)
        _decode_cache[key] = [msgs, f, tv, x_a, x_b, None]
    return tuple(_decode_cache[key][:5])


def decode_expected(keyset, okey, p, theta, n_out):
    """the oracle's key-switched results for decode_case (computed once per process)"""
    key = (p, theta, n_out)
    _, _, tv, x_a, x_b = decode_case(keyset, p, theta, n_out)
    if _decode_cache[key][5] is None:
        _decode_cache[key][5] = bootstrap_batch(okey, tv, x_a, x_b, theta, n_out)
    return _decode_cache[key][5]


def switched_phase(keyset, x_a, x_b, theta):
    """the phase (torus, in [0, 1)) the blind rotation sees: (barb - sum_i bara_i s_i) / 2N"""
    s = keyset.lwe_key.astype(np.int64)
    ph = (bar(x_b, theta).astype(np.int64) - bar(x_a, theta).astype(np.int64) @ s) % (2 * N)
    return ph / (2.0 * N)


# ---- circuits
def eval_circuit(C, okey, inputs, B):
    """Node-by-node evaluation of a circuit with many-LUT nodes (and LUT / gate / lincomb / NOT /
    COPY / CONST nodes, as lut_oracle.eval_circuit; no MUX): every wire an LWE sample, nothing
    folded.  inputs: {wire: (a [B][500], b [B])}; returns {wire: (a, b)} for every wire."""
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
                W[w] = LO.lin(0, [(-1 if gate == 13 else 1, W[ins[0]])], B)
        elif gate == LUT_MANY_GATE:
            table, c0, theta, n_out, index = C.lut_many_node(w)
            if index:
                continue   # filled with the node's first wire
            x = LO.lin(c0, [(s[k], W[ins[k]]) for k in range(3) if ins[k] >= 0 and s[k] != 0], B)
            r_a, r_b = bootstrap_batch(okey, C.lut_table_get(table), x[0], x[1], theta, n_out)
            for f in range(n_out):
                W[w + f] = (r_a[f], r_b[f])
        else:
            assert gate != 10, "MUX: use circuit_oracle.eval_circuit"
            if gate == LO.LUT_GATE:
                table, c0 = C.lut_node(w)
                tv = C.lut_table_get(table)
            else:
                tv = np.full(N, LO.E8, np.int32)
            x = LO.lin(c0, [(s[k], W[ins[k]]) for k in range(3) if ins[k] >= 0 and s[k] != 0], B)
            W[w] = LO.bootstrap_batch(okey, tv, x[0], x[1])
    return W


P = 8
Q27 = 1 << 27   # 1/(4p) of the torus for p = 8


def adder():
    """The 2-digit radix-4 adder of test_lut_gpu.py's _adder with ONE many-LUT row (theta = 1,
    n_out = 2) per digit: the interleaved table holds x & 3 and x >> 2 at p = 8.  Level 1 also
    holds the NAND row, a plain LUT row and a lut_many(theta = 2, n_out = 3) row on random tables."""
    import tfhe_amd as T
    rng = np.random.default_rng(4242)
    C = T.Circuit()
    a0, a1, b0, b1, e0, e1 = C.inputs(6)
    x = np.arange(P)
    t_add = C.lut_table(T.lut_table_many(P, np.stack([T.lut_encode(x & 3, P), T.lut_encode(x >> 2, P)]), 1))
    t_r1 = C.lut_table(rng.integers(-2**31, 2**31, N, dtype=np.int64).astype(np.int32))
    t_r2 = C.lut_table(rng.integers(-2**31, 2**31, N, dtype=np.int64).astype(np.int32))
    s0 = C.lut_many(t_add, 1, 2, -Q27, 1, a0, 1, b0)
    c0 = s0 + 1
    nand = C.gate("NAND", e0, e1)
    r1 = C.lut(t_r1, 0x01234567, 1, a0, -1, b1)
    m0 = C.lut_many(t_r2, 2, 3, -0x0BADCAFE, 1, b0, 2, a1)
    s1 = C.lut_many(t_add, 1, 2, -2 * Q27, 1, a1, 1, b1, 1, c0)
    c1 = s1 + 1
    return C, (a0, a1, b0, b1, e0, e1), (s0, c0, nand, s1, c1), (r1, m0, m0 + 1, m0 + 2)


_adder_cache = {}


def adder_case(keyset, okey, B):
    """inputs and the node-by-node oracle evaluation of the adder for B instances (once per B)"""
    if B not in _adder_cache:
        rng = np.random.default_rng(5200 + B)
        C, ins, outs, extra = adder()
        digits = [rng.integers(0, 4, B) for _ in range(4)]
        bits = [rng.integers(0, 2, B) for _ in range(2)]
        enc = [keyset.encrypt_digits(d, P, rng) for d in digits] + [keyset.encrypt(b, rng) for b in bits]
        W = eval_circuit(C, okey, dict(zip(ins, enc)), B)
        _adder_cache[B] = (C, ins, outs, digits, bits, enc, W)
    return _adder_cache[B]


def adder_decoded(keyset, case, W):
    """(sum, carry of digit 0, NAND) decoded from the wires W = {wire: (a, b)} of the adder"""
    import tfhe_amd as T
    C, ins, outs, digits, bits, enc, _ = case
    s0, c0, nand, s1, c1 = outs
    dec = {w: T.lut_decode(keyset.phase(*W[w]), P) for w in (s0, c0, s1, c1)}
    return dec[s0] + 4 * dec[s1] + 16 * dec[c1], dec[c0], keyset.decrypt(*W[nand])


def adder_truth(case):
    C, ins, outs, digits, bits, enc, _ = case
    a = digits[0] + 4 * digits[1]
    b = digits[2] + 4 * digits[3]
    return a + b, (digits[0] + digits[2]) >> 2, 1 - (bits[0] & bits[1])
