"""One-rotation adder cells on the CPU oracle (TEST INFRASTRUCTURE: the expected
values of tests/test_fa.py and tests/test_fa_gpu.py).

The cell is a many-LUT bootstrap (tests/many_lut_oracle.py) at p = 4, theta = 1, n_out = 2 of
(0, -(k - 1)/16) + a + b (+ c) over half-torus bits (H: 1/16 for 0, 3/16 for 1); the truth tables
and the four test vectors are written out here independently of the library's.  eval_circuit
evaluates a circuit node by node like many_lut_oracle.eval_circuit, extended to affine nodes
(gate code -4), and hands the oracle every row whose inputs are known in ONE threaded batch, so a
small B still fills the thread pool."""
import numpy as np

import lut_oracle as LO
import many_lut_oracle as MO
import oracle_ctypes as O

N, n_lwe = O.N, O.n_lwe
AFFINE_GATE = -4
G, H = 0, 1                      # TFHE_AMD_ENC_GATE, TFHE_AMD_ENC_HALF
E8, E16 = 1 << 29, 1 << 28       # 1/8, 1/16
P, THETA = 4, 1
wrap = LO.wrap


def enc_bit(enc, bit):
    """Torus32 of a bit in encoding enc: G -1/8, +1/8; H 1/16, 3/16"""
    bit = np.asarray(bit)
    return np.where(bit != 0, 3 * E16, E16).astype(np.int32) if enc == H else \
        np.where(bit != 0, E8, -E8).astype(np.int32)


def cell_truth(m):
    """(sum bit, carry bit) of m = a + b + c in [0, 3]"""
    m = np.asarray(m)
    return m & 1, m >> 1


def cell_values(enc_sum, enc_carry):
    """the two functions of the cell over the p = 4 boxes, as Torus32 words: [2][4]"""
    s, c = cell_truth(np.arange(P))
    return np.stack([enc_bit(enc_sum, s), enc_bit(enc_carry, c)])


def cell_table(enc_sum, enc_carry):
    """the cell's test vector written out by hand: coefficient j holds function j mod 2 of box
    floor(4 j / N)"""
    v = cell_values(enc_sum, enc_carry)
    j = np.arange(N)
    return v[j & 1, (j * P) // N].astype(np.int32)


def cell_input(a, b, c=None):
    """the blind-rotation input (0, -(k - 1)/16) + a + b (+ c) over samples (a [B][500], b [B])"""
    terms = [(1, a), (1, b)] + ([(1, c)] if c is not None else [])
    return LO.lin(-(len(terms) - 1) * E16, terms, a[1].shape[0])


def cell(okey, enc_sum, enc_carry, a, b, c=None):
    """the oracle's key-switched cell outputs -> (r_a [2][B][500], r_b [2][B])"""
    x = cell_input(a, b, c)
    return MO.bootstrap_batch(okey, cell_table(enc_sum, enc_carry), x[0], x[1], THETA, 2)


def half_phase_error(keyset, x, m):
    """signed distance (torus, float) of the phases of samples x from the centre of box m at p = 4"""
    ph = keyset.phase(*x).astype(np.int64) - (2 * np.asarray(m, dtype=np.int64) + 1) * E16
    return ((ph + 2**31) % 2**32 - 2**31) / 2.0**32


def decode(keyset, enc, x):
    """the bit of samples x in encoding enc (H: the p = 4 box, 2 or 3 mean the phase left the boxes)"""
    import tfhe_amd as T
    return T.lut_decode(keyset.phase(*x), P) if enc == H else keyset.decrypt(*x)


# ---- circuits
def eval_circuit(C, okey, inputs, B):
    """Node-by-node evaluation (nothing folded): inputs {wire: (a [B][500], b [B])} -> {wire: (a, b)}
    for every wire.  Gate / lincomb / LUT / many-LUT / NOT / COPY / CONST / affine nodes; no MUX."""
    n_w = C.info()["wires"]
    W = {}
    tables = {}
    pending = []   # (first wire, n_out, theta or None, table key, x)

    def table(key):
        if key not in tables:
            tables[key] = np.full(N, LO.E8, np.int32) if key is None else C.lut_table_get(key)
        return tables[key]

    def flush():
        groups = {}
        for job in pending:
            groups.setdefault((job[2], job[1]), []).append(job)
        for (theta, n_out), jobs in groups.items():
            keys = sorted({j[3] for j in jobs}, key=lambda k: -1 if k is None else k)
            tvs = np.stack([table(k) for k in keys])
            idx = np.concatenate([np.full(B, keys.index(j[3]), np.int64) for j in jobs])
            x_a = np.concatenate([j[4][0] for j in jobs])
            x_b = np.concatenate([j[4][1] for j in jobs])
            if theta is None:
                r_a, r_b = LO.bootstrap_batch(okey, tvs, x_a, x_b, idx)
                r_a, r_b = r_a[None], r_b[None]
            else:
                r_a, r_b = MO.bootstrap_batch(okey, tvs, x_a, x_b, theta, n_out, idx)
            for i, j in enumerate(jobs):
                for f in range(n_out):
                    W[j[0] + f] = (r_a[f, i * B:(i + 1) * B], r_b[f, i * B:(i + 1) * B])
        pending.clear()

    def wire(w):
        if w not in W:
            flush()
        return W[w]

    for w in range(n_w):
        kind, gate, c0, s, ins = C.node(w)
        if kind == 0:
            W[w] = tuple(np.asarray(v, dtype=np.int32) for v in inputs[w])
        elif kind == 2:
            if gate == 15:
                W[w] = (np.zeros((B, n_lwe), np.int32), np.full(B, c0, np.int32))
            elif gate == AFFINE_GATE:
                W[w] = LO.lin(c0, [(s[0], wire(ins[0]))], B)
            else:
                W[w] = LO.lin(0, [(-1 if gate == 13 else 1, wire(ins[0]))], B)
        else:
            assert gate != 10, "MUX: use circuit_oracle.eval_circuit"
            theta, n_out, key = None, 1, None
            if gate == MO.LUT_MANY_GATE:
                key, c0, theta, n_out, index = C.lut_many_node(w)
                if index:
                    continue   # filled with the node's first wire
            elif gate == LO.LUT_GATE:
                key, c0 = C.lut_node(w)
            x = LO.lin(c0, [(s[k], wire(ins[k])) for k in range(3) if ins[k] >= 0 and s[k] != 0], B)
            pending.append((w, n_out, theta, key, x))
    flush()
    return W


# ---- the seeded circuit cases shared by the CPU and the GPU tests
_cache = {}


def mul_case(keyset, okey, nbits, B, seed=None):
    """mul_fa nbits x nbits over B operand pairs: random, then (0, 0), (max, max), (max, 1) in the
    last three instances when B >= 4 -> (C, a wires, b wires, prod wires, x, y, enc, W)"""
    import tfhe_amd as T
    key = ("mul", nbits, B)
    if key not in _cache:
        rng = np.random.default_rng(7100 + 10 * nbits + B if seed is None else seed)
        top = (1 << nbits) - 1
        x, y = rng.integers(0, top + 1, B), rng.integers(0, top + 1, B)
        if B >= 4:
            x[-3:], y[-3:] = (0, top, top), (0, top, 1)
        C = T.Circuit()
        a, b = C.inputs(nbits), C.inputs(nbits)
        prod = C.mul_fa(a, b)
        enc = {w: keyset.encrypt(p, rng) for w, p in zip(a + b, T.bits_of(x, nbits) + T.bits_of(y, nbits))}
        _cache[key] = (C, a, b, prod, x, y, enc, eval_circuit(C, okey, enc, B))
    return _cache[key]


def dot_case(keyset, okey, B):
    """dot_fa of 2 terms x 3 bits into 8 bits -> (C, a terms, b terms, out wires, x [B][2], y [B][2], enc, W)"""
    import tfhe_amd as T
    key = ("dot", B)
    if key not in _cache:
        rng = np.random.default_rng(7200 + B)
        x, y = rng.integers(0, 8, (B, 2)), rng.integers(0, 8, (B, 2))
        x[0], y[0] = (7, 7), (7, 7)
        C = T.Circuit()
        a = [C.inputs(3) for _ in range(2)]
        b = [C.inputs(3) for _ in range(2)]
        out = C.dot_fa(a, b, 8)
        enc = {}
        for t in range(2):
            for w, p in zip(a[t] + b[t], T.bits_of(x[:, t], 3) + T.bits_of(y[:, t], 3)):
                enc[w] = keyset.encrypt(p, rng)
        _cache[key] = (C, a, b, out, x, y, enc, eval_circuit(C, okey, enc, B))
    return _cache[key]


def add_half_case(keyset, okey, B):
    """4-bit operands as gate bits -> to_half -> add_half with the sums in G and a second add_half
    chained on H sums -> (C, info, x, y, enc, W); info = dict of wire lists"""
    import tfhe_amd as T
    key = ("add_half", B)
    if key not in _cache:
        rng = np.random.default_rng(7300 + B)
        x, y = rng.integers(0, 16, B), rng.integers(0, 16, B)
        x[0], y[0] = 15, 15
        C = T.Circuit()
        a, b = C.inputs(4), C.inputs(4)
        ha, hb = [C.to_half(w) for w in a], [C.to_half(w) for w in b]
        sum_g, carry_g = C.add_half(ha, hb, enc_out=T.ENC_GATE)
        sum_h, carry_h = C.add_half(ha, hb, enc_out=T.ENC_HALF)
        sum2, carry2 = C.add_half(sum_h, ha, carry_in=carry_h, enc_out=T.ENC_GATE)   # (x + y) mod 16 + x + carry
        enc = {w: keyset.encrypt(p, rng) for w, p in zip(a + b, T.bits_of(x, 4) + T.bits_of(y, 4))}
        info = dict(ha=ha, hb=hb, sum_g=sum_g, carry_g=carry_g, sum_h=sum_h, carry_h=carry_h, sum2=sum2, carry2=carry2)
        _cache[key] = (C, info, x, y, enc, eval_circuit(C, okey, enc, B))
    return _cache[key]
