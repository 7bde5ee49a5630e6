"""One-rotation adder cells without a GPU: the tables, the conversions, the argument
checks, the builders' host logic against the gate builders, the noise condition the GPU decode
tests rest on, and decoding through the CPU oracle (tests/fa_oracle.py)."""
import ctypes

import numpy as np
import pytest

import fa_oracle as FO
import lut_oracle as LO
import tfhe_amd as T

N, n_lwe = 1024, 500
E_ARG = -1
ENCS = [(s, c) for s in (T.ENC_GATE, T.ENC_HALF) for c in (T.ENC_GATE, T.ENC_HALF)]


# ---------------------------------------------------------------- tables

@pytest.mark.parametrize("enc_sum,enc_carry", ENCS)
def test_tables(enc_sum, enc_carry):
    tv = T.full_add_table(enc_sum, enc_carry)
    m = np.arange(4)
    word = {T.ENC_GATE: lambda b: np.where(b != 0, T.MU, -T.MU), T.ENC_HALF: lambda b: T.lut_encode(b, 4)}
    want = T.lut_table_many(4, np.stack([word[enc_sum](m & 1), word[enc_carry](m >> 1)]), 1)
    assert np.array_equal(tv, want)
    assert np.array_equal(tv, FO.cell_table(enc_sum, enc_carry))
    # the circuit registers the same table, once, however many cells use it
    C = T.Circuit()
    a, b, c = C.inputs(3)
    s0, c0 = C.full_add(a, b, c, enc_sum, enc_carry)
    s1, c1 = C.full_add(a, b, -1, enc_sum, enc_carry)
    s2, none = C.full_add(a, b, c, enc_sum, enc_carry, carry=False)
    assert (c0, c1, none) == (s0 + 1, s1 + 1, None) and s2 == c1 + 1
    t0, k0, theta, n_out, ix = C.lut_many_node(s0)
    assert (theta, n_out, ix, k0) == (1, 2, 0, -2 * FO.E16)
    assert C.lut_many_node(c0)[4] == 1
    assert C.lut_many_node(s1)[:4] == (t0, -FO.E16, 1, 2)
    assert C.lut_many_node(s2)[:4] == (t0, -2 * FO.E16, 1, 1)
    assert np.array_equal(C.lut_table_get(t0), tv)
    assert C.node(s0)[3:] == ([1, 1, 1], [a, b, c]) and C.node(s1)[3:] == ([1, 1, 0], [a, b, -1])
    assert C.info() == {"wires": 8, "gates": 3, "bootstraps": 3, "depth": 1}
    with pytest.raises(T.TfheAmdError):
        C.lut_table_get(t0 + 1)


def test_half_encoding_is_the_p4_convention():
    assert np.array_equal(T.half_encode([0, 1]), T.lut_encode([0, 1], 4))
    assert [int(v) for v in T.half_encode([0, 1])] == [1 << 28, 3 << 28] == [T.H0, T.H1]


def test_a_circuit_holds_at_most_five_tables():
    C = T.Circuit()
    a, b = C.inputs(2)
    ha, hb, hc = C.to_half(a), C.to_half(b), C.and_half(a, b)
    for _ in range(2):
        for es, ec in ENCS:
            C.full_add(ha, hb, hc, es, ec)
    for t in range(5):
        C.lut_table_get(t)
    with pytest.raises(T.TfheAmdError):
        C.lut_table_get(5)
    assert np.array_equal(C.lut_table_get(C.lut_node(ha - 1)[0]), np.full(N, 1 << 28, np.int32))


# ---------------------------------------------------------------- nodes and argument errors

def test_affine_node():
    C = T.Circuit()
    a, = C.inputs(1)
    w = C.affine(0x12345678, -3, a)
    assert C.node(w) == (2, T.AFFINE_GATE, 0x12345678, [-3, 0, 0], [a, -1, -1])
    v = C.affine(-5, 7, w)        # affine of affine folds: 7 (c + s a) - 5
    g = C.lincomb(11, 2, v)
    assert C.info() == {"wires": 4, "gates": 3, "bootstraps": 1, "depth": 1}
    assert C.level_sizes() == [0, 1]
    z = C.affine(9, 0, a)         # s = 0: the trivial sample
    assert C.node(z)[2:4] == (9, [0, 0, 0])
    assert C.info()["bootstraps"] == 1
    assert g == 3


def test_conversion_nodes():
    C = T.Circuit()
    a, b = C.inputs(2)
    h = C.to_half(a)
    assert C.node(h) == (2, T.AFFINE_GATE, T.MU, [1, 0, 0], [h - 1, -1, -1])
    assert C.node(h - 1)[:2] == (1, T.LUT_GATE) and C.lut_node(h - 1)[1] == 0
    assert C.node(h - 1)[3:] == ([1, 0, 0], [a, -1, -1])
    g = C.to_gate(h)
    assert C.node(g) == (2, T.AFFINE_GATE, -(1 << 30), [2, 0, 0], [h, -1, -1])
    p = C.and_half(a, b)
    assert C.node(p)[:3] == (2, T.AFFINE_GATE, T.MU) and C.lut_node(p - 1)[1] == -T.MU
    assert C.node(p - 1)[3:] == ([1, 1, 0], [a, b, -1])
    assert C.info() == {"wires": 7, "gates": 5, "bootstraps": 2, "depth": 1}


def test_argument_errors():
    lib = T.lib
    C = T.Circuit()
    a, b, c = C.inputs(3)
    n0 = C.info()["wires"]
    ip = ctypes.c_int
    s, co = ip(), ip()
    for bad in (-1, 3, 99):
        assert lib.tfhe_amd_circuit_affine(C.h, 0, 1, bad) == E_ARG
        assert lib.tfhe_amd_circuit_to_gate(C.h, bad) == E_ARG
        assert lib.tfhe_amd_circuit_to_half(C.h, bad) == E_ARG
        assert lib.tfhe_amd_circuit_and_half(C.h, a, bad) == E_ARG
        assert lib.tfhe_amd_circuit_and_half(C.h, bad, a) == E_ARG
        assert lib.tfhe_amd_circuit_full_add(C.h, bad, b, c, 1, 1, ctypes.byref(s), ctypes.byref(co)) == E_ARG
        assert lib.tfhe_amd_circuit_full_add(C.h, a, bad, c, 1, 1, ctypes.byref(s), ctypes.byref(co)) == E_ARG
    for bad in (-2, 3, 99):
        assert lib.tfhe_amd_circuit_full_add(C.h, a, b, bad, 1, 1, ctypes.byref(s), ctypes.byref(co)) == E_ARG
    for es, ec in ((2, 0), (0, 2), (-1, 1), (1, -1)):
        assert lib.tfhe_amd_circuit_full_add(C.h, a, b, c, es, ec, ctypes.byref(s), ctypes.byref(co)) == E_ARG
        assert lib.tfhe_amd_circuit_full_add(C.h, a, b, c, es, ec, ctypes.byref(s), None) == E_ARG
        assert lib.tfhe_amd_full_add_table(T._p(np.zeros(N, np.int32)), es, ec) == E_ARG
    assert lib.tfhe_amd_circuit_full_add(C.h, a, b, c, 1, 1, None, ctypes.byref(co)) == E_ARG
    assert lib.tfhe_amd_full_add_table(None, 0, 0) == E_ARG
    for fn in (lib.tfhe_amd_circuit_affine, ):
        assert fn(None, 0, 1, 0) == E_ARG
    assert lib.tfhe_amd_circuit_to_gate(None, 0) == E_ARG and lib.tfhe_amd_circuit_to_half(None, 0) == E_ARG
    assert lib.tfhe_amd_circuit_and_half(None, 0, 0) == E_ARG
    assert lib.tfhe_amd_circuit_full_add(None, 0, 0, 0, 1, 1, ctypes.byref(s), ctypes.byref(co)) == E_ARG
    # the vector builders
    ids, out = T._ids([a, b]), (ip * 8)()
    bad_ids = T._ids([a, 99])
    for fn in (lib.tfhe_amd_circuit_mul_fa, ):
        assert fn(None, 2, ids, ids, out) == E_ARG and fn(C.h, 0, ids, ids, out) == E_ARG
        assert fn(C.h, 2, None, ids, out) == E_ARG and fn(C.h, 2, ids, None, out) == E_ARG
        assert fn(C.h, 2, ids, ids, None) == E_ARG
        assert fn(C.h, 2, bad_ids, ids, out) == E_ARG and fn(C.h, 2, ids, bad_ids, out) == E_ARG
    dot = lib.tfhe_amd_circuit_dot_fa
    assert dot(None, 1, 2, ids, ids, 4, out) == E_ARG and dot(C.h, 0, 2, ids, ids, 4, out) == E_ARG
    assert dot(C.h, 1, 0, ids, ids, 4, out) == E_ARG and dot(C.h, 1, 2, ids, ids, 0, out) == E_ARG
    assert dot(C.h, 1, 2, None, ids, 4, out) == E_ARG and dot(C.h, 1, 2, ids, None, 4, out) == E_ARG
    assert dot(C.h, 1, 2, ids, ids, 4, None) == E_ARG and dot(C.h, 1, 2, bad_ids, ids, 4, out) == E_ARG
    add = lib.tfhe_amd_circuit_add_half
    assert add(None, 2, ids, ids, -1, 1, out) == E_ARG and add(C.h, 0, ids, ids, -1, 1, out) == E_ARG
    assert add(C.h, 2, None, ids, -1, 1, out) == E_ARG and add(C.h, 2, ids, None, -1, 1, out) == E_ARG
    assert add(C.h, 2, ids, ids, -1, 1, None) == E_ARG and add(C.h, 2, ids, ids, -1, 2, out) == E_ARG
    assert add(C.h, 2, ids, ids, 99, 1, out) == E_ARG and add(C.h, 2, ids, ids, -2, 1, out) == E_ARG
    assert add(C.h, 2, bad_ids, ids, -1, 1, out) == E_ARG
    # nothing was added by any refused call, not even a table
    assert C.info()["wires"] == n0
    with pytest.raises(T.TfheAmdError):
        C.lut_table_get(0)
    # the batch forms refuse before they touch a device (a null context included)
    z = np.zeros((2, n_lwe), np.int32)
    zb = np.zeros(2, np.int32)
    r_a, r_b = np.zeros((2, 2, n_lwe), np.int32), np.zeros((2, 2), np.int32)
    p = T._p
    assert lib.tfhe_amd_full_add_batch_host(None, 2, 1, 1, p(z), p(zb), p(z), p(zb), None, None, p(r_a), p(r_b)) == E_ARG
    assert lib.tfhe_amd_full_add_batch_dev(None, 2, 1, 1, None, None, None, None, None, None, None, None, None) == E_ARG


# ---------------------------------------------------------------- host logic

def _pair(n, fa):
    C = T.Circuit()
    a, b = C.inputs(n), C.inputs(n)
    (C.mul_fa if fa else C.mul)(a, b)
    return C


def _dot(fa, nterms=3, nbits=4, out_bits=10):
    C = T.Circuit()
    a = [C.inputs(nbits) for _ in range(nterms)]
    b = [C.inputs(nbits) for _ in range(nterms)]
    (C.dot_fa if fa else C.dot)(a, b, out_bits)
    return C


def _cells(C):
    n = 0
    for w in range(C.info()["wires"]):
        kind, gate, c0, s, ins = C.node(w)
        n += gate == T.LUT_MANY_GATE and C.lut_many_node(w)[4] == 0
    return n


@pytest.mark.parametrize("case", [2, 3, 4, 8, 16, "dot"])
def test_same_depth_one_bootstrap_less_per_cell(case):
    gates, fa = (_dot(False), _dot(True)) if case == "dot" else (_pair(case, False), _pair(case, True))
    ig, ifa = gates.info(), fa.info()
    assert ifa["depth"] == ig["depth"]
    cells = _cells(fa)
    assert ig["bootstraps"] - ifa["bootstraps"] == cells
    assert cells > 0 or case == 2
    # level by level: the same rows, less one per cell
    lg, lf = gates.level_sizes(), fa.level_sizes()
    assert len(lg) == len(lf) and lg[1] == lf[1] and all(f <= g for f, g in zip(lf, lg))
    print(case, "bootstraps", ig["bootstraps"], "->", ifa["bootstraps"], "cells", cells, "depth", ig["depth"])


# info() and level_sizes() of the gate builders as the parent commit gives them: these builders must
# emit exactly the circuits they emitted before the one-rotation cells existed
PARENT = {
    ("mul", 2): ((28, 24, 23, 5), [0, 6, 6, 5, 5, 1]),
    ("add", 2): ((8, 4, 4, 2), [0, 2, 2]),
    ("add_prefix", 2): ((11, 7, 7, 2), [0, 4, 3]),
    ("mul", 3): ((51, 45, 44, 7), [0, 11, 8, 9, 7, 3, 5, 1]),
    ("add", 3): ((12, 6, 6, 3), [0, 2, 2, 2]),
    ("add_prefix", 3): ((18, 12, 12, 3), [0, 6, 3, 3]),
    ("mul", 4): ((84, 76, 75, 8), [0, 18, 10, 11, 11, 7, 6, 9, 3]),
    ("add", 4): ((16, 8, 8, 4), [0, 2, 2, 2, 2]),
    ("add_prefix", 4): ((27, 19, 19, 4), [0, 8, 5, 5, 1]),
    ("mul", 8): ((276, 260, 259, 11), [0, 66, 36, 25, 23, 23, 22, 15, 14, 11, 17, 7]),
    ("add", 8): ((32, 16, 16, 8), [0, 2, 2, 2, 2, 2, 2, 2, 2]),
    ("add_prefix", 8): ((63, 47, 47, 5), [0, 16, 9, 9, 10, 3]),
    ("mul", 16): ((964, 932, 931, 14), [0, 258, 154, 91, 79, 67, 50, 47, 40, 19, 29, 28, 21, 33, 15]),
    ("add", 16): ((64, 32, 32, 16), [0] + [2] * 16),
    ("add_prefix", 16): ((143, 111, 111, 6), [0, 32, 17, 17, 18, 20, 7]),
    ("dot", 0): ((208, 184, 183, 12), [0, 50, 28, 14, 16, 12, 15, 15, 9, 6, 9, 8, 1]),
}


@pytest.mark.parametrize("name,n", sorted(PARENT))
def test_existing_builders_emit_what_they_emitted(name, n):
    if name == "dot":
        C = _dot(False)
    else:
        C = T.Circuit()
        a, b = C.inputs(n), C.inputs(n)
        getattr(C, name)(a, b)
    i = C.info()
    assert ((i["wires"], i["gates"], i["bootstraps"], i["depth"]), C.level_sizes()) == PARENT[(name, n)]
    assert not any(C.node(w)[1] in (T.LUT_GATE, T.LUT_MANY_GATE, T.AFFINE_GATE) for w in range(i["wires"]))


def test_matvec_matmat_keyword():
    import matmat
    import matvec
    for mod, args in ((matvec, (3, 4)), (matmat, (3, 4, True))):
        plain, fa = mod.build(T, *args)[0], mod.build(T, *args, fa=True)[0]
        assert _cells(plain) == 0 and plain.info() == _dot(False).info()
        assert fa.info() == _dot(True).info() and _cells(fa) > 0


# ---------------------------------------------------------------- through the oracle

def test_conversions_through_the_oracle(keyset, okey):
    rng = np.random.default_rng(7001)
    B = 8
    bits = np.array([0, 1, 0, 1, 1, 0, 1, 0])
    other = np.array([0, 0, 1, 1, 1, 1, 0, 0])
    C = T.Circuit()
    a, b = C.inputs(2)
    h = C.to_half(a)
    g = C.to_gate(h)
    p = C.and_half(a, b)
    pg = C.to_gate(p)
    W = FO.eval_circuit(C, okey, {a: keyset.encrypt(bits, rng), b: keyset.encrypt(other, rng)}, B)
    assert np.array_equal(FO.decode(keyset, FO.H, W[h]), bits)
    assert np.array_equal(FO.decode(keyset, FO.G, W[g]), bits)
    assert np.array_equal(FO.decode(keyset, FO.H, W[p]), bits & other)
    assert np.array_equal(FO.decode(keyset, FO.G, W[pg]), bits & other)
    # to_gate is exactly 2 H - 1/4, word for word
    assert np.array_equal(W[g][0], LO.wrap(2 * W[h][0].astype(np.int64)))
    assert np.array_equal(W[g][1], LO.wrap(2 * W[h][1].astype(np.int64) - (1 << 30)))
    # a bootstrapped H bit sits within 1/16 of its box centre, its G image within 1/8 of +-1/8
    assert np.max(np.abs(FO.half_phase_error(keyset, W[h], bits))) < 1 / 16
    # trivial (noiseless) samples, both bit values: the affine maps alone
    for bit in (0, 1):
        hw = int(T.half_encode(bit))
        assert LO.wrap(2 * hw - (1 << 30)) == (T.MU if bit else -T.MU)


def test_noise_condition_chain(keyset, okey):
    """The condition the GPU decode tests rest on: 8 levels x B = 128 cells whose THREE inputs are all
    bootstrapped (the previous level's sum and carry and a fresh and_half product bit), the last
    level emitted in the gate encoding.  Every cell's input phase stays within the box margin 1/16 and
    every output decodes.  No sample is left out.
    Measured with this seed: largest deviation 0.0234, r.m.s. 0.0076 of the margin 0.0625 (8.2 sigma);
    into gates after to_gate: largest 0.0303, r.m.s. 0.0082 of 0.125 (15 sigma)."""
    rng = np.random.default_rng(7400)
    B, levels = 128, 8
    sign = np.full(N, FO.E16, np.int32)

    def product():
        x, y = rng.integers(0, 2, B), rng.integers(0, 2, B)
        ex, ey = keyset.encrypt(x, rng), keyset.encrypt(y, rng)
        u = LO.lin(-T.MU, [(1, ex), (1, ey)], B)
        r = LO.bootstrap_batch(okey, sign, u[0], u[1])
        return x & y, LO.lin(T.MU, [(1, r)], B)

    (ma, a), (mb, b), (mc, c) = product(), product(), product()
    for m, x in ((ma, a), (mb, b), (mc, c)):
        assert np.array_equal(FO.decode(keyset, FO.H, x), m)
    dev, dev_gate = [], []
    for level in range(levels):
        last = level == levels - 1
        enc = FO.G if last else FO.H
        m = ma + mb + mc
        dev.append(FO.half_phase_error(keyset, FO.cell_input(a, b, c), m))
        r_a, r_b = FO.cell(okey, enc, enc, a, b, c)
        ms, mco = FO.cell_truth(m)
        s, co = (r_a[0], r_b[0]), (r_a[1], r_b[1])
        assert np.array_equal(FO.decode(keyset, enc, s), ms), level
        assert np.array_equal(FO.decode(keyset, enc, co), mco), level
        if not last:
            for mm, x in ((ms, s), (mco, co)):   # what a gate would see after to_gate
                g = LO.lin(-(1 << 30), [(2, x)], B)
                e = keyset.phase(*g).astype(np.int64) - np.where(mm != 0, T.MU, -T.MU)
                dev_gate.append(((e + 2**31) % 2**32 - 2**31) / 2.0**32)
            (ma, a), (mb, b), (mc, c) = (ms, s), (mco, co), product()
    dev, dev_gate = np.concatenate(dev), np.concatenate(dev_gate)
    print("cells %d: largest deviation %.4f, r.m.s. %.4f, margin %.4f (%.1f sigma)" %
          (dev.size, np.max(np.abs(dev)), np.sqrt(np.mean(dev**2)), 1 / 16, (1 / 16) / np.sqrt(np.mean(dev**2))))
    print("into gates after to_gate (%d bits): largest %.4f, r.m.s. %.4f, margin %.4f" %
          (dev_gate.size, np.max(np.abs(dev_gate)), np.sqrt(np.mean(dev_gate**2)), 1 / 8))
    assert dev.size == levels * B
    assert np.max(np.abs(dev)) < 1 / 16
    assert np.max(np.abs(dev_gate)) < 1 / 8


def test_radix4_cells_do_not_survive_bootstrapped_inputs(keyset, okey):
    """Why there are no radix-4 builders: a radix-4 digit with carry room (p = 8,
    theta = 1) built from bootstrapped terms, then digit + digit + bootstrapped carry.  The input's
    deviation from its box centre is measured against the margin 1/32; this records the figures and
    asserts only what the design rests on: the r.m.s. is above a fifth of the margin (under 5 sigma,
    against 7 for the one-bit cell), so cells fail at a rate no builder can carry.
    Measured with this seed: r.m.s. 0.0144, largest 0.0442 of the margin 0.0312 (2.2 sigma); 5 of
    256 inputs left their box."""
    rng = np.random.default_rng(7500)
    B, p = 256, 8
    q = (1 << 30) // p   # 1/(4p)

    def boot_bit():
        """a bootstrapped bit at weight 1/(2p): 0 -> 0, 1 -> 1/16 (+- noise), via a sign row"""
        m = rng.integers(0, 2, B)
        e = keyset.encrypt(m, rng)
        r = LO.bootstrap_batch(okey, np.full(N, q, np.int32), e[0], e[1])   # -+1/32
        return m, LO.lin(q, [(1, r)], B)   # 0 or 1/16

    def digit():
        """a radix-4 digit from two bootstrapped terms: d = b0 + 2 b1 at (2 d + 1)/32"""
        (m0, b0), (m1, b1) = boot_bit(), boot_bit()
        return m0 + 2 * m1, LO.lin(q, [(1, b0), (2, b1)], B)

    (md, d), (me, e), (mc, cin) = digit(), digit(), boot_bit()
    x = LO.lin(-q, [(1, d), (1, e), (1, cin)], B)   # (2 (d + e + c) + 1)/32
    m = md + me + mc
    ph = keyset.phase(*x).astype(np.int64) - (2 * m + 1) * q
    dev = ((ph + 2**31) % 2**32 - 2**31) / 2.0**32
    rms, worst, out = np.sqrt(np.mean(dev**2)), np.max(np.abs(dev)), int(np.sum(np.abs(dev) >= 1 / 32))
    print("radix-4 cell inputs %d: r.m.s. %.4f, largest %.4f, margin %.4f (%.1f sigma), %d left the box" %
          (dev.size, rms, worst, 1 / 32, (1 / 32) / rms, out))
    assert rms > (1 / 32) / 5


def test_decode_mul_fa(keyset, okey):
    C, a, b, prod, x, y, enc, W = FO.mul_case(keyset, okey, 4, 11)
    assert [(int(x[i]), int(y[i])) for i in (-3, -2, -1)] == [(0, 0), (15, 15), (15, 1)]
    got = T.int_of([keyset.decrypt(*W[w]) for w in prod])
    assert np.array_equal(got, x * y)
    # the partial products are H bits, the cells' outputs too
    for w in range(C.info()["wires"]):
        kind, gate, c0, s, ins = C.node(w)
        if gate == T.LUT_MANY_GATE:
            assert np.all(FO.decode(keyset, FO.H, W[w]) < 2), w


def test_decode_dot_fa(keyset, okey):
    C, a, b, out, x, y, enc, W = FO.dot_case(keyset, okey, 5)
    got = T.int_of([keyset.decrypt(*W[w]) for w in out])
    assert np.array_equal(got, (x * y).sum(axis=1) % 256)
    assert (x * y).sum(axis=1).max() == 98


def test_decode_add_half(keyset, okey):
    C, info, x, y, enc, W = FO.add_half_case(keyset, okey, 5)
    bits = lambda ws, e: [FO.decode(keyset, e, W[w]) for w in ws]
    assert np.array_equal(T.int_of(bits(info["sum_g"] + [info["carry_g"]], FO.G)), x + y)
    assert np.array_equal(T.int_of(bits(info["sum_h"] + [info["carry_h"]], FO.H)), x + y)
    assert np.array_equal(T.int_of(bits(info["sum2"] + [info["carry2"]], FO.G)), (x + y) % 16 + x + ((x + y) >> 4))
    assert C.info()["bootstraps"] == 8 + 3 * 4 and C.info()["depth"] == 1 + 4 + 4
