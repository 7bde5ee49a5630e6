"""tests/dag_oracle.py, the one evaluator for every node kind, equals each of the three older
evaluators word for word on a circuit that one can evaluate (CPU only): circuit_oracle on gates and
MUX, lut_oracle on LUT rows, many_lut_oracle on many-LUT rows, fa_oracle on adder cells and affine
nodes.  The older modules' cached cases are reused, so only the new evaluator runs twice."""
import numpy as np

import circuit_oracle
import dag_oracle as DO
import fa_oracle as FO
import lut_oracle as LO
import many_lut_oracle as MO
import tfhe_amd as T


def _same_wires(got, want, what):
    assert sorted(got) == sorted(want), what
    for w in want:
        assert got[w][0].dtype == np.int32 and got[w][1].dtype == np.int32, (what, w)
        assert got[w][0].shape == want[w][0].shape and got[w][1].shape == want[w][1].shape, (what, w)
        assert np.array_equal(got[w][0], want[w][0]) and np.array_equal(got[w][1], want[w][1]), (what, w)


def test_equals_circuit_oracle_on_gates_and_mux(keyset, okey):
    """8-bit minmax: the comparison tree (gate and lincomb rows) and one level of MUXes; plus NOT,
    COPY, CONST and a MUX over them"""
    rng = np.random.default_rng(9101)
    B, n = 2, 8
    C = T.Circuit()
    a, b = C.inputs(n), C.inputs(n)
    mn = C.minmax(a, b)
    C.gate("MUX", C.gate("NOT", mn[0]), C.gate("CONST", 1), C.gate("COPY", a[3]))
    x, y = rng.integers(0, 2**n, B), rng.integers(0, 2**n, B)
    enc = {w: keyset.encrypt(p, rng) for w, p in zip(a + b, T.bits_of(x, n) + T.bits_of(y, n))}
    want = circuit_oracle.eval_circuit(C, okey, enc, B)
    got = DO.eval_circuit(C, okey, enc, B)
    _same_wires(got, want, "minmax")
    assert np.array_equal(T.int_of([keyset.decrypt(*got[w]) for w in mn]), np.minimum(x, y))


def test_equals_lut_oracle_on_the_radix4_adder(keyset, okey):
    """the 2-digit radix-4 adder of tests/test_lut_gpu.py: LUT rows of two tables and a NAND row"""
    rng = np.random.default_rng(9102)
    B, P, Q27 = 3, 8, 1 << 27
    C = T.Circuit()
    a0, a1, b0, b1, e0, e1 = C.inputs(6)
    x = np.arange(P)
    t_sum = C.lut_table(T.lut_table(P, T.lut_encode(x & 3, P)))
    t_car = C.lut_table(T.lut_table(P, T.lut_encode(x >> 2, P)))
    s0 = C.lut(t_sum, -Q27, 1, a0, 1, b0)
    c0 = C.lut(t_car, -Q27, 1, a0, 1, b0)
    C.gate("NAND", e0, e1)
    s1 = C.lut(t_sum, -2 * Q27, 1, a1, 1, b1, 1, c0)
    c1 = C.lut(t_car, -2 * Q27, 1, a1, 1, b1, 1, c0)
    digits = [rng.integers(0, 4, B) for _ in range(4)]
    enc = [keyset.encrypt_digits(d, P, rng) for d in digits] + [keyset.encrypt(rng.integers(0, 2, B), rng) for _ in range(2)]
    enc = dict(zip((a0, a1, b0, b1, e0, e1), enc))
    got = DO.eval_circuit(C, okey, enc, B)
    _same_wires(got, LO.eval_circuit(C, okey, enc, B), "radix-4 adder")
    dec = [T.lut_decode(keyset.phase(*got[w]), P) for w in (s0, s1, c1)]
    assert np.array_equal(dec[0] + 4 * dec[1] + 16 * dec[2], digits[0] + 4 * digits[1] + digits[2] + 4 * digits[3])


def test_equals_many_lut_oracle_on_its_adder(keyset, okey):
    C, ins, outs, digits, bits, enc, W = MO.adder_case(keyset, okey, 5)
    _same_wires(DO.eval_circuit(C, okey, dict(zip(ins, enc)), 5), W, "many-LUT adder")


def test_equals_fa_oracle_on_add_half(keyset, okey):
    C, info, x, y, enc, W = FO.add_half_case(keyset, okey, 5)
    _same_wires(DO.eval_circuit(C, okey, enc, 5), W, "add_half")


def test_known_wires_are_kept_and_only_the_rest_is_computed(keyset, okey):
    """a circuit that grew: the wires handed in are returned as they are"""
    C, info, x, y, enc, W = FO.add_half_case(keyset, okey, 5)
    cut = max(W) - 3
    while C.node(cut + 1)[1] == DO.LUT_MANY_GATE and C.lut_many_node(cut + 1)[4] > 0:
        cut -= 1                                               # whole nodes only
    known = {w: v for w, v in W.items() if w <= cut}
    got = DO.eval_circuit(C, okey, enc, 5, known=known)
    assert all(got[w] is known[w] for w in known)
    _same_wires(got, W, "add_half from known wires")
