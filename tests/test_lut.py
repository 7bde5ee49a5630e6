"""Programmable bootstrapping, the parts that need no GPU: tfhe_amd_lut_fill, the circuit host
logic of LUT nodes, and the expected values themselves — the oracle composition of
tests/lut_oracle.py reproduces the oracle's own bootstrap for a constant table and decodes
every sample of the encoding convention (include/tfhe_amd.h) at the key-switch noise."""
import numpy as np
import pytest

import lut_oracle as LO
import tfhe_amd as T

E_ARG = -1
N = 1024


def test_lut_fill_layout_and_arguments():
    rng = np.random.default_rng(11)
    for p in (1, 4, 1024):
        values = rng.integers(-2**31, 2**31, p, dtype=np.int64).astype(np.int32)
        tv = T.lut_table(p, values)
        assert tv.shape == (N,) and tv.dtype == np.int32
        assert np.array_equal(tv, values[(np.arange(N) * p) // N]), p
    tv = np.full(N, 7, np.int32)
    values = np.arange(2048, dtype=np.int32)
    for p in (0, 3, 2048, -4):
        assert T.lib.tfhe_amd_lut_fill(T._p(tv), p, T._p(values)) == E_ARG, p
    assert np.all(tv == 7)
    assert T.lib.tfhe_amd_lut_fill(None, 4, T._p(values)) == E_ARG
    assert T.lib.tfhe_amd_lut_fill(T._p(tv), 4, None) == E_ARG
    with pytest.raises(T.TfheAmdError):
        T.lut_table(3, [1, 2, 3])


def test_encoding_helpers():
    for p in (1, 4, 8, 1024):
        m = np.arange(p)
        enc = T.lut_encode(m, p)
        # (2m + 1) / (4p) of the torus, exactly
        assert np.array_equal(enc.astype(np.int64) * 4 * p, (2 * m + 1) * 2**32)
        assert np.array_equal(T.lut_decode(enc, p), m)
        half = (1 << 30) // p   # 1/(4p): the box's half width
        assert np.array_equal(T.lut_decode(enc.astype(np.int64) + half - 1, p), m)
        assert np.array_equal(T.lut_decode(enc.astype(np.int64) - half, p), m)
    with pytest.raises(T.TfheAmdError):
        T.lut_encode([4], 4)
    with pytest.raises(T.TfheAmdError):
        T.lut_decode([0], 12)


def test_modswitch_formula_matches_the_oracle():
    import oracle_ctypes as O
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.integers(-2**31, 2**31, 200, dtype=np.int64),
                         [0, -1, 2**31 - 1, -2**31, (1 << 20) - 1, 1 << 20, -(1 << 20), -(1 << 20) - 1]])
    assert [int(v) for v in LO.modswitch_2n(xs)] == [O.modswitch_from(int(x), 2 * N) for x in xs]


def test_composition_reproduces_the_oracle_bootstrap(keyset, okey):
    """tv = (2^29, ..., 2^29): the composition IS orc_bootstrap_woKS, word for word"""
    rng = np.random.default_rng(3)
    x_a, x_b = keyset.encrypt(np.array([0, 1, 1]), rng)
    x_b = x_b.copy()
    x_b[2] = np.int32(-2**31)   # barb = N: the rotation's sign wrap
    u_a, u_b = LO.woks_batch(okey, np.full(N, 1 << 29, np.int32), x_a, x_b)
    w_a, w_b = okey.woks_batch(1 << 29, x_a, x_b, nthreads=LO.THREADS)
    assert np.array_equal(u_a, w_a) and np.array_equal(u_b, w_b)


def test_circuit_lut_host_logic():
    C = T.Circuit()
    rng = np.random.default_rng(9)
    tv0 = rng.integers(-2**31, 2**31, N, dtype=np.int64).astype(np.int32)
    tv1 = T.lut_table(8, T.lut_encode(np.arange(8) % 4, 8))
    a, b, c = C.inputs(3)
    assert C.lut_table(tv0) == 0 and C.lut_table(tv1) == 1
    assert np.array_equal(C.lut_table_get(0), tv0) and np.array_equal(C.lut_table_get(1), tv1)
    g = C.gate("NAND", a, b)
    x = C.lut(1, -5, 1, a, 2, b)                 # level 1, beside the NAND
    y = C.lut(0, 77, 3, x, -1, g, 4, c)          # level 2
    assert (g, x, y) == (3, 4, 5)
    assert C.info() == {"wires": 6, "gates": 3, "bootstraps": 3, "depth": 2}
    assert C.level_sizes() == [0, 2, 1]
    # the node report: gate code -2, the table id in c0's place, coefficients and inputs as a lincomb
    assert C.node(x) == (1, T.LUT_GATE, 1, [1, 2, 0], [a, b, -1])
    assert C.node(y) == (1, T.LUT_GATE, 0, [3, -1, 4], [x, g, c])
    assert C.lut_node(x) == (1, -5) and C.lut_node(y) == (0, 77)
    # the other node kinds report as before
    assert C.node(g) == (1, T.GATES["NAND"], 1 << 29, [-1, -1, 0], [a, b, -1])
    assert C.node(a) == (0, -1, 0, [0, 0, 0], [-1, -1, -1])
    lib = T.lib
    assert lib.tfhe_amd_circuit_lut_node(C.h, g, None, None) == E_ARG
    assert lib.tfhe_amd_circuit_lut_node(C.h, 99, None, None) == E_ARG
    # unknown table ids and wires
    for table in (-1, 2, 1000):
        assert lib.tfhe_amd_circuit_lut(C.h, table, 0, 1, a, 0, -1, 0, -1) == E_ARG, table
    assert lib.tfhe_amd_circuit_lut(C.h, 0, 0, 1, 6, 0, -1, 0, -1) == E_ARG      # wire not yet defined
    assert lib.tfhe_amd_circuit_lut(C.h, 0, 0, 1, -1, 0, -1, 0, -1) == E_ARG     # no first input
    assert lib.tfhe_amd_circuit_lut(C.h, 0, 0, 1, a, 1, 17, 0, -1) == E_ARG
    out = np.zeros(N, np.int32)
    for table in (-1, 2):
        assert lib.tfhe_amd_circuit_lut_table_get(C.h, table, T._p(out)) == E_ARG
    assert lib.tfhe_amd_circuit_lut_table(C.h, None) == E_ARG
    assert C.info()["wires"] == 6                # the refused nodes added nothing
    # a table registered after a compile is usable at once
    assert C.lut_table(tv1) == 2
    z = C.lut(2, 0, 1, y)
    assert C.info()["depth"] == 3 and C.level_sizes() == [0, 2, 1, 1] and C.node(z)[2] == 2
    with pytest.raises(T.TfheAmdError, match="LUT"):
        C.eval_plain({a: [0], b: [1], c: [1]})
    C.close()


@pytest.mark.parametrize("p", [4, 8])
def test_oracle_decodes_every_sample(keyset, okey, p):
    """The condition the GPU decode test rests on: at the encoding (2m + 1) / (4p), fresh inputs at
    the key-switch noise look up a random table exactly (margin 1/(4p) = 0.0625 / 0.031 torus)."""
    msgs, f, tv, x_a, x_b = LO.decode_case(keyset, p)
    r_a, r_b = LO.decode_expected(keyset, okey, p)
    assert np.array_equal(T.lut_decode(keyset.phase(r_a, r_b), p), f[msgs])
