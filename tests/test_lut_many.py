"""Many-LUT bootstrapping, the parts that need no GPU: tfhe_amd_lut_fill_many, the
circuit host logic of many-LUT nodes, and the expected values themselves — the pieces of
tests/many_lut_oracle.py that are numpy (the coarse modulus switch, the extraction at index f) are
pinned to the oracle's own functions, the composition reproduces the single-table one at
theta = 0, and the oracle decodes every sample of the seeded cases the GPU decode tests use."""
import numpy as np
import pytest

import lut_oracle as LO
import many_lut_oracle as MO
import oracle_ctypes as O
import tfhe_amd as T

E_ARG = -1
N = 1024


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def test_fill_many_layout_and_arguments():
    rng = np.random.default_rng(21)
    j = np.arange(N)
    for p, theta, n_fn in ((4, 1, 2), (8, 1, 2), (4, 2, 4), (4, 2, 3), (8, 3, 5), (64, 4, 16), (1, 4, 1), (1024, 0, 1)):
        nu = 1 << theta
        values = _rand32(rng, (n_fn, p))
        tv = T.lut_table_many(p, values, theta)
        assert tv.shape == (N,) and tv.dtype == np.int32
        f = j & (nu - 1)
        want = np.where(f < n_fn, values[np.minimum(f, n_fn - 1), (j * p) // N], 0)
        assert np.array_equal(tv, want), (p, theta, n_fn)
    # theta = 0, one function: tfhe_amd_lut_fill
    for p in (1, 4, 1024):
        values = _rand32(rng, (1, p))
        assert np.array_equal(T.lut_table_many(p, values, 0), T.lut_table(p, values[0])), p
    # every argument error, and a refused call leaves the output untouched
    tv = np.full(N, 7, np.int32)
    values = np.arange(4096, dtype=np.int32)
    fill = T.lib.tfhe_amd_lut_fill_many
    for p, theta, n_fn in ((0, 1, 1), (3, 1, 1), (-4, 1, 1), (2048, 0, 1),      # p
                           (4, -1, 1), (4, 5, 1),                                # log_nu
                           (4, 1, 0), (4, 1, 3), (4, 0, 2), (4, 2, -1),          # n_fn outside [1, nu]
                           (1024, 1, 1), (512, 2, 1), (128, 4, 1)):              # p nu > N
        assert fill(T._p(tv), p, theta, n_fn, T._p(values)) == E_ARG, (p, theta, n_fn)
    assert fill(None, 4, 1, 2, T._p(values)) == E_ARG
    assert fill(T._p(tv), 4, 1, 2, None) == E_ARG
    assert np.all(tv == 7)
    assert fill(T._p(tv), 512, 1, 2, T._p(values)) == 0          # p nu = N is allowed
    with pytest.raises(T.TfheAmdError):
        T.lut_table_many(4, np.zeros(4, np.int32), 1)            # values must be [n_fn][p]
    with pytest.raises(T.TfheAmdError):
        T.lut_table_many(4, np.zeros((3, 4), np.int32), 1)       # n_fn > nu


def test_bar_theta_matches_the_oracle():
    rng = np.random.default_rng(22)
    for theta in range(5):
        nu = 1 << theta
        h = 1 << (20 + theta)
        xs = np.concatenate([rng.integers(0, 2**32, 300, dtype=np.int64),
                             [0, 2**32 - 1, 2**31 - 1, 2**31, h - 1, h, 2**32 - h - 1, 2**32 - h]])
        want = [(nu * O.modswitch_from(int(x), 2 * N // nu)) % (2 * N) for x in xs]
        got = MO.bar(xs, theta)
        assert [int(v) for v in got] == want, theta
        assert np.all(got % nu == 0)
        assert int(MO.bar(2**32 - h, theta)) == 0 and int(MO.bar(2**32 - 1, theta)) == 0   # the wrap
        assert int(MO.bar(2**32 - h - 1, theta)) == 2 * N - nu
        # signed and unsigned views of a word agree
        assert np.array_equal(MO.bar(xs.astype(np.uint32).view(np.int32), theta), got)
    xs = rng.integers(-2**31, 2**31, 300, dtype=np.int64)
    assert np.array_equal(MO.bar(xs, 0), LO.modswitch_2n(xs))


def test_extraction_at_index_f_matches_the_oracle():
    """index-f extraction of acc = index-0 extraction of X^{2N - f} acc (X^{-f} acc has acc[f] at
    coefficient 0), the rotation by the oracle's own orc_mul_by_xai"""
    rng = np.random.default_rng(23)
    acc = _rand32(rng, (2, N))
    for f in (1, 2, 15):
        rot = [O.mul_by_xai(2 * N - f, acc[c]) for c in range(2)]
        w_a, w_b = MO.extract(rot[0], rot[1], 0)
        g_a, g_b = MO.extract(acc[0], acc[1], f)
        assert np.array_equal(g_a, w_a) and g_b == w_b, f
    # index 0 is lut_oracle's extraction
    u_a, u_b = MO.extract(acc[0], acc[1], 0)
    assert u_a[0] == acc[0, 0] and np.array_equal(u_a[1:], LO.wrap(-acc[0, :0:-1].astype(np.int64)))
    assert u_b == acc[1, 0]


def test_composition_at_theta_0_is_the_single_table_one(keyset, okey):
    rng = np.random.default_rng(24)
    tvs = _rand32(rng, (2, N))
    x_a, x_b = _rand32(rng, (3, 500)), _rand32(rng, 3)
    idx = np.array([1, 0, 1])
    u_a, u_b = MO.woks_batch(okey, tvs, x_a, x_b, 0, 1, idx)
    w_a, w_b = LO.woks_batch(okey, tvs, x_a, x_b, idx)
    assert u_a.shape == (1, 3, N) and u_b.shape == (1, 3)
    assert np.array_equal(u_a[0], w_a) and np.array_equal(u_b[0], w_b)


def test_circuit_lut_many_host_logic():
    C = T.Circuit()
    rng = np.random.default_rng(25)
    a, b, c = C.inputs(3)
    t0 = C.lut_table(_rand32(rng, N))
    t1 = C.lut_table(_rand32(rng, N))
    g = C.gate("NAND", a, b)
    x = C.lut(t1, -5, 1, a, 2, b)                            # level 1, beside the NAND
    m = C.lut_many(t0, 2, 3, 77, 3, a, -1, b, 4, c)          # level 1: three wires, one row
    assert (g, x, m) == (3, 4, 5)
    y = C.lut_many(t1, 1, 2, 9, 1, m + 2, 1, g)              # level 2
    z = C.lut_many(t1, 0, 1, 0, 1, y + 1)                    # level 3: theta = 0, one wire
    assert (y, z) == (8, 10)
    # one bootstrap and one gate per many-LUT node, n_out wires; one row per node
    assert C.info() == {"wires": 11, "gates": 5, "bootstraps": 5, "depth": 3}
    assert C.level_sizes() == [0, 3, 1, 1]
    for f in range(3):
        assert C.node(m + f) == (1, T.LUT_MANY_GATE, t0, [3, -1, 4], [a, b, c])
        assert C.lut_many_node(m + f) == (t0, 77, 2, 3, f)
    for f in range(2):
        assert C.node(y + f) == (1, T.LUT_MANY_GATE, t1, [1, 1, 0], [m + 2, g, -1])
        assert C.lut_many_node(y + f) == (t1, 9, 1, 2, f)
    assert C.lut_many_node(z) == (t1, 0, 0, 1, 0)
    assert T.LUT_MANY_GATE == -3
    # the other node kinds report as before
    assert C.node(x) == (1, T.LUT_GATE, t1, [1, 2, 0], [a, b, -1]) and C.lut_node(x) == (t1, -5)
    assert C.node(g) == (1, T.GATES["NAND"], 1 << 29, [-1, -1, 0], [a, b, -1])
    assert C.node(a) == (0, -1, 0, [0, 0, 0], [-1, -1, -1])
    lib = T.lib
    for w in (a, g, x, 99, -1):
        assert lib.tfhe_amd_circuit_lut_many_node(C.h, w, None, None, None, None, None) == E_ARG, w
    assert lib.tfhe_amd_circuit_lut_node(C.h, m, None, None) == E_ARG
    # every refused argument adds nothing
    many = lib.tfhe_amd_circuit_lut_many
    for table in (-1, 2, 1000):
        assert many(C.h, table, 1, 2, 0, 1, a, 0, -1, 0, -1) == E_ARG, table
    for theta, n_out in ((-1, 1), (5, 1), (1, 0), (1, 3), (0, 2), (4, 17), (2, -1)):
        assert many(C.h, t0, theta, n_out, 0, 1, a, 0, -1, 0, -1) == E_ARG, (theta, n_out)
    assert many(C.h, t0, 1, 2, 0, 1, 11, 0, -1, 0, -1) == E_ARG      # wire not yet defined
    assert many(C.h, t0, 1, 2, 0, 1, -1, 0, -1, 0, -1) == E_ARG      # no first input
    assert many(C.h, t0, 1, 2, 0, 1, a, 1, 17, 0, -1) == E_ARG
    assert many(None, t0, 1, 2, 0, 1, a, 0, -1, 0, -1) == E_ARG
    assert C.info()["wires"] == 11 and C.level_sizes() == [0, 3, 1, 1]
    # the widest node
    w16 = C.lut_many(t0, 4, 16, 0, 1, a)
    assert w16 == 11 and C.info()["wires"] == 27 and C.level_sizes() == [0, 4, 1, 1]
    assert C.lut_many_node(w16 + 15) == (t0, 0, 4, 16, 15)
    C.close()
    # eval_plain refuses such nodes the way it refuses LUT nodes
    D = T.Circuit()
    a, = D.inputs(1)
    D.lut_many(D.lut_table(_rand32(rng, N)), 1, 2, 0, 1, a)
    with pytest.raises(T.TfheAmdError, match="many-LUT"):
        D.eval_plain({a: [0]})
    D.close()


@pytest.mark.parametrize("p,theta,n_out", MO.DECODE_CASES)
def test_oracle_decodes_every_sample(keyset, okey, p, theta, n_out):
    """The condition the GPU decode tests rest on: fresh inputs at the key-switch
    noise, switched to a multiple of 2^theta, stay inside their box of half width 1/(4p), and every
    one of the n_out functions is looked up exactly.  Prints the largest deviation from the box
    centre the blind rotation sees (recorded in DESIGN.md)."""
    msgs, f, tv, x_a, x_b = MO.decode_case(keyset, p, theta, n_out)
    dev = np.abs(MO.switched_phase(keyset, x_a, x_b, theta) - (2 * msgs + 1) / (4.0 * p))
    print(f"many-LUT decode case p={p} theta={theta} n_out={n_out}: largest deviation {dev.max():.4f}, "
          f"std {np.sqrt(np.mean(dev**2)):.4f}, margin {1 / (4.0 * p):.4f}")
    assert dev.max() < 1 / (4.0 * p)
    r_a, r_b = MO.decode_expected(keyset, okey, p, theta, n_out)
    assert r_a.shape == (n_out, 48, 500)
    for r in range(n_out):
        assert np.array_equal(T.lut_decode(keyset.phase(r_a[r], r_b[r]), p), f[r][msgs]), r


def test_oracle_decodes_the_many_lut_adder(keyset, okey):
    """the radix-4 adder with one many-LUT row per digit (p = 8, theta = 1; the second digit adds one
    bootstrapped term, the carry): the oracle's node-by-node evaluation adds correctly"""
    B = 5
    case = MO.adder_case(keyset, okey, B)
    C, ins, outs, digits, bits, enc, W = case
    assert C.level_sizes() == [0, 4, 1]      # one row per digit where test_lut_gpu.py's adder has two
    assert C.info() == {"wires": 15, "gates": 5, "bootstraps": 5, "depth": 2}
    # the phase the second digit's rotation sees, against its box centre
    s0, c0, nand, s1, c1 = outs
    x = LO.lin(-2 * MO.Q27, [(1, W[ins[1]]), (1, W[ins[3]]), (1, W[c0])], B)
    total = digits[1] + digits[3] + ((digits[0] + digits[2]) >> 2)
    dev = np.abs(MO.switched_phase(keyset, x[0], x[1], 1) - (2 * total + 1) / 32.0)
    print(f"many-LUT adder, digit 1 (one bootstrapped term), B={B}: largest deviation {dev.max():.4f}, margin 0.0312")
    assert dev.max() < 1 / 32.0
    got = MO.adder_decoded(keyset, case, W)
    for g, w in zip(got, MO.adder_truth(case)):
        assert np.array_equal(g, w)
