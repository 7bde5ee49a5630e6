"""The construction behind the partly flagged guard batches (tests/guard_cases.py), checked on the
CPU: the inverse-prologue builders give gate inputs whose prologue combination is the wanted x word
for word — through the oracle's own gate code, for NAND, XOR, both MUX halves and circuit rows — and
with the head-250 key the fp64 CPU port (no guard) keeps every clean sample below 1/8 and right,
drives every dirty sample to 1/8 or more and gets at least half of them wrong.  The GPU tests in
tests/test_guard_partial_gpu.py place such samples in every launch form."""
import numpy as np
import pytest

import circuit_oracle
import guard_cases as G
import oracle_ctypes as O
import tfhe_amd as T


@pytest.fixture(scope="module")
def xs():
    """three samples x with few non-zero words at random places (every bootstrap of the real-key
    oracle below costs only those steps), even like the dirty samples"""
    rng = np.random.default_rng(61)
    a, b = G.dirty(rng, 3)
    keep = np.zeros(G.n_lwe, bool)
    keep[rng.choice(G.n_lwe, 12, replace=False)] = True
    a[:, ~keep] = 0
    return a, b


def _boot(okey, x_a, x_b):
    return okey.keyswitch_batch(*okey.woks_batch(G.MU, x_a, x_b))


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("gate", ["NAND", "OR", "ANDNY", "XOR"])
def test_inverse_prologue_binary_gates(okey, xs, gate):
    """the oracle's gate on the built inputs = its bootstrap of x itself"""
    ins = G.gate_inputs(gate, *xs)
    assert _same(okey.gate_batch(gate, *ins), _boot(okey, *xs))
    c, sa, sb = O.GATE_SPEC[gate]
    assert np.array_equal(G.wrap(np.int64(sa) * ins[0] + np.int64(sb) * ins[2]), xs[0])
    assert np.array_equal(G.wrap(c + np.int64(sa) * ins[1] + np.int64(sb) * ins[3]), xs[1])


def test_inverse_prologue_refuses_odd_words(xs):
    with pytest.raises(ValueError):
        G.gate_inputs("XOR", xs[0] | 1, xs[1])


def test_inverse_prologue_mux_halves(okey, xs):
    """half 0 is x0 and half 1 is x1, independently: MUX = KS(u(x0) + u(x1) + (0, mu))"""
    x0 = xs
    x1 = (xs[0][::-1].copy(), G.wrap(xs[1][::-1].astype(np.int64) + 12345678))
    ins = G.mux_inputs(*x0, *x1)
    u0, u1 = okey.woks_batch(G.MU, *x0), okey.woks_batch(G.MU, *x1)
    want = okey.keyswitch_batch(G.wrap(u0[0].astype(np.int64) + u1[0]), G.wrap(u0[1].astype(np.int64) + u1[1] + G.MU))
    assert _same(okey.gate_batch("MUX", *ins), want)


def test_inverse_prologue_circuit_rows(okey, xs):
    """three gate rows of one level, each on its own input wires: every row's output wire is the
    bootstrap of its own x (node by node through circuit_oracle)"""
    gates = G.placements(256)["circuit"]["gates"]
    C = T.Circuit()
    B = xs[1].shape[0]
    inputs, outs = {}, []
    for r, gate in enumerate(gates):
        wa, wb = C.inputs(2)
        x = (np.roll(xs[0], r, axis=0), np.roll(xs[1], r))
        ins = G.gate_inputs(gate, *x)
        inputs[wa], inputs[wb] = ins[:2], ins[2:]
        outs.append((C.gate(gate, wa, wb), x))
    W = circuit_oracle.eval_circuit(C, okey, inputs, B)
    for w, x in outs:
        assert _same(W[w], _boot(okey, *x)), w
    C.close()


def test_batch_places_the_samples():
    rng = np.random.default_rng(3)
    pool = G.dirty(rng, 4)
    a, b = G.batch(rng, 9, [2, 7], [0, 8], pool)
    nz = (a != 0).any(axis=1)
    assert list(np.flatnonzero(nz)) == [0, 2, 7, 8]
    assert np.array_equal(a[2], pool[0][0]) and np.array_equal(a[7], pool[0][1]) and b[7] == pool[1][1]
    assert not a[0, :G.HEAD].any() and a[0, G.HEAD:].any() and a[2, :G.HEAD].any()
    (a0, b0), (a1, b1) = G.mux_batch(rng, 5, [(1, 0), (3, 1)], [(0, 0), (4, 1)], pool)
    assert list(np.flatnonzero((a0 != 0).any(axis=1))) == [0, 1] and list(np.flatnonzero((a1 != 0).any(axis=1))) == [3, 4]
    assert np.array_equal(a1[3], pool[0][1])


@pytest.mark.parametrize("cus", [256, 304])
def test_placements_reach_their_forms(cus):
    """the shapes, against the launchers' thresholds (blind_rotate_v6.hip: paired for CUs < n <= 2 CUs,
    reg-rotation above 2 CUs, launches of 4 CUs; host_batch.cpp: slices of 1 024)"""
    P = G.placements(cus)
    paired = lambda n: cus < n <= 2 * cus
    assert P["lds"]["B"] <= cus and 2 * P["mux_small"]["B"] <= cus
    assert paired(P["paired"]["B"]) and P["paired"]["B"] % 2 == 1 and paired(P["paired_even"]["B"])
    assert 2 * cus < P["reg"]["B"] <= 4 * cus
    c = P["chunked"]
    assert c["base"] == 4 * cus and paired(c["B"] - c["base"]) and (c["B"] - c["base"]) % 2 == 1
    m = P["mux_seam_a"]
    assert paired(2 * m["B"]) and m["B"] % 2 == 1 and P["mux_seam_b"]["B"] == m["B"]
    m = P["mux_chunked"]
    assert 2 * m["B"] > 4 * cus and 2 * m["B"] - m["base"] <= cus and [k for k, h in m["dirty"]] == \
        [m["base"] - m["B"] - 1, m["base"] - m["B"]]
    for name, p in P.items():
        assert len(p["real"]) >= 2 and len(p["dirty"]) <= 12, name


def test_cpu_port_proxy_of_the_construction(keyset):
    """The unguarded fp64 CPU port under the head-250 key, a pool of 16 dirty and 8 clean samples:
    every clean sample stays below 1/8 and is right on every word, every dirty sample reaches 1/8
    (the port reports the largest distance a key has seen, so each dirty sample runs on a fresh
    handle) and at least half of the dirty samples come out wrong."""
    bk = G.head_key(keyset.bk)
    okey = O.OracleKey(bk, keyset.ksk, use_ntt=True)
    rng = np.random.default_rng(7)
    d_a, d_b = G.dirty(rng, 16)
    c_a, c_b = G.clean(rng, 8)
    f = O.CpuFftKey(bk, keyset.ksk)
    got = f.woks_batch(G.MU, c_a, c_b, nthreads=8)
    want = okey.woks_batch(G.MU, c_a, c_b, nthreads=8)
    assert 0.0 < f.max_round_error() < 0.125, f.max_round_error()
    assert _same(got, want)
    want = okey.woks_batch(G.MU, d_a, d_b, nthreads=8)
    wrong, dist = 0, []
    for k in range(d_b.shape[0]):
        f = O.CpuFftKey(bk, keyset.ksk)
        got = f.woks_batch(G.MU, d_a[k:k + 1], d_b[k:k + 1], nthreads=1)
        dist.append(f.max_round_error())
        wrong += int(np.any(got[0][0] != want[0][k]) or got[1][0] != want[1][k])
    print(f"dirty: {wrong} of {len(dist)} wrong, distances {min(dist):.3f} .. {max(dist):.3f}")
    assert min(dist) >= 0.125, dist
    assert 2 * wrong >= len(dist), (wrong, len(dist))
