"""Leveled automata, the parts that need no GPU: the host-only builders against
brute force, the live sets against a plain Python reachability, the argument checks that return
before a device is touched, and the oracle composition of tests/dfa_oracle.py on the library's own
encryptions: every output decodes, the error before the key switch is printed and bounded."""
import ctypes
import itertools

import numpy as np
import pytest

import dfa_oracle as DO
import tfhe_amd as T
import tgsw_oracle as TO

N, n_lwe = 1024, 500
E_ARG = -1
E8 = 1 << 29


def _seed(*values):
    s = (ctypes.c_uint32 * len(values))(*values)
    T.lib.tfhe_random_generator_setSeed(s, len(values))


def _words(n):
    return itertools.product((0, 1), repeat=n)


# ---- builders against brute force

def test_compare_every_pair_of_5_bit_integers():
    nxt, start, cls = T.dfa_compare()
    assert nxt.shape == (5, 2) and cls.shape == (5,) and cls[start] == T.DFA_EQ
    for x in range(32):
        for y in range(32):
            word = [((v >> k) & 1) for k in range(4, -1, -1) for v in (x, y)]
            want = T.DFA_LT if x < y else T.DFA_GT if x > y else T.DFA_EQ
            assert cls[T.dfa_simulate(nxt, start, word)] == want, (x, y)
            assert cls[T.dfa_simulate(nxt, start, word[:-1])] in (T.DFA_MID, T.DFA_LT, T.DFA_GT)
    # between the bits of a pair the undecided word is in a mid-pair state
    assert cls[T.dfa_simulate(nxt, start, [1, 1, 0])] == T.DFA_MID


def test_contains_every_pattern_up_to_4_bits_over_every_word_up_to_10_bits():
    for m in range(1, 5):
        for pat in _words(m):
            nxt, start = T.dfa_contains(pat)
            assert nxt.shape == (m + 1, 2) and start == 0
            assert tuple(nxt[m]) == (m, m)
            p = "".join(map(str, pat))
            for n in range(0, 11):
                for word in _words(n):
                    got = DO.simulate(nxt, start, word) == m
                    assert got == (p in "".join(map(str, word))), (pat, word)
    # the library's own simulation agrees with the Python one
    nxt, start = T.dfa_contains([1, 0, 1, 1])
    for word in _words(9):
        assert T.dfa_simulate(nxt, start, word) == DO.simulate(nxt, start, word)


def test_at_least_t_up_to_4_over_every_word_up_to_8_bits():
    for t in range(1, 5):
        nxt, start = T.dfa_at_least(t)
        assert nxt.shape == (t + 1, 2) and start == 0
        for n in range(0, 9):
            for word in _words(n):
                assert T.dfa_simulate(nxt, start, word) == min(sum(word), t), (t, word)


def test_builders_at_their_limits_and_beyond():
    nxt, _ = T.dfa_contains([1] * 63)
    assert nxt.shape == (64, 2) and T.dfa_simulate(nxt, 0, [0] + [1] * 63) == 63
    nxt, _ = T.dfa_at_least(63)
    assert T.dfa_simulate(nxt, 0, [1] * 70) == 63 and T.dfa_simulate(nxt, 0, [1] * 62) == 62
    for bad in ([1] * 64, [], [0, 2]):
        with pytest.raises(T.TfheAmdError):
            T.dfa_contains(bad)
    for bad in (0, 64, -1):
        with pytest.raises(T.TfheAmdError):
            T.dfa_at_least(bad)
    L = T.lib
    start = ctypes.c_int()
    buf = np.zeros(200, np.int32)
    assert L.tfhe_amd_dfa_build_compare(None, ctypes.byref(start), None) == E_ARG
    assert L.tfhe_amd_dfa_build_compare(T._p(buf), None, None) == E_ARG
    assert L.tfhe_amd_dfa_build_compare(T._p(buf), ctypes.byref(start), None) == 5
    assert L.tfhe_amd_dfa_build_contains(2, None, T._p(buf), ctypes.byref(start)) == E_ARG
    assert L.tfhe_amd_dfa_build_at_least(2, None, ctypes.byref(start)) == E_ARG


def test_fin_fill_places_the_outputs_at_the_first_coefficients():
    vals = np.arange(1, 16, dtype=np.int32).reshape(5, 3)
    fin = T.dfa_fin(vals)
    assert fin.shape == (1, 5, 1, N) and np.array_equal(fin[0, :, 0, :3], vals) and not fin[0, :, 0, 3:].any()
    assert T.dfa_fin(np.array([7, -7], np.int32)).shape == (1, 2, 1, N)
    out = np.ones((2, N), np.int32)
    v = np.zeros((2, 17), np.int32)
    assert T.lib.tfhe_amd_dfa_fin_fill(2, 17, T._p(v), T._p(out)) == E_ARG
    assert T.lib.tfhe_amd_dfa_fin_fill(2, 0, T._p(v), T._p(out)) == E_ARG
    assert T.lib.tfhe_amd_dfa_fin_fill(65, 1, T._p(v), T._p(out)) == E_ARG
    assert T.lib.tfhe_amd_dfa_fin_fill(2, 1, None, T._p(out)) == E_ARG
    assert out.all()                                 # refused before anything is written


def test_simulate_refuses_bad_words_and_tables():
    nxt, start, _ = T.dfa_compare()
    L = T.lib
    assert T.dfa_simulate(nxt, start, []) == start
    assert T.dfa_simulate(nxt, 3, [1]) == 1
    bits = np.array([0, 2], np.int32)
    assert L.tfhe_amd_dfa_simulate(5, 0, T._p(nxt), 2, T._p(bits)) == E_ARG
    assert L.tfhe_amd_dfa_simulate(5, 5, T._p(nxt), 0, None) == E_ARG
    assert L.tfhe_amd_dfa_simulate(5, 0, T._p(nxt), 1, None) == E_ARG
    assert L.tfhe_amd_dfa_simulate(4, 0, T._p(nxt), 0, None) == E_ARG      # a transition to state 4 of 4
    assert L.tfhe_amd_dfa_simulate(5, 0, None, 0, None) == E_ARG


# ---- live sets

def _random_automaton(rng, Q):
    nxt = rng.integers(0, Q, (Q, 2)).astype(np.int32)
    return nxt, int(rng.integers(0, Q))


def test_live_sets_against_the_python_reachability():
    rng = np.random.default_rng(31)
    cases = [T.dfa_compare()[:2], T.dfa_contains([1, 1, 0, 1]), T.dfa_at_least(5)]
    cases += [_random_automaton(rng, Q) for Q in (1, 2, 5, 17, 64, 64)]
    ring = np.array([[(s + 1) % 64, (s + 1) % 64] for s in range(64)], np.int32)   # one state live per step
    cases.append((ring, 63))
    for nxt, start in cases:
        max_len = 70
        dfa = T.Dfa.host(nxt, start, max_len)
        try:
            assert (dfa.n_states, dfa.start, dfa.max_len, dfa.device) == (nxt.shape[0], start, max_len, -1)
            want = DO.reach(nxt, start, max_len)
            for i in range(max_len + 1):
                assert dfa.live(i).tolist() == want[i], i
            assert T.lib.tfhe_amd_dfa_live(dfa.h, 0, None) == 1        # the count alone
            for bad in (-1, max_len + 1):
                with pytest.raises(T.TfheAmdError):
                    dfa.live(bad)
        finally:
            dfa.close()
    # the comparison: one or two products per step (the decided states copy)
    nxt, start, _ = T.dfa_compare()
    live = DO.reach(nxt, start, 8)
    assert [sum(nxt[s][0] != nxt[s][1] for s in r) for r in live[:8]] == [1, 2] * 4


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = T.lib
    nxt, start, _ = T.dfa_compare()
    h = ctypes.c_void_p(1234)

    def create(n, st, table, max_len, out=h):
        return L.tfhe_amd_dfa_create(None, n, st, table, max_len, None if out is None else ctypes.byref(out))

    assert create(5, 0, T._p(nxt), 8, None) == E_ARG
    for args in ((0, 0, T._p(nxt), 8), (65, 0, T._p(nxt), 8), (5, -1, T._p(nxt), 8), (5, 5, T._p(nxt), 8),
                 (5, 0, None, 8), (5, 0, T._p(nxt), 0), (5, 0, T._p(nxt), 1025), (4, 0, T._p(nxt), 8)):
        h.value = 1234
        assert create(*args) == E_ARG and h.value is None, args[:2] + args[3:]
    bad = nxt.copy()
    bad[2, 1] = -1
    assert create(5, 0, T._p(bad), 8) == E_ARG
    assert create(5, 0, T._p(nxt), 1024) == 0 and h.value
    dfa = T.Dfa(h.value)
    assert L.tfhe_amd_dfa_info(None, None, None, None, None) == E_ARG
    assert L.tfhe_amd_dfa_info(dfa.h, None, None, None, None) == 0
    assert L.tfhe_amd_dfa_live(None, 0, None) == E_ARG
    assert L.tfhe_amd_dfa_destroy(None) == 0
    # the runs: a null context, set or automaton is refused before anything is read
    buf = np.zeros(5 * N, np.int32)
    p = buf.ctypes.data
    for f in ("tfhe_amd_dfa_run_woks_dev", "tfhe_amd_dfa_run_dev"):
        assert getattr(L, f)(None, None, None, 1, 1, p, 1, 1, p, None, 1, p, p, None) == E_ARG
        assert getattr(L, f)(None, None, dfa.h, 1, 1, p, 1, 1, p, None, 1, p, p, None) == E_ARG
    for f in ("tfhe_amd_dfa_run_woks_host", "tfhe_amd_dfa_run_host"):
        q = T._p(buf)
        assert getattr(L, f)(None, None, None, 1, 1, q, 1, 1, q, None, 1, q, q) == E_ARG
        assert getattr(L, f)(None, None, dfa.h, 1, 1, q, 1, 1, q, None, 1, q, q) == E_ARG
    dfa.close()


# ---- real encryptions through the oracle composition

def _pool(keyset, seed, count=24):
    """a pool of `count` TGSW samples on random bits (both values present), shared by the queries"""
    _seed(seed)
    bits = np.random.default_rng(seed).integers(0, 2, count).astype(np.int32)
    bits[:2] = (0, 1)
    return bits, keyset.tgsw_encrypt(bits)


def _compare_case():
    """the comparison automaton with the outputs (x < y, x = y, x > y) as +-1/8"""
    nxt, start, cls = T.dfa_compare()
    vals = np.array([[E8 if c == k else -E8 for k in (T.DFA_LT, T.DFA_EQ, T.DFA_GT)] for c in cls], np.int32)
    return nxt, start, vals, T.dfa_fin(vals)


def _compare_words(rng, length):
    """three words of length / 2 pairs: all-equal, differing in the last pair only, random"""
    d = length // 2
    x = rng.integers(0, 2, (3, d))
    y = x.copy()
    y[1, -1] ^= 1
    y[2] = rng.integers(0, 2, d)
    return np.stack([x, y], axis=2).reshape(3, length)


def _errors(keyset, u, want):
    """phase error of the extracted samples [n_out][B] against the expected torus values, in torus units"""
    ph = keyset.phase_extracted(u[0].reshape(-1, N), u[1].reshape(-1)).astype(np.int64)
    return TO.wrap(ph - np.asarray(want, dtype=np.int64).reshape(-1)).astype(np.float64) / 2.0**32


def test_zero_difference_has_an_exactly_zero_product(keyset):
    """what lets a state with next0 == next1 copy its operand: the digits of 0 + 2^11 are all zero"""
    _, g = _pool(keyset, 5)
    ok = TO.key(g, keyset.ksk)
    for i in (0, 1, 7):
        assert not ok.external_product(np.full((2, N), DO.ROUND, np.int32), i).any()
        assert not ok.external_product(np.zeros((2, N), np.int32), i).any()
    d = np.random.default_rng(5).integers(-2**31, 2**31, (2, N), dtype=np.int64).astype(np.int32)
    assert np.array_equal(DO.step(ok, 3, d, d), d)


@pytest.mark.parametrize("length", [64, 256])
def test_comparison_every_output_decodes(keyset, capsys, length):
    """the 32-bit and the 128-bit comparison on real encryptions: three words (all-equal, last pair
    differs, random), n_out = 3: all 9 outputs decode after the key switch, and the error before it
    stays below 1/32, half of the 1/16 a gate input may carry.
    Measured (this seed): len 64: largest 0.00144, r.m.s. 0.00064; len 256: largest 0.00359, r.m.s. 0.00164."""
    rng = np.random.default_rng(length)
    bits, g = _pool(keyset, length)
    ok = TO.key(g, keyset.ksk)
    nxt, start, vals, fin = _compare_case()
    words = _compare_words(rng, length)
    sel = TO.pick(rng, bits, words)
    states = [DO.simulate(nxt, start, w) for w in words]
    assert states[0] == start and states[1] != start
    want = np.stack([vals[s] for s in states], axis=1)            # [n_out][B]
    u = DO.run_woks(ok, nxt, start, sel, fin, None, 3)
    assert u[0].shape == (3, 3, N)
    err = _errors(keyset, u, want)
    with capsys.disabled():
        print(f"dfa compare len={length} (before the key switch): {err.size} samples, largest error "
              f"{np.abs(err).max():.5f}, r.m.s. {np.sqrt(np.mean(err**2)):.5f}")
    assert np.abs(err).max() < 1.0 / 32
    r_a, r_b = TO.MO.keyswitch(ok, u)
    assert r_a.shape == (3, 3, n_lwe)
    assert np.array_equal(keyset.decrypt(r_a.reshape(-1, n_lwe), r_b.reshape(-1)), (want.reshape(-1) > 0).astype(np.int32))


def test_truncating_composition_is_biased(keyset, capsys):
    """the diagnostic behind the 2^11: on the all-equal word at len = 128 the truncating composition's
    largest error is at least twice the rounding one's (its mean adds up along the chain).
    Measured (this seed): truncating 0.01630, rounding 0.00201."""
    rng = np.random.default_rng(128)
    bits, g = _pool(keyset, 128)
    ok = TO.key(g, keyset.ksk)
    nxt, start, vals, fin = _compare_case()
    x = rng.integers(0, 2, 64)
    word = np.stack([x, x], axis=1).reshape(1, 128)
    sel = TO.pick(rng, bits, word)
    want = vals[start][:, None]
    worst = {}
    for rounding in (True, False):
        u = DO.run_woks(ok, nxt, start, sel, fin, None, 3, rounding=rounding)
        worst[rounding] = np.abs(_errors(keyset, u, want)).max()
    with capsys.disabled():
        print(f"dfa compare len=128 all-equal: largest error truncating {worst[False]:.5f}, rounding {worst[True]:.5f}")
    assert worst[False] >= 2 * worst[True]
