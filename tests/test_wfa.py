"""Weighted leveled automata, the parts that need no GPU: the host-only builders
against brute force through tfhe_amd_wfa_simulate, the argument checks that return before a device
is touched, and the oracle composition of tests/wfa_oracle.py on the library's own encryptions:
every output decodes to the plain result, the error before the key switch is printed and bounded,
and with all-zero weights the composition is tests/dfa_oracle.py's word for word."""
import ctypes
import itertools

import numpy as np
import pytest

import dfa_oracle as DO
import tfhe_amd as T
import tgsw_oracle as TO
import wfa_oracle as WO

N, n_lwe = 1024, 500
E_ARG = -1
E8 = 1 << 29
ONE = 1 << 30


def _seed(*values):
    s = (ctypes.c_uint32 * len(values))(*values)
    T.lib.tfhe_random_generator_setSeed(s, len(values))


def _words(n):
    return itertools.product((0, 1), repeat=n)


def _bits(v, n):
    return [(v >> f) & 1 for f in range(n)]


# ---- builders against brute force

@pytest.mark.parametrize("want_max", [True, False])
def test_max_and_min_of_every_pair_of_3_bit_integers(want_max):
    d = 3
    nxt, start, (w_val, w_pos), fin = T.wfa_max(d, want_max)
    assert nxt.shape == (7, 2) and w_val.shape == (7, 2) and start == 0
    assert w_pos.tolist() == [2, 2, 1, 1, 0, 0]
    assert fin.shape == (1, 7, 1, N) and (fin[0, :, 0, :d] == -E8).all() and not fin[0, :, 0, d:].any()
    assert set(np.unique(w_val).tolist()) == {0, ONE}
    for x in range(8):
        for y in range(8):
            word = WO.max_word(x, y, d)
            s, poly = T.wfa_simulate(nxt, start, (w_val, w_pos), word)
            want = max(x, y) if want_max else min(x, y)
            assert poly[:d].tolist() == [ONE * b for b in _bits(want, d)], (x, y)
            assert not poly[d:].any()
            # output f = fin + the path's weights at coefficient f: the gate encoding of bit f
            assert (fin[0, s, 0, :d] + poly[:d]).tolist() == [E8 if b else -E8 for b in _bits(want, d)]
            # the final state is the comparison's, and the Python simulation agrees
            assert (s == 0) == (x == y) and (s == 3) == (x < y) and (s == 5) == (x > y)
            s2, poly2 = WO.simulate(nxt, start, w_val, w_pos, word)
            assert s2 == s and np.array_equal(poly2, poly)
    # at most 5 products per pair: 2 on the x bit, 3 on the y bit
    live = DO.reach(nxt, start, 2 * d)
    prod = [sum(nxt[s][0] != nxt[s][1] or w_val[s][0] != w_val[s][1] for s in r) for r in live[:2 * d]]
    assert all(a + b <= 5 for a, b in zip(prod[0::2], prod[1::2])) and prod[2:4] == [2, 3]


def test_popcount_modulo_8_over_every_word_up_to_7_bits():
    p = 8
    for length in range(1, p):
        nxt, start, (w_val, w_pos), fin = T.wfa_popcount(length, p)
        assert nxt.tolist() == [[0, 0]] and start == 0 and w_val.tolist() == [[0, 2**32 // (2 * p)]]
        assert w_pos.tolist() == [0] * length and fin[0, 0, 0, 0] == 2**32 // (4 * p) and not fin[0, 0, 0, 1:].any()
        for word in _words(length):
            s, poly = T.wfa_simulate(nxt, start, (w_val, w_pos), word)
            c = sum(word)
            assert s == 0 and not poly[1:].any()
            # the LUT digit (2 c + 1) / (4 p) of DESIGN.md §3.2
            assert (int(fin[0, 0, 0, 0]) + int(poly[0])) % 2**32 == (2 * c + 1) * 2**32 // (4 * p), word


def test_first_one_over_every_5_bit_word():
    length = 5
    nxt, start, (w_val, w_pos), fin = T.wfa_first_one(length)
    assert nxt.tolist() == [[0, 1], [1, 1]] and start == 0 and w_val.tolist() == [[0, ONE], [0, 0]]
    assert w_pos.tolist() == list(range(length))
    for word in _words(length):
        s, poly = T.wfa_simulate(nxt, start, (w_val, w_pos), word)
        first = word.index(1) if 1 in word else -1
        assert s == (first >= 0)
        assert (fin[0, s, 0, :length] + poly[:length]).tolist() == [E8 if f == first else -E8 for f in range(length)]
        assert not poly[length:].any()


def test_builders_at_their_limits_and_beyond():
    nxt, start, (w_val, w_pos), fin = T.wfa_max(64)
    assert w_pos.shape == (128,) and w_pos[0] == 63 and w_pos[-1] == 0 and (fin[0, :, 0, :64] == -E8).all()
    x, y = 0xF00DFACE12345678, 0xF00DFACE12345679
    s, poly = T.wfa_simulate(nxt, start, (w_val, w_pos), WO.max_word(x, y, 64))
    assert poly[:64].tolist() == [ONE * b for b in _bits(y, 64)] and s == 3
    assert T.wfa_first_one(64)[2][1].tolist() == list(range(64))
    assert T.wfa_popcount(15, 16)[2][0].tolist() == [[0, 2**27]]
    assert T.wfa_popcount(1, 2)[2][0].tolist() == [[0, ONE]]
    for bad in (0, 65, -1):
        with pytest.raises(T.TfheAmdError):
            T.wfa_max(bad)
        with pytest.raises(T.TfheAmdError):
            T.wfa_first_one(bad)
    for length, p in ((0, 8), (8, 8), (1, 3), (1, 32), (1, 1), (2, 2)):
        with pytest.raises(T.TfheAmdError):
            T.wfa_popcount(length, p)
    L = T.lib
    st = ctypes.c_int()
    a, b, c = (np.full(200, 7, np.int32) for _ in range(3))
    pa, pb, pc, ps = T._p(a), T._p(b), T._p(c), ctypes.byref(st)
    assert L.tfhe_amd_wfa_build_max(3, 1, None, ps, pb, pc) == E_ARG
    assert L.tfhe_amd_wfa_build_max(3, 1, pa, None, pb, pc) == E_ARG
    assert L.tfhe_amd_wfa_build_max(3, 1, pa, ps, None, pc) == E_ARG
    assert L.tfhe_amd_wfa_build_max(3, 1, pa, ps, pb, None) == E_ARG
    assert L.tfhe_amd_wfa_build_popcount(3, 8, pa, ps, None, pc) == E_ARG
    assert L.tfhe_amd_wfa_build_first_one(3, pa, ps, pb, None) == E_ARG
    assert L.tfhe_amd_wfa_build_max(65, 1, pa, ps, pb, pc) == E_ARG
    assert (a == 7).all() and (b == 7).all() and (c == 7).all()          # refused before anything is written
    assert L.tfhe_amd_wfa_build_max(3, 0, pa, ps, pb, pc) == 7 and (a[14:] == 7).all() and (c[6:] == 7).all()
    fin = np.ones((2, N), np.int32)
    assert L.tfhe_amd_wfa_fin_fill(2, 65, 5, T._p(fin)) == E_ARG and L.tfhe_amd_wfa_fin_fill(2, 0, 5, T._p(fin)) == E_ARG
    assert L.tfhe_amd_wfa_fin_fill(65, 1, 5, T._p(fin)) == E_ARG and L.tfhe_amd_wfa_fin_fill(2, 1, 5, None) == E_ARG
    assert fin.all()
    assert L.tfhe_amd_wfa_fin_fill(2, 64, 5, T._p(fin)) == 0 and (fin[:, :64] == 5).all() and not fin[:, 64:].any()


def test_simulate_refuses_bad_words_weights_and_tables():
    nxt, start, (w_val, w_pos), _ = T.wfa_max(2)
    L = T.lib
    poly = np.full(N, 9, np.int32)
    p = T._p

    def sim(n=7, st=0, table=nxt, wv=w_val, wp=w_pos, length=4, bits=np.array([0, 1, 1, 0], np.int32), out=poly):
        return L.tfhe_amd_wfa_simulate(n, st, p(table), p(wv), p(wp), length, p(bits), p(out))

    assert sim(bits=np.array([0, 2, 0, 0], np.int32)) == E_ARG
    assert sim(wp=np.array([0, 0, 1024, 0], np.int32)) == E_ARG and sim(wp=np.array([0, -1, 0, 0], np.int32)) == E_ARG
    assert sim(st=7) == E_ARG and sim(n=6) == E_ARG and sim(table=None) == E_ARG and sim(wv=None) == E_ARG
    assert sim(bits=None) == E_ARG and sim(wp=None) == E_ARG and sim(out=None) == E_ARG and sim(length=-1) == E_ARG
    assert (poly == 9).all()                                          # refused before anything is written
    assert sim(length=0, bits=None, wp=None) == 0 and not poly.any()  # the empty word: no weight
    assert sim() == 3 and poly[:2].tolist() == [0, ONE]               # x = 01, y = 10: x < y, the maximum is y
    # the weights wrap modulo 2^32
    s, q = T.wfa_simulate([[0, 0]], 0, ([[0, -2**31]], [5, 5, 5]), [1, 1, 1])
    assert s == 0 and q[5] == -2**31 and not np.delete(q, 5).any()


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = T.lib
    nxt, start, (w_val, w_pos), _ = T.wfa_max(2)
    dfa = T.Dfa.host(nxt, start, 4)
    buf = np.zeros(7 * N, np.int32)
    p = buf.ctypes.data
    for f in ("tfhe_amd_wfa_run_woks_dev", "tfhe_amd_wfa_run_dev"):
        assert getattr(L, f)(None, None, None, 1, 1, p, p, p, 1, 1, p, None, 1, p, p, None) == E_ARG
        assert getattr(L, f)(None, None, dfa.h, 1, 1, p, p, p, 1, 1, p, None, 1, p, p, None) == E_ARG
    q = T._p(buf)
    for f in ("tfhe_amd_wfa_run_woks_host", "tfhe_amd_wfa_run_host"):
        assert getattr(L, f)(None, None, None, 1, 1, q, q, q, 1, 1, q, None, 1, q, q) == E_ARG
        assert getattr(L, f)(None, None, dfa.h, 1, 1, q, q, q, 1, 1, q, None, 1, q, q) == E_ARG
    dfa.close()


# ---- real encryptions through the oracle composition

def _pool(keyset, seed, count=24):
    """a pool of `count` TGSW samples on random bits (both values present), shared by the queries"""
    _seed(seed)
    bits = np.random.default_rng(seed).integers(0, 2, count).astype(np.int32)
    bits[:2] = (0, 1)
    return bits, keyset.tgsw_encrypt(bits)


def _errors(keyset, u, want):
    """phase error of the extracted samples [n_out][B] against the expected torus values, in torus units"""
    ph = keyset.phase_extracted(u[0].reshape(-1, N), u[1].reshape(-1)).astype(np.int64)
    return TO.wrap(ph - np.asarray(want, dtype=np.int64).reshape(-1)).astype(np.float64) / 2.0**32


def _check_real(keyset, capsys, what, nxt, start, weights, fin, words, n_out, decode):
    """run the oracle composition on real encryptions of `words`: the phase of every output before the
    key switch is the plain value fin + the path's weights within 1/32 (test_dfa.py's bound, half of
    the 1/16 a gate input may carry), and decode(r_a, r_b) of the key-switched outputs is checked by
    the caller"""
    w_val, w_pos = weights
    rng = np.random.default_rng(len(words) * 1000 + n_out)
    bits, g = _pool(keyset, 100 + n_out)
    ok = TO.key(g, keyset.ksk)
    sel = TO.pick(rng, bits, np.asarray(words))
    want = np.empty((n_out, len(words)), np.int64)
    for q, word in enumerate(words):
        s, poly = T.wfa_simulate(nxt, start, weights, word)
        want[:, q] = fin[0, s, 0, :n_out].astype(np.int64) + poly[:n_out]
    u = WO.run_woks(ok, nxt, start, sel, fin, w_val, w_pos, None, n_out)
    assert u[0].shape == (n_out, len(words), N)
    err = _errors(keyset, u, want)
    with capsys.disabled():
        print(f"wfa {what} (before the key switch): {err.size} samples, largest error {np.abs(err).max():.5f}, "
              f"r.m.s. {np.sqrt(np.mean(err**2)):.5f}")
    assert np.abs(err).max() < 1.0 / 32
    r_a, r_b = TO.MO.keyswitch(ok, u)
    assert r_a.shape == (n_out, len(words), n_lwe)
    return decode(r_a, r_b), TO.wrap(want)


@pytest.mark.parametrize("want_max", [True, False])
def test_max_of_3_bit_integers_decrypts(keyset, capsys, want_max):
    """five pairs (equal, x < y, x > y, the extremes): all 15 output bits decrypt to max / min.
    Measured (this seed): largest error 0.00038 (max), 0.00075 (min)."""
    d = 3
    nxt, start, weights, fin = T.wfa_max(d, want_max)
    pairs = [(5, 5), (2, 6), (7, 0), (0, 0), (3, 4)]
    words = [WO.max_word(x, y, d) for x, y in pairs]
    got, _ = _check_real(keyset, capsys, "max" if want_max else "min", nxt, start, weights, fin, words, d,
                         lambda a, b: keyset.decrypt(a.reshape(-1, n_lwe), b.reshape(-1)).reshape(d, -1))
    truth = np.array([_bits(max(x, y) if want_max else min(x, y), d) for x, y in pairs]).T
    assert np.array_equal(got, truth)


def test_popcount_of_7_flags_is_a_lut_digit(keyset, capsys):
    """the count of set flags modulo 8: the phase after the key switch is within 1/32 of (2 c + 1) / 32,
    so the output is a digit tfhe_amd_bootstrap_lut_* accepts.
    Measured (this seed): largest error below 0.00001 before the key switch (every product multiplies
    one digit, 32, of one word)."""
    nxt, start, weights, fin = T.wfa_popcount(7, 8)
    words = [[0] * 7, [1] * 7, [1, 0, 1, 1, 0, 0, 1], [0, 0, 0, 0, 0, 0, 1]]
    got, want = _check_real(keyset, capsys, "popcount", nxt, start, weights, fin, words, 1,
                            lambda a, b: keyset.phase(a.reshape(-1, n_lwe), b.reshape(-1)))
    assert want.reshape(-1).tolist() == [(2 * sum(w) + 1) * 2**27 for w in words]
    assert np.abs(TO.wrap(got.astype(np.int64) - want.reshape(-1))).max() < 2**32 // 32


def test_first_one_of_5_bits_decrypts_one_hot(keyset, capsys):
    """Measured (this seed): largest error 0.00039."""
    nxt, start, weights, fin = T.wfa_first_one(5)
    words = [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 1, 0, 1], [0, 0, 0, 0, 1]]
    got, _ = _check_real(keyset, capsys, "first_one", nxt, start, weights, fin, words, 5,
                         lambda a, b: keyset.decrypt(a.reshape(-1, n_lwe), b.reshape(-1)).reshape(5, -1))
    truth = np.array([[int(1 in w and w.index(1) == f) for w in words] for f in range(5)])
    assert np.array_equal(got, truth)


def test_all_zero_weights_are_the_unweighted_composition_word_for_word(keyset):
    """random words as samples and final weights, a copy state, a bad selector and a fin_index"""
    rng = np.random.default_rng(77)
    g = rng.integers(-2**31, 2**31, (6, 4, 2, N), dtype=np.int64).astype(np.int32)
    ok = TO.key(g, keyset.ksk)
    nxt = np.array([[1, 2], [3, 3], [2, 0], [0, 1]], np.int32)
    fin = rng.integers(-2**31, 2**31, (2, 4, 2, N), dtype=np.int64).astype(np.int32)
    sel = np.array([[0, 1, 2, 3], [5, 6, 4, -1]], np.int32)
    idx = np.array([1, 0], np.int32)
    w_pos = np.array([0, 1023, 7, 7], np.int32)
    want = DO.run_woks(ok, nxt, 0, sel, fin, idx, 3)
    got = WO.run_woks(ok, nxt, 0, sel, fin, np.zeros((4, 2), np.int32), w_pos, idx, 3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # and a weight changes exactly what it should when nothing is multiplied: len = 1 from a copy state
    w_val = np.zeros((4, 2), np.int32)
    w_val[1] = (1234, 1234)
    one = WO.run_woks(ok, nxt, 1, sel[:, :1], fin, w_val, np.array([2], np.int32), idx, 3)
    base = DO.run_woks(ok, nxt, 1, sel[:, :1], fin, idx, 3)
    assert np.array_equal(one[0], base[0])
    assert np.array_equal(one[1][2], TO.wrap(base[1][2].astype(np.int64) + 1234)) and np.array_equal(one[1][:2], base[1][:2])
