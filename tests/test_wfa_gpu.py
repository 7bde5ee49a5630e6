"""Weighted leveled automata on the GPU (tfhe_amd_wfa_*): every output word of the
weighted instantiations of k_tgsw_dfa_v4 against the oracle composition of tests/wfa_oracle.py, word
for word with no tolerance.  Bit-exactness does not need valid ciphertexts, so the corner cases run
on uniformly random words as TGSW samples and final weights; the three built automata run on real
encryptions and decrypt.  Every device call lies in a tests/dev_arena.py arena: poisoned outputs,
guard bands around every array, inputs compared with their host copies afterwards."""
import ctypes

import numpy as np
import pytest

import dev_arena as DA
import dfa_oracle as DO
import tfhe_amd as T
import tgsw_oracle as TO
import wfa_oracle as WO

pytestmark = pytest.mark.gpu

N, n_lwe = 1024, 500
E_ARG = -1
COUNT = 24


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _same(got, want):
    return (got[0].shape == want[0].shape and got[1].shape == want[1].shape and
            np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


_cache = {}


def _random_pool(ctx, keyset):
    """24 samples of uniformly random words: (imported set, oracle key), once per session"""
    if "rand" not in _cache:
        words = _rand32(np.random.default_rng(3110), (COUNT, 4, 2, N))
        _cache["rand"] = (ctx.tgsw_import(words), TO.key(words, keyset.ksk))
    return _cache["rand"]


def _real_pool(ctx, keyset):
    if "real" not in _cache:
        seed = (ctypes.c_uint32 * 2)(2026, 3)
        T.lib.tfhe_random_generator_setSeed(seed, 2)
        bits = np.random.default_rng(2026).integers(0, 2, COUNT).astype(np.int32)
        bits[:2] = (0, 1)
        g = keyset.tgsw_encrypt(bits)
        _cache["real"] = (bits, ctx.tgsw_import(g), TO.key(g, keyset.ksk))
    return _cache["real"]


def _run_dev(ctx, tset, dfa, sel, fin, weights, idx=None, n_out=1, woks=True, poison="const"):
    """the device form inside an arena -> (out_a, out_b) as numpy, after the band and input checks;
    weights = None: the unweighted tfhe_amd_dfa_run_*_dev"""
    B = sel.shape[0]
    outs = [("out_a", (n_out, B, N if woks else n_lwe)), ("out_b", (n_out, B))]
    inps = [("sel", sel), ("fin", fin)]
    if weights is not None:
        inps += [("w_val", weights[0]), ("w_pos", weights[1])]
    if idx is not None:
        inps.append(("fin_index", idx))
    arena, v = DA.Arena.of("cuda", poison, outs, inps)
    ctx.dfa_run_dev(tset, dfa, v["sel"], v["fin"], v["out_a"], v["out_b"], v.get("fin_index"), n_out, woks=woks,
                    weights=None if weights is None else (v["w_val"], v["w_pos"]))
    kern = ctx.last_kernels()
    ctx.sync()
    arena.check()
    return (v["out_a"].cpu().numpy(), v["out_b"].cpu().numpy()), kern


def _every_form(ctx, tset, ok, dfa, nxt, start, sel, fin, weights, idx, n_out):
    """woks and key-switched, device and host forms, each against the oracle -> the key-switched result"""
    want_u = WO.run_woks(ok, nxt, start, sel, fin, weights[0], weights[1], idx, n_out)
    want_r = TO.MO.keyswitch(ok, want_u)
    assert _same(_run_dev(ctx, tset, dfa, sel, fin, weights, idx, n_out, woks=True)[0], want_u)
    assert _same(_run_dev(ctx, tset, dfa, sel, fin, weights, idx, n_out, woks=False, poison="index")[0], want_r)
    assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, idx, n_out, woks=True, weights=weights), want_u)
    assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, idx, n_out, weights=weights), want_r)
    return want_r


def _bits(v, n):
    return [(v >> f) & 1 for f in range(n)]


PAIRS = [(5, 5), (2, 6), (7, 0), (0, 0), (3, 4)]


def _max_case(ctx, keyset, want_max):
    """max / min at d = 3 over the five pairs on real encryptions: (automaton parts, sel)"""
    bits, tset, ok = _real_pool(ctx, keyset)
    nxt, start, weights, fin = T.wfa_max(3, want_max)
    words = np.array([WO.max_word(x, y, 3) for x, y in PAIRS])
    sel = TO.pick(np.random.default_rng(35 + want_max), bits, words)
    return tset, ok, nxt, start, weights, fin, sel


@pytest.mark.parametrize("want_max", [True, False])
def test_max_and_min_of_3_bit_integers_every_form(ctx, keyset, want_max):
    """d = 3, B = 5: woks and key-switched, device and host forms equal the oracle, and all 15 output
    bits decrypt to max / min"""
    tset, ok, nxt, start, weights, fin, sel = _max_case(ctx, keyset, want_max)
    dfa = ctx.dfa_create(nxt, start, 6)
    try:
        r_a, r_b = _every_form(ctx, tset, ok, dfa, nxt, start, sel, fin, weights, None, 3)
        truth = np.array([_bits(max(x, y) if want_max else min(x, y), 3) for x, y in PAIRS]).T
        assert np.array_equal(keyset.decrypt(r_a.reshape(-1, n_lwe), r_b.reshape(-1)).reshape(3, -1), truth)
    finally:
        dfa.close()


def test_popcount_of_7_flags_modulo_8(ctx, keyset):
    bits, tset, ok = _real_pool(ctx, keyset)
    nxt, start, weights, fin = T.wfa_popcount(7, 8)
    words = np.array([[0] * 7, [1] * 7, [1, 0, 1, 1, 0, 0, 1], [0, 0, 0, 0, 0, 0, 1]])
    sel = TO.pick(np.random.default_rng(78), bits, words)
    dfa = ctx.dfa_create(nxt, start, 7)
    try:
        r_a, r_b = _every_form(ctx, tset, ok, dfa, nxt, start, sel, fin, weights, None, 1)
        want = np.array([(2 * int(w.sum()) + 1) * 2**27 for w in words], np.int64)
        got = keyset.phase(r_a[0], r_b[0]).astype(np.int64)
        assert np.abs(TO.wrap(got - want)).max() < 2**32 // 32        # a LUT digit modulo 8: the slots are 1/8 apart
    finally:
        dfa.close()


def test_first_one_of_5_bits(ctx, keyset):
    bits, tset, ok = _real_pool(ctx, keyset)
    nxt, start, weights, fin = T.wfa_first_one(5)
    words = [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 1, 0, 1], [0, 0, 0, 0, 1]]
    sel = TO.pick(np.random.default_rng(51), bits, np.array(words))
    dfa = ctx.dfa_create(nxt, start, 5)
    try:
        r_a, r_b = _every_form(ctx, tset, ok, dfa, nxt, start, sel, fin, weights, None, 5)
        truth = np.array([[int(1 in w and w.index(1) == f) for w in words] for f in range(5)])
        assert np.array_equal(keyset.decrypt(r_a.reshape(-1, n_lwe), r_b.reshape(-1)).reshape(5, -1), truth)
    finally:
        dfa.close()


def _small(rng):
    """five states: the start state branches, state 1 has one successor but two weights (a product),
    state 3 one successor and one weight (a copy that still adds its weight), state 2 a self-loop;
    random weights elsewhere"""
    nxt = np.array([[1, 2], [3, 3], [2, 0], [4, 4], [0, 3]], np.int32)
    w_val = _rand32(rng, (5, 2))
    w_val[3] = w_val[3, 0]
    assert w_val[1, 0] != w_val[1, 1] and w_val[3, 0] != 0
    return nxt, 0, w_val


@pytest.mark.parametrize("length", [1, 2, 5])
def test_random_weights_names_and_lengths(ctx, keyset, length):
    """len = 1 (the single launch), len = 2 (first + last, no middle step) and len = 5; fin_rows = 1
    and 2 (TLWE final weights) with a fin_index; positions at both ends of the polynomial; the launch
    names of every form"""
    tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(900 + length)
    nxt, start, w_val = _small(rng)
    w_pos = np.array([0, 1023, 5, 5, 517], np.int32)[:length]
    names = {1: ["k_tgsw_dfa_v4(weights+tw+extract)"], 2: ["k_tgsw_dfa_v4(weights+tw)", "k_tgsw_dfa_v4(tw+extract)"],
             5: ["k_tgsw_dfa_v4(weights+tw)", "k_tgsw_dfa_v4(tw)", "k_tgsw_dfa_v4(tw+extract)"]}[length]
    dfa = ctx.dfa_create(nxt, start, 5)
    try:
        for fin_rows in (1, 2):
            fin = _rand32(rng, (2, 5, fin_rows, N))
            sel = rng.integers(0, COUNT, (3, length)).astype(np.int32)
            idx = np.array([1, 0, 1], np.int32)
            n_out = 4 if fin_rows == 1 else 17
            want_u = WO.run_woks(ok, nxt, start, sel, fin, w_val, w_pos, idx, n_out)
            got, kern = _run_dev(ctx, tset, dfa, sel, fin, (w_val, w_pos), idx, n_out, woks=True)
            assert _same(got, want_u), (length, fin_rows)
            assert kern == names, kern
            got, kern = _run_dev(ctx, tset, dfa, sel, fin, (w_val, w_pos), idx, n_out, woks=False, poison="index")
            assert _same(got, TO.MO.keyswitch(ok, want_u))
            assert kern[:-1] == names and kern[-1].startswith("k_keyswitch"), kern
            assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, idx, n_out, woks=True, weights=(w_val, w_pos)), want_u)
        # the weights are seen: the same call without them gives other words
        assert not _same(_run_dev(ctx, tset, dfa, sel, fin, None, idx, 16)[0], tuple(w[:16] for w in want_u))
    finally:
        dfa.close()


def test_one_successor_two_weights_is_a_product(ctx, keyset):
    """a single state with next0 == next1 = itself and w0 != w1 (the popcount's shape on random words):
    every step multiplies; with w0 == w1 the same automaton copies and only adds"""
    tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(11)
    nxt = np.array([[0, 0]], np.int32)
    fin = _rand32(rng, (1, 1, 2, N))
    sel = rng.integers(0, COUNT, (2, 3)).astype(np.int32)
    w_pos = np.array([1, 0, 1], np.int32)
    dfa = ctx.dfa_create(nxt, 0, 3)
    try:
        for w_val in (np.array([[-7, 2**31 - 1]], np.int32), np.array([[12345, 12345]], np.int32)):
            want = WO.run_woks(ok, nxt, 0, sel, fin, w_val, w_pos, None, 2)
            assert _same(_run_dev(ctx, tset, dfa, sel, fin, (w_val, w_pos), None, 2)[0], want)
        # the copy: fin with 12345 added twice at coefficient 1 and once at coefficient 0, nothing else
        assert want[1][:, 0].tolist() == [int(TO.wrap(np.int64(fin[0, 0, 1, f]) + k * 12345)) for f, k in ((0, 1), (1, 2))]
    finally:
        dfa.close()


def test_bad_selectors_and_positions_on_the_device_forms(ctx, keyset):
    """device arrays: a selector outside [0, count) gives d0 + w0 X^p, a w_pos outside [0, 1024) makes
    its step weightless, a fin_index is clamped"""
    tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(668)
    nxt, start, w_val = _small(rng)
    fin = _rand32(rng, (2, 5, 2, N))
    sel = np.array([[3, -1, 7, COUNT], [COUNT, 2, -1, 4], [1, 2, 3, -2**31], [-1, -1, COUNT, 2**31 - 1]], np.int32)
    idx = np.array([-1, 2, 1, 0], np.int32)
    dfa = ctx.dfa_create(nxt, start, 4)
    try:
        for w_pos in ([3, 3, 0, 1], [1024, 2, -1, 3], [-2**31, 2**31 - 1, 1024, 4096]):
            w_pos = np.array(w_pos, np.int32)
            want = WO.run_woks(ok, nxt, start, sel, fin, w_val, w_pos, idx, 4)
            assert _same(_run_dev(ctx, tset, dfa, sel, fin, (w_val, w_pos), idx, 4)[0], want), w_pos
        # every position bad: the unweighted run's words
        assert _same(want, DO.run_woks(ok, nxt, start, sel, fin, idx, 4))
        # len = 1 with a bad selector: the start state's next0 weights plus w0, extracted as they are
        one = np.array([[COUNT]], np.int32)
        got = _run_dev(ctx, tset, dfa, one, fin, (w_val, np.array([2], np.int32)), None, 3)[0]
        d0 = fin[0, nxt[start][0]]
        assert got[1][:, 0].tolist() == [int(d0[1][0]), int(d0[1][1]), int(TO.wrap(np.int64(d0[1][2]) + w_val[start][0]))]
        assert _same(got, WO.run_woks(ok, nxt, start, one, fin, w_val, [2], None, 3))
    finally:
        dfa.close()


def test_all_zero_weights_give_the_unweighted_words(ctx, keyset):
    tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(5)
    nxt, start, _ = _small(rng)
    fin = _rand32(rng, (2, 5, 2, N))
    sel = rng.integers(0, COUNT, (3, 4)).astype(np.int32)
    idx = np.array([0, 1, 1], np.int32)
    zero = (np.zeros((5, 2), np.int32), np.array([9, 0, 1023, 4], np.int32))
    dfa = ctx.dfa_create(nxt, start, 4)
    try:
        for woks in (True, False):
            plain = _run_dev(ctx, tset, dfa, sel, fin, None, idx, 3, woks=woks)[0]
            assert _same(_run_dev(ctx, tset, dfa, sel, fin, zero, idx, 3, woks=woks)[0], plain)
            assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, idx, 3, woks=woks, weights=zero), plain)
        assert _same(plain, DO.run(ok, nxt, start, sel, fin, idx, 3))
    finally:
        dfa.close()


def test_64_outputs_of_the_64_bit_maximum(ctx, keyset):
    """d = 64, len = 128, n_out = 64, B = 3: every thread below n_out writes a b word; real encryptions,
    all 192 bits decrypt"""
    bits, tset, ok = _real_pool(ctx, keyset)
    nxt, start, weights, fin = T.wfa_max(64)
    rng = np.random.default_rng(64)
    x = [int(v) for v in rng.integers(0, 2**63, 3, dtype=np.uint64) * 2 + rng.integers(0, 2, 3, dtype=np.uint64)]
    y = [x[0], x[1] ^ 1, int(rng.integers(0, 2**63, dtype=np.uint64))]
    words = np.array([WO.max_word(a, b, 64) for a, b in zip(x, y)])
    sel = TO.pick(rng, bits, words)
    dfa = ctx.dfa_create(nxt, start, 128)
    try:
        want_u = WO.run_woks(ok, nxt, start, sel, fin, weights[0], weights[1], None, 64)
        assert _same(_run_dev(ctx, tset, dfa, sel, fin, weights, None, 64, woks=True)[0], want_u)
        got = _run_dev(ctx, tset, dfa, sel, fin, weights, None, 64, woks=False, poison="index")[0]
        assert _same(got, TO.MO.keyswitch(ok, want_u))
        truth = np.array([_bits(max(a, b), 64) for a, b in zip(x, y)]).T
        assert np.array_equal(keyset.decrypt(got[0].reshape(-1, n_lwe), got[1].reshape(-1)).reshape(64, -1), truth)
        # the unweighted forms keep their limit of 16 outputs
        o_a, o_b = np.full((17, 3, N), 77, np.int32), np.full((17, 3), 77, np.int32)
        assert T.lib.tfhe_amd_dfa_run_woks_host(ctx.h, tset.h, dfa.h, 3, 128, T._p(sel), 1, 1, T._p(fin), None, 17,
                                                T._p(o_a), T._p(o_b)) == E_ARG
        assert (o_a == 77).all() and (o_b == 77).all()
    finally:
        dfa.close()


def test_two_slices(ctx, keyset):
    """Q = 64, B = 257: the state scratch holds 256 queries, so the batch runs in two slices; the
    transitions are a small automaton's (three live states, three products per query), the other 61
    states loop on themselves"""
    tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(2571)
    nxt = np.array([[s, s] for s in range(64)], np.int32)
    nxt[:3] = [[1, 2], [3, 3], [2, 0]]
    w_val = _rand32(rng, (64, 2))
    B = 257
    sel = rng.integers(0, COUNT, (B, 2)).astype(np.int32)
    fin = _rand32(rng, (2, 64, 1, N))
    idx = rng.integers(0, 2, B).astype(np.int32)
    w_pos = np.array([1000, 1], np.int32)
    dfa = ctx.dfa_create(nxt, 0, 2)
    try:
        want = WO.run_woks(ok, nxt, 0, sel, fin, w_val, w_pos, idx, 2)
        assert _same(_run_dev(ctx, tset, dfa, sel, fin, (w_val, w_pos), idx, 2)[0], want)
    finally:
        dfa.close()


def test_host_forms_refuse_and_write_nothing(ctx, keyset):
    tset, _ = _random_pool(ctx, keyset)
    rng = np.random.default_rng(404)
    nxt, start, w_val = _small(rng)
    fin = _rand32(rng, (2, 5, 2, N))
    good = rng.integers(0, COUNT, (4, 4)).astype(np.int32)
    bad_sel = good.copy()
    bad_sel[2, 1] = COUNT
    w_pos = np.array([0, 1, 2, 1023], np.int32)
    idx = np.array([0, 1, 2, 0], np.int32)          # 2 of 2 tables
    L, p = T.lib, T._p
    dfa = ctx.dfa_create(nxt, start, 4)
    try:
        for woks, width in ((True, N), (False, n_lwe)):
            f = L.tfhe_amd_wfa_run_woks_host if woks else L.tfhe_amd_wfa_run_host
            o_a, o_b = np.full((65, 4, width), 77, np.int32), np.full((65, 4), 77, np.int32)

            def run(B=4, length=4, s_=good, wv=w_val, wp=w_pos, n_fin=2, rows=2, fin_=fin, i_=None, n_out=2, a=o_a, b=o_b):
                return f(ctx.h, tset.h, dfa.h, B, length, p(s_), p(wv), p(wp), n_fin, rows, p(fin_), p(i_), n_out, p(a), p(b))

            for wp in ([0, 1, 1024, 3], [-1, 1, 2, 3]):
                assert run(wp=np.array(wp, np.int32)) == E_ARG
            assert run(s_=bad_sel) == E_ARG and run(i_=idx) == E_ARG
            assert run(wv=None) == E_ARG and run(wp=None) == E_ARG and run(s_=None) == E_ARG and run(fin_=None) == E_ARG
            assert run(a=None) == E_ARG and run(b=None) == E_ARG
            assert run(length=5) == E_ARG and run(length=0) == E_ARG and run(n_out=65) == E_ARG and run(n_out=0) == E_ARG
            assert run(rows=3) == E_ARG and run(n_fin=0) == E_ARG and run(B=-1) == E_ARG
            assert (o_a == 77).all() and (o_b == 77).all()
            assert run(B=0) == 0 and run(B=0, wv=None, wp=None) == 0 and (o_a == 77).all() and (o_b == 77).all()
            assert run() == 0 and (o_a[:2] != 77).any() and (o_a[2:] == 77).all() and (o_b[2:] == 77).all()
        # the device forms refuse null weight arrays too, and a host-only automaton
        import torch
        d_sel, d_fin = torch.from_numpy(good).cuda(), torch.from_numpy(fin).cuda()
        u_a, u_b = DA.poisoned((2, 4, N)), DA.poisoned((2, 4))
        torch.cuda.synchronize()
        for wv, wp in ((None, d_sel.data_ptr()), (d_sel.data_ptr(), None)):
            assert L.tfhe_amd_wfa_run_woks_dev(ctx.h, tset.h, dfa.h, 4, 4, d_sel.data_ptr(), wv, wp, 2, 2, d_fin.data_ptr(),
                                               None, 2, u_a.data_ptr(), u_b.data_ptr(), None) == E_ARG
        ctx.sync()
        assert (u_a == DA.POISON_I32).all() and (u_b == DA.POISON_I32).all()
        hdfa = T.Dfa.host(nxt, start, 4)
        with pytest.raises(T.TfheAmdError, match="-1"):
            ctx.dfa_run_host(tset, hdfa, good, fin, None, 2, woks=True, weights=(w_val, w_pos))
        hdfa.close()
    finally:
        dfa.close()


def test_maximum_bits_are_ordinary_gate_inputs(ctx, keyset):
    """the chain: the d = 3 maximum's outputs through a NAND gate batch with themselves decrypt to the
    complement of max(x, y)"""
    tset, ok, nxt, start, weights, fin, sel = _max_case(ctx, keyset, True)
    dfa = ctx.dfa_create(nxt, start, 6)
    try:
        r_a, r_b = ctx.dfa_run_host(tset, dfa, sel, fin, None, 3, weights=weights)
        a, b = np.ascontiguousarray(r_a.reshape(-1, n_lwe)), np.ascontiguousarray(r_b.reshape(-1))
        g_a, g_b = ctx.gate_host("NAND", a, b, a, b)
        truth = np.array([_bits(max(x, y), 3) for x, y in PAIRS]).T.reshape(-1)
        assert np.array_equal(keyset.decrypt(a, b), truth)
        assert np.array_equal(keyset.decrypt(g_a, g_b), 1 - truth)
    finally:
        dfa.close()
