"""Leveled automata on the GPU (tfhe_amd_dfa_*): every output word of k_tgsw_dfa_v4
against the oracle composition of tests/dfa_oracle.py, word for word with no tolerance.
Bit-exactness does not need valid ciphertexts, so most cases run on uniformly random words as TGSW
samples, final weights and masks; the last cases run real encryptions and decrypt.  Every case uses
a pool of 24 samples shared by its queries."""
import ctypes

import numpy as np
import pytest

import dev_arena as DA
import dfa_oracle as DO
import tfhe_amd as T
import tgsw_oracle as TO

pytestmark = pytest.mark.gpu

N, n_lwe = 1024, 500
E_ARG = -1
E8 = 1 << 29
COUNT = 24


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _same(got, want):
    return (got[0].shape == want[0].shape and got[1].shape == want[1].shape and
            np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


def _dev(x):
    """x on the GPU, complete before the context's own (non-blocking) stream may touch it"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def _zeros(shape):
    """an output tensor: every word the constant poison of tests/dev_arena.py, not a plausible 0"""
    import torch
    t = DA.poisoned(shape)
    torch.cuda.synchronize()
    return t


_cache = {}


def _random_pool(ctx, keyset):
    """24 samples of uniformly random words: (words, imported set, oracle key), once per session"""
    if "rand" not in _cache:
        words = _rand32(np.random.default_rng(2410), (COUNT, 4, 2, N))
        _cache["rand"] = (words, ctx.tgsw_import(words), TO.key(words, keyset.ksk))
    return _cache["rand"]


def _automaton(rng, Q):
    """random transitions with, from Q = 5 on, a copy state (next0 == next1), a self-loop and a state
    nothing leads to; (next [Q][2], start)"""
    nxt = rng.integers(0, Q, (Q, 2)).astype(np.int32)
    start = 0
    if Q == 2:
        nxt[0] = (1, 0)                       # the start state branches
    if Q >= 5:
        dead = Q - 1
        nxt[nxt == dead] = 1                  # nothing leads to the last state
        nxt[0] = (1, 2)                       # the start state branches
        nxt[1] = (3, 3)                       # a copy
        nxt[2] = (2, 0)                       # a self-loop
        if Q == 64:                           # a wide front: many states live after a few bits
            for s in range(3, 31):
                nxt[s] = (2 * s % 62 + 1, (2 * s + 1) % 62 + 1)
        live = DO.reach(nxt, start, 8)
        assert all(dead not in r for r in live) and 1 in live[1]
    return nxt, start


@pytest.mark.parametrize("length", [1, 2, 3, 7])
@pytest.mark.parametrize("Q", [1, 2, 5, 64])
def test_random_automata(ctx, keyset, Q, length):
    """random words as samples, weights and encrypted-weight masks; two weight tables with a
    fin_index; the extracted samples directly and the key-switched results against the oracle's key
    switch of them"""
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(1000 * Q + length)
    nxt, start = _automaton(rng, Q)
    dfa = ctx.dfa_create(nxt, start, 8)
    try:
        assert (dfa.n_states, dfa.start, dfa.max_len, dfa.device) == (Q, start, 8, ctx.device)
        assert dfa.live(length).tolist() == DO.reach(nxt, start, length)[length]
        for fin_rows in (1, 2):
            fin = _rand32(rng, (2, Q, fin_rows, N))
            for k, n_out in enumerate((1, 3, 16)):
                B = (1, 3)[(k + fin_rows + length) % 2]
                sel = rng.integers(0, COUNT, (B, length)).astype(np.int32)
                idx = np.array([1, 0, 1], np.int32)[:B]
                want_u = DO.run_woks(ok, nxt, start, sel, fin, idx, n_out)
                got_u = ctx.dfa_run_host(tset, dfa, sel, fin, idx, n_out, woks=True)
                assert got_u[0].shape == (n_out, B, N)
                assert _same(got_u, want_u), (Q, length, fin_rows, n_out, B)
                if n_out == 3:
                    assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, idx, n_out), TO.MO.keyswitch(ok, want_u))
        # no fin_index: table 0
        sel = rng.integers(0, COUNT, (3, length)).astype(np.int32)
        assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, None, 2, woks=True),
                     DO.run_woks(ok, nxt, start, sel, fin, None, 2))
    finally:
        dfa.close()


def test_extreme_words(ctx, keyset):
    """a pool of constant -2^31 and 2^31 - 1 words, weights of the same extremes"""
    words = np.empty((4, 4, 2, N), np.int32)
    words[0::2] = -2**31
    words[1::2] = 2**31 - 1
    words[2, :, 1] = 2**31 - 1
    words[3, :, 1] = -2**31
    tset = ctx.tgsw_import(words)
    ok = TO.key(words, keyset.ksk)
    nxt = np.array([[1, 2], [2, 0], [0, 1]], np.int32)
    fin = np.empty((2, 3, 2, N), np.int32)
    fin[0] = -2**31
    fin[1] = 2**31 - 1
    fin[0, 1] = 2**31 - 1
    fin[1, 2, 1, ::2] = -2**31
    sel = np.array([[0, 1, 2, 3], [3, 3, 0, 0], [1, 2, 1, 2]], np.int32)
    idx = np.array([0, 1, 1], np.int32)
    dfa = ctx.dfa_create(nxt, 0, 4)
    try:
        for n_out in (1, 8):
            want = DO.run_woks(ok, nxt, 0, sel, fin, idx, n_out)
            assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, idx, n_out, woks=True), want)
        fin1 = np.ascontiguousarray(fin[:, :, 1:])
        assert _same(ctx.dfa_run_host(tset, dfa, sel, fin1, idx, 2, woks=True),
                     DO.run_woks(ok, nxt, 0, sel, fin1, idx, 2))
    finally:
        dfa.close()
        tset.close()


def test_more_workgroups_than_compute_units(ctx, keyset):
    """B = CUs / 2 + 1 queries of a fully reachable 4-state automaton: 4 B workgroups at the first step"""
    import torch
    _, tset, ok = _random_pool(ctx, keyset)
    B = int(torch.cuda.get_device_properties(0).multi_processor_count) // 2 + 1
    rng = np.random.default_rng(258)
    nxt = np.array([[0, 1], [2, 3], [0, 1], [2, 3]], np.int32)
    assert DO.reach(nxt, 0, 3)[2] == [0, 1, 2, 3]
    sel = rng.integers(0, COUNT, (B, 3)).astype(np.int32)
    fin = _rand32(rng, (1, 4, 1, N))
    dfa = ctx.dfa_create(nxt, 0, 3)
    try:
        assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, woks=True), DO.run_woks(ok, nxt, 0, sel, fin))
    finally:
        dfa.close()


def test_two_slices(ctx, keyset):
    """Q = 64, B = 257: the state scratch holds 256 queries, so the batch runs in two slices; the
    pruning keeps this at three products per query"""
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(2570)
    nxt, start = _automaton(rng, 64)
    B = 257
    sel = rng.integers(0, COUNT, (B, 2)).astype(np.int32)
    fin = _rand32(rng, (2, 64, 1, N))
    idx = rng.integers(0, 2, B).astype(np.int32)
    dfa = ctx.dfa_create(nxt, start, 2)
    try:
        want = DO.run_woks(ok, nxt, start, sel, fin, idx, 2)
        assert _same(ctx.dfa_run_host(tset, dfa, sel, fin, idx, 2, woks=True), want)
    finally:
        dfa.close()


def test_bad_indices(ctx, keyset):
    """device arrays: a selector outside [0, count) gives that step the next[s][0] operand, a fin_index
    outside [0, n_fin) is clamped; the host forms return TFHE_AMD_E_ARG and leave the outputs untouched"""
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(667)
    nxt, start = _automaton(rng, 5)
    fin = _rand32(rng, (2, 5, 2, N))
    sel = np.array([[3, -1, 7, COUNT], [COUNT, 2, -1, 4], [1, 2, 3, -2**31], [-1, -1, COUNT, 2**31 - 1]], np.int32)
    idx = np.array([-1, 2, 1, 0], np.int32)
    dfa = ctx.dfa_create(nxt, start, 4)
    try:
        want = DO.run_woks(ok, nxt, start, sel, fin, idx, 2)
        u_a, u_b = _zeros((2, 4, N)), _zeros((2, 4))
        ctx.dfa_run_dev(tset, dfa, _dev(sel), _dev(fin), u_a, u_b, _dev(idx), 2, woks=True)
        ctx.sync()
        assert _same((u_a.cpu().numpy(), u_b.cpu().numpy()), want)
        # len = 1 with a bad selector: the start state's next0 weights, extracted as they are
        u_a, u_b = _zeros((1, 1, N)), _zeros((1, 1))
        one = np.array([[COUNT]], np.int32)
        ctx.dfa_run_dev(tset, dfa, _dev(one), _dev(fin), u_a, u_b, None, 1, woks=True)
        ctx.sync()
        d0 = fin[0, nxt[start][0]]
        assert _same((u_a.cpu().numpy(), u_b.cpu().numpy()), DO.run_woks(ok, nxt, start, one, fin))
        assert u_b.cpu().numpy()[0, 0] == d0[1][0]
        good = np.clip(sel, 0, COUNT - 1)
        L = T.lib
        for woks, width in ((True, N), (False, n_lwe)):
            f = L.tfhe_amd_dfa_run_woks_host if woks else L.tfhe_amd_dfa_run_host
            for s_, i_ in ((sel, None), (good, idx)):
                o_a, o_b = np.full((2, 4, width), 77, np.int32), np.full((2, 4), 77, np.int32)
                assert f(ctx.h, tset.h, dfa.h, 4, 4, T._p(s_), 2, 2, T._p(fin), T._p(i_), 2, T._p(o_a), T._p(o_b)) == E_ARG
                assert (o_a == 77).all() and (o_b == 77).all()
        # shapes outside the limits: len > max_len, len = 0, n_out = 17 and 0, fin_rows = 3, n_fin = 0
        p = T._p
        o_a, o_b = np.zeros((17, 4, N), np.int32), np.zeros((17, 4), np.int32)
        fin3 = np.zeros((2, 5, 3, N), np.int32)

        def run(B=4, length=4, n_fin=2, rows=2, n_out=2, s_=good, fin_=fin):
            return L.tfhe_amd_dfa_run_woks_host(ctx.h, tset.h, dfa.h, B, length, p(s_), n_fin, rows, p(fin_), None,
                                                n_out, p(o_a), p(o_b))

        assert run() == 0
        assert run(length=5) == E_ARG and run(length=0) == E_ARG and run(n_out=17) == E_ARG and run(n_out=0) == E_ARG
        assert run(rows=3, fin_=fin3) == E_ARG and run(n_fin=0) == E_ARG and run(B=-1) == E_ARG
        assert run(B=0) == 0
        assert L.tfhe_amd_dfa_run_woks_host(ctx.h, tset.h, dfa.h, 4, 4, None, 2, 2, p(fin), None, 2, p(o_a), p(o_b)) == E_ARG
        assert L.tfhe_amd_dfa_run_woks_host(ctx.h, tset.h, dfa.h, 4, 4, p(good), 2, 2, None, None, 2, p(o_a), p(o_b)) == E_ARG
        assert L.tfhe_amd_dfa_run_woks_host(ctx.h, tset.h, dfa.h, 4, 4, p(good), 2, 2, p(fin), None, 2, None, p(o_b)) == E_ARG
        # a host-only automaton is refused by every run
        hdfa = T.Dfa.host(nxt, start, 4)
        with pytest.raises(T.TfheAmdError, match="-1"):
            ctx.dfa_run_host(tset, hdfa, good, fin, None, 2, woks=True)
        hdfa.close()
    finally:
        dfa.close()


def test_same_automaton_on_two_streams_back_to_back(ctx, keyset):
    """two runs in flight share the automaton's state scratch: the second waits for the first"""
    import torch
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(22)
    nxt, start = _automaton(rng, 64)
    dfa = ctx.dfa_create(nxt, start, 7)
    try:
        jobs = []
        for B in (4, 2):
            sel = rng.integers(0, COUNT, (B, 7)).astype(np.int32)
            fin = _rand32(rng, (1, 64, 2, N))
            jobs.append((sel, fin, _dev(sel), _dev(fin), _zeros((3, B, n_lwe)), _zeros((3, B)), torch.cuda.Stream()))
        torch.cuda.synchronize()
        for _, _, d_sel, d_fin, r_a, r_b, st in jobs:
            ctx.dfa_run_dev(tset, dfa, d_sel, d_fin, r_a, r_b, None, 3, stream=st.cuda_stream)
        torch.cuda.synchronize()
        for sel, fin, _, _, r_a, r_b, _ in jobs:
            assert _same((r_a.cpu().numpy(), r_b.cpu().numpy()), DO.run(ok, nxt, start, sel, fin, None, 3))
    finally:
        dfa.close()


def test_automaton_outlives_its_context(keyset):
    """an automaton lives on its context's device, not in the context"""
    rng = np.random.default_rng(6)
    words = _rand32(rng, (3, 4, 2, N))
    nxt, start = T.dfa_contains([1, 0])
    a = T.Context(keyset.bk, keyset.ksk, device=0)
    tset = a.tgsw_import(words)
    dfa = a.dfa_create(nxt, start, 3)
    a.close()
    b = T.Context(keyset.bk, keyset.ksk, device=0)
    try:
        sel = np.array([[0, 1, 2], [2, 2, 1]], np.int32)
        fin = _rand32(rng, (1, 3, 1, N))
        assert _same(b.dfa_run_host(tset, dfa, sel, fin), DO.run(TO.key(words, keyset.ksk), nxt, start, sel, fin))
    finally:
        dfa.close()
        tset.close()
        b.close()


def test_automaton_on_the_wrong_device_is_refused(ctx, keyset):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _, tset, _ = _random_pool(ctx, keyset)
    nxt, start = T.dfa_at_least(1)
    other = T.Context(keyset.bk, keyset.ksk, device=1)
    dfa0, dfa1 = ctx.dfa_create(nxt, start, 2), other.dfa_create(nxt, start, 2)
    oset = other.tgsw_import(np.zeros((1, 4, 2, N), np.int32))
    try:
        sel, fin = np.zeros((1, 2), np.int32), np.zeros((1, 2, 1, N), np.int32)
        for c, s, d in ((other, oset, dfa0), (other, tset, dfa1), (ctx, tset, dfa1)):
            with pytest.raises(T.TfheAmdError, match="-1"):
                c.dfa_run_host(s, d, sel, fin, woks=True)
    finally:
        dfa0.close()
        dfa1.close()
        oset.close()
        other.close()


# ---- real encryptions

def _real_pool(ctx, keyset):
    if "real" not in _cache:
        seed = (ctypes.c_uint32 * 2)(2025, 7)
        T.lib.tfhe_random_generator_setSeed(seed, 2)
        bits = np.random.default_rng(2025).integers(0, 2, COUNT).astype(np.int32)
        bits[:2] = (0, 1)
        g = keyset.tgsw_encrypt(bits)
        _cache["real"] = (bits, g, ctx.tgsw_import(g), TO.key(g, keyset.ksk))
    return _cache["real"]


def test_real_8_bit_comparison_decrypts_and_feeds_a_gate(ctx, keyset):
    """x against y, 8 bits each (len = 16), outputs (x < y, x = y, x > y) as +-1/8: every output equals
    the oracle's and decrypts under the LWE key after the key switch; the lt output is an ordinary
    gate input: AND with a fresh bit decrypts right"""
    bits, _, tset, ok = _real_pool(ctx, keyset)
    rng = np.random.default_rng(88)
    nxt, start, cls = T.dfa_compare()
    vals = np.array([[E8 if c == k else -E8 for k in (T.DFA_LT, T.DFA_EQ, T.DFA_GT)] for c in cls], np.int32)
    fin = T.dfa_fin(vals)
    x = np.concatenate([[0, 255, 77, 77, 128], rng.integers(0, 256, 7)])
    y = np.concatenate([[0, 255, 77, 78, 127], rng.integers(0, 256, 7)])
    B = x.shape[0]
    k = np.arange(7, -1, -1)
    words = np.stack([(x[:, None] >> k) & 1, (y[:, None] >> k) & 1], axis=2).reshape(B, 16)
    sel = TO.pick(rng, bits, words)
    dfa = ctx.dfa_create(nxt, start, 16)
    try:
        r_a, r_b = ctx.dfa_run_host(tset, dfa, sel, fin, None, 3)
        assert _same((r_a, r_b), DO.run(ok, nxt, start, sel, fin, None, 3))
        truth = np.stack([x < y, x == y, x > y]).astype(np.int32)
        assert np.array_equal(keyset.decrypt(r_a.reshape(-1, n_lwe), r_b.reshape(-1)), truth.reshape(-1))
        other = rng.integers(0, 2, B)
        o_a, o_b = keyset.encrypt(other, rng)
        g_a, g_b = ctx.gate_host("AND", r_a[0], r_b[0], o_a, o_b)
        assert np.array_equal(keyset.decrypt(g_a, g_b), truth[0] & other)
    finally:
        dfa.close()


def test_real_contains_decrypts(ctx, keyset):
    """does a 20-bit word contain 1011?  encrypted final weights"""
    bits, _, tset, ok = _real_pool(ctx, keyset)
    rng = np.random.default_rng(1011)
    pat = [1, 0, 1, 1]
    nxt, start = T.dfa_contains(pat)
    vals = np.array([-E8] * 4 + [E8], np.int32)
    plain = T.dfa_fin(vals)
    words = rng.integers(0, 2, (8, 20))
    words[0] = 0
    words[1, -4:] = pat
    sel = TO.pick(rng, bits, words)
    truth = np.array(["1011" in "".join(map(str, w)) for w in words]).astype(np.int32)
    assert truth[0] == 0 and truth[1] == 1
    dfa = ctx.dfa_create(nxt, start, 20)
    try:
        for fin in (plain, keyset.tlwe_encrypt(plain[0, :, 0]).reshape(1, 5, 2, N)):
            r_a, r_b = ctx.dfa_run_host(tset, dfa, sel, fin)
            assert _same((r_a, r_b), DO.run(ok, nxt, start, sel, fin))
            assert np.array_equal(keyset.decrypt(r_a[0], r_b[0]), truth)
    finally:
        dfa.close()


def test_host_and_device_forms_agree_and_name_their_kernels(ctx, keyset):
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(4343)
    nxt, start = _automaton(rng, 5)
    fin = _rand32(rng, (2, 5, 2, N))
    idx = np.array([0, 1, 1], np.int32)
    dfa = ctx.dfa_create(nxt, start, 7)
    names = {1: ["k_tgsw_dfa_v4(weights+extract)"], 2: ["k_tgsw_dfa_v4(weights)", "k_tgsw_dfa_v4(extract)"],
             5: ["k_tgsw_dfa_v4(weights)", "k_tgsw_dfa_v4", "k_tgsw_dfa_v4(extract)"]}
    try:
        for length in (1, 2, 5):
            sel = rng.integers(0, COUNT, (3, length)).astype(np.int32)
            for woks in (True, False):
                host = ctx.dfa_run_host(tset, dfa, sel, fin, idx, 4, woks=woks)
                out_a, out_b = _zeros(host[0].shape), _zeros(host[1].shape)
                ctx.dfa_run_dev(tset, dfa, _dev(sel), _dev(fin), out_a, out_b, _dev(idx), 4, woks=woks)
                kern = ctx.last_kernels()
                ctx.sync()
                assert _same((out_a.cpu().numpy(), out_b.cpu().numpy()), host)
                n = len(names[length])
                assert kern[:n] == names[length], kern
                assert (len(kern) == n) if woks else (len(kern) == n + 1 and kern[n].startswith("k_keyswitch")), kern
            assert _same(host, DO.run(ok, nxt, start, sel, fin, idx, 4))
    finally:
        dfa.close()
