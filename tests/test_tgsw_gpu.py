"""Leveled table lookup on the GPU (tfhe_amd_tgsw_*): every output word of
k_tgsw_lookup_v4 and k_tgsw_cmux_v4 against the oracle composition of tests/tgsw_oracle.py, word for
word with no tolerance.  Bit-exactness does not need valid ciphertexts, so most cases run on
uniformly random words as TGSW samples, tables and masks; the last cases run real encryptions and
decrypt.  Every case uses a pool of at most 24 samples shared by its queries."""
import ctypes

import numpy as np
import pytest

import dev_arena as DA
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
        words = _rand32(np.random.default_rng(2401), (COUNT, 4, 2, N))
        _cache["rand"] = (words, ctx.tgsw_import(words), TO.key(words, keyset.ksk))
    return _cache["rand"]


def _queries(rng, d, n_tab):
    """B = 1 and B = 3 with distinct selectors, B = 3 with shared ones; a table index per query"""
    distinct = rng.permutation(COUNT)[:3 * d].reshape(3, d) if 3 * d <= COUNT else rng.integers(0, COUNT, (3, d))
    shared = np.tile(rng.integers(0, COUNT, (1, d)), (3, 1))
    idx = np.array([1, 0, 1], np.int32) % n_tab
    return [(distinct[:1].astype(np.int32), idx[:1]), (distinct.astype(np.int32), idx), (shared.astype(np.int32), idx)]


@pytest.mark.parametrize("tab_rows", [1, 2])
@pytest.mark.parametrize("d_h,log_stride,n_out", [(1, 0, 1), (10, 0, 1), (1, 1, 2), (1, 4, 16), (1, 3, 8),
                                                  (6, 4, 16), (7, 3, 8)])
def test_lookup_random_words(ctx, keyset, d_h, log_stride, n_out, tab_rows):
    """random words as samples, tables and encrypted-table masks; two tables with a tab_index; the
    extracted samples and the key-switched results, function-major"""
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(100 * d_h + 10 * log_stride + tab_rows)
    tab = _rand32(rng, (2, 1, tab_rows, N))
    for sel, idx in _queries(rng, d_h, 2):
        B = sel.shape[0]
        want_u = TO.lookup_woks(ok, sel, tab, idx, log_stride, n_out)
        got_u = ctx.tgsw_lookup_host(tset, sel, tab, idx, log_stride, n_out, woks=True)
        assert got_u[0].shape == (n_out, B, N)
        assert _same(got_u, want_u), (B, d_h, log_stride, n_out)
        got_r = ctx.tgsw_lookup_host(tset, sel, tab, idx, log_stride, n_out)
        assert _same(got_r, TO.MO.keyswitch(ok, want_u))
    # no tab_index: table 0
    sel, _ = _queries(rng, d_h, 2)[1]
    assert _same(ctx.tgsw_lookup_host(tset, sel, tab, None, log_stride, n_out, woks=True),
                 TO.lookup_woks(ok, sel, tab, None, log_stride, n_out))


def test_lookup_extreme_words(ctx, keyset):
    """a pool of constant -2^31 and 2^31 - 1 words, tables of the same extremes"""
    words = np.empty((4, 4, 2, N), np.int32)
    words[0::2] = -2**31
    words[1::2] = 2**31 - 1
    words[2, :, 1] = 2**31 - 1
    words[3, :, 1] = -2**31
    tset = ctx.tgsw_import(words)
    ok = TO.key(words, keyset.ksk)
    tab = np.empty((2, 1, 2, N), np.int32)
    tab[0] = -2**31
    tab[1] = 2**31 - 1
    tab[1, 0, 1, ::2] = -2**31
    sel = np.array([[0, 1, 2, 3], [3, 3, 0, 0], [1, 2, 1, 2]], np.int32)
    idx = np.array([0, 1, 1], np.int32)
    try:
        for ls, n_out in ((0, 1), (3, 8)):
            want = TO.lookup_woks(ok, sel, tab, idx, ls, n_out)
            assert _same(ctx.tgsw_lookup_host(tset, sel, tab, idx, ls, n_out, woks=True), want)
    finally:
        tset.close()


def test_lookup_more_queries_than_compute_units(ctx, keyset):
    import torch
    _, tset, ok = _random_pool(ctx, keyset)
    B = int(torch.cuda.get_device_properties(0).multi_processor_count) + 1
    rng = np.random.default_rng(257)
    sel = rng.integers(0, COUNT, (B, 4)).astype(np.int32)
    tab = _rand32(rng, (1, 1, 1, N))
    want = TO.lookup_woks(ok, sel, tab)
    assert _same(ctx.tgsw_lookup_host(tset, sel, tab, woks=True), want)


@pytest.mark.parametrize("n_poly,tab_rows", [(2, 1), (2, 2), (16, 1), (16, 2)])
def test_lookup_vertical_packing(ctx, keyset, n_poly, tab_rows):
    """the CMux tree on the address bits d_h .. d - 1, one launch per level, then d_h = 3 steps"""
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(1600 + n_poly + tab_rows)
    levels = n_poly.bit_length() - 1
    d = 3 + levels
    sel = rng.integers(0, COUNT, (3, d)).astype(np.int32)
    tab = _rand32(rng, (2, n_poly, tab_rows, N))
    idx = np.array([1, 0, 1], np.int32)
    want_u = TO.lookup_woks(ok, sel, tab, idx, 2, 3)
    assert _same(ctx.tgsw_lookup_host(tset, sel, tab, idx, 2, 3, woks=True), want_u)
    kern = ctx.last_kernels()
    assert kern == [f"k_tgsw_cmux_v4(tree-level-{l})" for l in range(levels)] + ["k_tgsw_lookup_v4"], kern
    assert _same(ctx.tgsw_lookup_host(tset, sel, tab, idx, 2, 3), TO.MO.keyswitch(ok, want_u))
    kern = ctx.last_kernels()
    assert len(kern) == levels + 2 and kern[levels] == "k_tgsw_lookup_v4" and kern[-1].startswith("k_keyswitch"), kern
    # d_h = 0: the tree alone picks the polynomial, coefficient 0 .. n_out - 1 read as they are
    sel0 = np.ascontiguousarray(sel[:, 3:])
    assert _same(ctx.tgsw_lookup_host(tset, sel0, tab, idx, 4, 16, woks=True), TO.lookup_woks(ok, sel0, tab, idx, 4, 16))


def test_cmux_kernel_aliasing_and_external_product(ctx, keyset):
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(77)
    B = 5
    sel = rng.integers(0, COUNT, B).astype(np.int32)
    d0, d1 = _rand32(rng, (B, 2, N)), _rand32(rng, (B, 2, N))
    want = np.stack([TO.cmux(ok, int(sel[w]), d1[w], d0[w]) for w in range(B)])
    t_sel = _dev(sel)
    out = _zeros((B, 2, N))
    ctx.tgsw_cmux_dev(tset, t_sel, _dev(d1), _dev(d0), out)
    assert ctx.last_kernels() == ["k_tgsw_cmux_v4"]
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), want)
    for alias in (0, 1):          # out = d0, out = d1
        t0, t1 = _dev(d0), _dev(d1)
        ctx.tgsw_cmux_dev(tset, t_sel, t1, t0, (t0, t1)[alias])
        ctx.sync()
        assert np.array_equal((t0, t1)[alias].cpu().numpy(), want), alias
        assert np.array_equal((t0, t1)[1 - alias].cpu().numpy(), (d0, d1)[1 - alias])
    # d0 = NULL: the external product; on the bootstrapping key's own words imported as a set it is
    # tfhe_amd_external_product_dev's result
    kset = ctx.tgsw_import(keyset.bk[:COUNT])
    try:
        ctx.tgsw_cmux_dev(kset, t_sel, _dev(d1), None, out)
        acc = _dev(d1)
        T._check(T.lib.tfhe_amd_external_product_dev(ctx.h, B, t_sel.data_ptr(), acc.data_ptr(), None), "xp")
        ctx.sync()
        assert np.array_equal(out.cpu().numpy(), acc.cpu().numpy())
        kkey = TO.key(keyset.bk[:COUNT], keyset.ksk)
        assert np.array_equal(out.cpu().numpy(), np.stack([TO.cmux(kkey, int(sel[w]), d1[w]) for w in range(B)]))
    finally:
        kset.close()


def test_bad_indices(ctx, keyset):
    """device arrays: a selector outside [0, count) skips its step in the lookup and gives d0 in the
    CMux kernel, a tab_index outside [0, n_tab) is clamped; the host forms return TFHE_AMD_E_ARG"""
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(666)
    tab = _rand32(rng, (2, 2, 1, N))
    sel = np.array([[3, -1, 7, COUNT, 5], [COUNT, 2, -1, 4, -1], [1, 2, 3, 4, COUNT]], np.int32)   # d_h = 4 + one tree bit
    idx = np.array([-1, 2, 1], np.int32)
    want = TO.lookup_woks(ok, sel, tab, idx, 1, 2)
    u_a = _zeros((2, 3, N))
    u_b = _zeros((2, 3))
    ctx.tgsw_lookup_dev(tset, _dev(sel), _dev(tab), u_a, u_b, _dev(idx), 1, 2, woks=True)
    ctx.sync()
    assert _same((u_a.cpu().numpy(), u_b.cpu().numpy()), want)
    d0, d1 = _rand32(rng, (3, 2, N)), _rand32(rng, (3, 2, N))
    out = _zeros((3, 2, N))
    bad = np.array([-1, COUNT, 2], np.int32)
    ctx.tgsw_cmux_dev(tset, _dev(bad), _dev(d1), _dev(d0), out)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.array_equal(got[:2], d0[:2]) and np.array_equal(got[2], TO.cmux(ok, 2, d1[2], d0[2]))
    good = np.clip(sel, 0, COUNT - 1)
    with pytest.raises(T.TfheAmdError, match="-1"):
        ctx.tgsw_lookup_host(tset, sel, tab, None, 1, 2)
    with pytest.raises(T.TfheAmdError, match="-1"):
        ctx.tgsw_lookup_host(tset, good, tab, idx, 1, 2, woks=True)
    # shapes outside the limits: d_h + log_stride > 10, n_out > 2^log_stride, n_out > 16
    with pytest.raises(T.TfheAmdError, match="-1"):
        ctx.tgsw_lookup_host(tset, np.zeros((1, 11), np.int32), tab[:, :1], None, 0, 1)
    with pytest.raises(T.TfheAmdError, match="-1"):
        ctx.tgsw_lookup_host(tset, good, tab, None, 1, 3)
    with pytest.raises(T.TfheAmdError, match="-1"):
        ctx.tgsw_lookup_host(tset, good[:, :3], tab, None, 5, 17)
    assert T.lib.tfhe_amd_tgsw_cmux_dev(ctx.h, None, 1, out.data_ptr(), out.data_ptr(), None, out.data_ptr(), None) == E_ARG


def _real_pool(ctx, keyset):
    if "real" not in _cache:
        seed = (ctypes.c_uint32 * 2)(2024, 6)
        T.lib.tfhe_random_generator_setSeed(seed, 2)
        bits = np.random.default_rng(2024).integers(0, 2, COUNT).astype(np.int32)
        bits[:2] = (0, 1)
        g = keyset.tgsw_encrypt(bits)
        _cache["real"] = (bits, g, ctx.tgsw_import(g), TO.key(g, keyset.ksk))
    return _cache["real"]


def test_real_lookup_1024_entries_decrypts_and_feeds_a_gate(ctx, keyset):
    """a 1024-entry +-1/8 table at d_h = 10 on real TGSW encryptions: every output equals the
    oracle's, decrypts to its table entry under the LWE key after the key switch, and is an
    ordinary gate input: NAND with a fresh bit decrypts right"""
    bits, _, tset, ok = _real_pool(ctx, keyset)
    rng = np.random.default_rng(1024)
    table = (rng.integers(0, 2, N) * 2 - 1) * E8
    addr = np.concatenate([[0, N - 1], rng.integers(0, N, 10)])
    sel = TO.pick(rng, bits, (addr[:, None] >> np.arange(10)) & 1)
    tab = table.astype(np.int32).reshape(1, 1, 1, N)
    r_a, r_b = ctx.tgsw_lookup_host(tset, sel, tab)
    assert _same((r_a, r_b), TO.lookup(ok, sel, tab))
    entry = (table[addr] > 0).astype(np.int32)
    assert np.array_equal(keyset.decrypt(r_a[0], r_b[0]), entry)
    other = rng.integers(0, 2, addr.shape[0])
    o_a, o_b = keyset.encrypt(other, rng)
    g_a, g_b = ctx.gate_host("NAND", r_a[0], r_b[0], o_a, o_b)
    assert np.array_equal(keyset.decrypt(g_a, g_b), 1 - (entry & other))


def test_real_lookup_128_bytes_at_stride_8(ctx, keyset):
    """a 128 x 8-bit table, one bit per word: 8 outputs per query from 7 CMux steps; encrypted table"""
    bits, _, tset, ok = _real_pool(ctx, keyset)
    rng = np.random.default_rng(128)
    table = (rng.integers(0, 2, N) * 2 - 1) * E8
    addr = np.concatenate([[0, 127], rng.integers(0, 128, 4)])
    sel = TO.pick(rng, bits, (addr[:, None] >> np.arange(7)) & 1)
    want = np.stack([table[addr * 8 + f] for f in range(8)])
    for tab in (table.astype(np.int32).reshape(1, 1, 1, N), keyset.tlwe_encrypt(table).reshape(1, 1, 2, N)):
        r_a, r_b = ctx.tgsw_lookup_host(tset, sel, tab, None, 3, 8)
        assert _same((r_a, r_b), TO.lookup(ok, sel, tab, None, 3, 8))
        assert np.array_equal(keyset.decrypt(r_a.reshape(-1, n_lwe), r_b.reshape(-1)),
                              (want.reshape(-1) > 0).astype(np.int32))


def test_host_and_device_forms_agree_and_name_their_kernels(ctx, keyset):
    _, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(4242)
    sel = rng.integers(0, COUNT, (3, 6)).astype(np.int32)
    tab = _rand32(rng, (2, 4, 2, N))
    idx = np.array([0, 1, 1], np.int32)
    for woks in (True, False):
        host = ctx.tgsw_lookup_host(tset, sel, tab, idx, 2, 4, woks=woks)
        out_a = _zeros(host[0].shape)
        out_b = _zeros(host[1].shape)
        ctx.tgsw_lookup_dev(tset, _dev(sel), _dev(tab), out_a, out_b, _dev(idx), 2, 4, woks=woks)
        kern = ctx.last_kernels()
        ctx.sync()
        assert _same((out_a.cpu().numpy(), out_b.cpu().numpy()), host)
        assert kern[:3] == ["k_tgsw_cmux_v4(tree-level-0)", "k_tgsw_cmux_v4(tree-level-1)", "k_tgsw_lookup_v4"], kern
        assert (len(kern) == 3) if woks else (len(kern) == 4 and kern[3].startswith("k_keyswitch")), kern
    assert _same(host, TO.lookup(ok, sel, tab, idx, 2, 4))


def test_import_destroy_import_again(ctx, keyset):
    words, tset, ok = _random_pool(ctx, keyset)
    rng = np.random.default_rng(99)
    sel = rng.integers(0, COUNT, (2, 5)).astype(np.int32)
    tab = _rand32(rng, (1, 2, 1, N))
    first = ctx.tgsw_lookup_host(tset, sel, tab, woks=True)
    for _ in range(2):
        again = ctx.tgsw_import(words)
        assert len(again) == COUNT
        got = ctx.tgsw_lookup_host(again, sel, tab, woks=True)
        again.close()
        assert len(again) == 0
        assert _same(got, first)
    assert _same(first, TO.lookup_woks(ok, sel, tab))


def test_set_outlives_its_context(keyset):
    """a set lives on its context's device, not in the context"""
    rng = np.random.default_rng(5)
    words = _rand32(rng, (3, 4, 2, N))
    a = T.Context(keyset.bk, keyset.ksk, device=0)
    tset = a.tgsw_import(words)
    a.close()
    b = T.Context(keyset.bk, keyset.ksk, device=0)
    try:
        sel = np.array([[0, 1, 2]], np.int32)
        tab = _rand32(rng, (1, 1, 1, N))
        assert _same(b.tgsw_lookup_host(tset, sel, tab), TO.lookup(TO.key(words, keyset.ksk), sel, tab))
    finally:
        tset.close()
        b.close()


def test_set_on_the_wrong_device_is_refused(ctx, keyset):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _, tset, _ = _random_pool(ctx, keyset)
    other = T.Context(keyset.bk, keyset.ksk, device=1)
    try:
        with pytest.raises(T.TfheAmdError, match="-1"):
            other.tgsw_lookup_host(tset, np.zeros((1, 2), np.int32), np.zeros((1, 1, 1, N), np.int32), woks=True)
    finally:
        other.close()
