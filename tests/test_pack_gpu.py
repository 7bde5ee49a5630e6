"""Packing key switch on the GPU (tfhe_amd_pack_*): every output word of
k_pack_digits + k_pack_v4 against the oracle of tests/pack_oracle.py, word for word with no
tolerance.  Bit-exactness does not need valid ciphertexts, so most cases run on uniformly random
words as key and inputs; the last cases run real gate outputs through a generated key, decrypt, and
feed the leveled lookup."""
import ctypes

import numpy as np
import pytest

import dev_arena as DA
import pack_oracle as PO
import tfhe_amd as T
import tgsw_oracle as TO

pytestmark = pytest.mark.gpu

N, n_lwe = 1024, 500
E_ARG = -1


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


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


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


SPLIT, WHOLE = ["k_pack_digits", "k_pack_v4(split)"], ["k_pack_digits", "k_pack_v4"]
_cache = {}


def _random_key(ctx):
    """a key of uniformly random words: (words, imported key), once per session"""
    if "rand" not in _cache:
        words = _rand32(np.random.default_rng(3701), (n_lwe, 6, 2, N))
        _cache["rand"] = (words, ctx.pack_key_import(words))
    return _cache["rand"]


def _real_key(ctx, keyset):
    """a generated key and 1 024 NAND outputs of gate_host with their truth table"""
    if "real" not in _cache:
        T.lib.tfhe_random_generator_setSeed((ctypes.c_uint32 * 2)(2025, 7), 2)
        words = keyset.pack_key()
        rng = np.random.default_rng(2025)
        x, y = rng.integers(0, 2, N), rng.integers(0, 2, N)
        g_a, g_b = ctx.gate_host("NAND", *keyset.encrypt(x, rng), *keyset.encrypt(y, rng))
        _cache["real"] = (words, ctx.pack_key_import(words), 1 - (x & y), np.ascontiguousarray(g_a),
                          np.ascontiguousarray(g_b))
    return _cache["real"]


@pytest.mark.parametrize("T_,P,pos", [(1, 1, None), (1, N, None), (3, 5, [0, 1, 511, 512, 1023]), (2, 64, "perm")])
def test_shapes_random_words(ctx, T_, P, pos):
    words, pkey = _random_key(ctx)
    rng = np.random.default_rng(1000 * T_ + P)
    if pos == "perm":
        pos = rng.permutation(N)[:P]
    in_a, in_b = _rand32(rng, (T_, P, n_lwe)), _rand32(rng, (T_, P))
    got = ctx.pack_host(pkey, in_a, in_b, pos)
    assert ctx.last_kernels() == SPLIT
    assert got.shape == (T_, 2, N)
    assert np.array_equal(got, PO.pack_rows(words, in_a, in_b, pos))


def test_split_and_whole_forms(ctx):
    """T = 1 splits each output's key rows over the most workgroups; the first T above the device's
    compute units takes one workgroup per output.  P = 1 at a scattered position keeps the oracle
    (input by input) cheap; T = 1 is also checked row by row."""
    words, pkey = _random_key(ctx)
    rng = np.random.default_rng(555)
    for T_, kern in ((1, SPLIT), (_cus(), SPLIT), (_cus() + 1, WHOLE)):
        in_a, in_b = _rand32(rng, (T_, 1, n_lwe)), _rand32(rng, (T_, 1))
        pos = np.array([777], np.int32)
        got = ctx.pack_host(pkey, in_a, in_b, pos)
        assert ctx.last_kernels() == kern, (T_, ctx.last_kernels())
        assert np.array_equal(got, PO.pack_inputs(words, in_a, in_b, pos)), T_
        if T_ == 1:
            assert np.array_equal(got, PO.pack_rows(words, in_a, in_b, pos))


@pytest.mark.parametrize("key_words", [-2**31, 2**31 - 1, None])
def test_extreme_words(ctx, key_words):
    """the lazy reductions: a key of all -2^31, all 2^31 - 1 and random words, each with 1 024 inputs
    whose digits are all -8 (0x77777800) and all +7 (0x77777700), T = 1 (split form)"""
    rng = np.random.default_rng(88)
    words = _rand32(rng, (n_lwe, 6, 2, N)) if key_words is None else np.full((n_lwe, 6, 2, N), key_words, np.int32)
    pkey = ctx.pack_key_import(words)
    try:
        for a_word in (0x77777800, 0x77777700):
            in_a = np.full((1, N, n_lwe), a_word, np.int32)
            in_b = _rand32(rng, (1, N))
            got = ctx.pack_host(pkey, in_a, in_b)
            assert np.array_equal(got, PO.pack_rows(words, in_a, in_b)), hex(a_word)
    finally:
        pkey.close()


@pytest.mark.parametrize("key_words", [-2**31, 2**31 - 1, None])
def test_extreme_words_one_workgroup_per_output(ctx, key_words):
    """the chunk bound: in the unsplit form one workgroup runs all 250 units of an output and so
    sums every full chunk of 252 rows in the NTT domain.  With a constant key and constant digits
    every row's product has the same sign and the chunk sum reaches 252 * 1024 * 8 * 2^31.
    T = compute units + 1 outputs, alternately the all -8 and the all +7 inputs, P = 1 024, filled
    on the device"""
    import torch
    rng = np.random.default_rng(89)
    words = _rand32(rng, (n_lwe, 6, 2, N)) if key_words is None else np.full((n_lwe, 6, 2, N), key_words, np.int32)
    pkey = ctx.pack_key_import(words)
    T_ = _cus() + 1
    try:
        in_a = torch.empty((T_, N, n_lwe), dtype=torch.int32, device="cuda")
        in_a[0::2] = 0x77777800
        in_a[1::2] = 0x77777700
        b = _rand32(rng, (1, N))
        in_b = _dev(np.ascontiguousarray(np.broadcast_to(b, (T_, N))))
        out = _zeros((T_, 2, N))
        ctx.pack_dev(pkey, in_a, in_b, out)
        assert ctx.last_kernels() == WHOLE
        ctx.sync()
        got = out.cpu().numpy()
        two = np.stack([np.full((N, n_lwe), 0x77777800, np.int32), np.full((N, n_lwe), 0x77777700, np.int32)])
        want = PO.pack_rows(words, two, np.concatenate([b, b]))
        assert np.array_equal(got[0::2], np.broadcast_to(want[0], got[0::2].shape))
        assert np.array_equal(got[1::2], np.broadcast_to(want[1], got[1::2].shape))
    finally:
        pkey.close()


def test_more_outputs_than_one_batch(ctx):
    """T = 513 runs as a batch of 512 outputs and a batch of one on the same scratch, in stream order;
    P = 1 keeps the inputs and the oracle small"""
    words, pkey = _random_key(ctx)
    rng = np.random.default_rng(513)
    in_a, in_b = _rand32(rng, (513, 1, n_lwe)), _rand32(rng, (513, 1))
    pos = np.array([1023], np.int32)
    got = ctx.pack_host(pkey, in_a, in_b, pos)
    kern = ctx.last_kernels()   # the batch of one is split; the batch of 512 is unsplit on fewer than 512 CUs
    assert kern[0] == "k_pack_digits" and kern[-1] == "k_pack_v4(split)" and len(kern) == (3 if _cus() < 512 else 2), kern
    assert np.array_equal(got, PO.pack_inputs(words, in_a, in_b, pos))


def test_device_index_rules(ctx):
    """device form: a pos entry of -1, 1024 or 2^30 drops that input and the rest are exact; the host
    form refuses those and duplicates and writes no output"""
    words, pkey = _random_key(ctx)
    rng = np.random.default_rng(31)
    P = 7
    in_a, in_b = _rand32(rng, (2, P, n_lwe)), _rand32(rng, (2, P))
    pos = np.array([5, -1, 1023, 1024, 0, 1 << 30, 600], np.int32)
    out = _zeros((2, 2, N))
    ctx.pack_dev(pkey, _dev(in_a), _dev(in_b), out, _dev(pos))
    ctx.sync()
    keep = [0, 2, 4, 6]
    want = PO.pack_rows(words, in_a[:, keep], in_b[:, keep], pos[keep])
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(want, PO.pack_rows(words, in_a, in_b, pos))
    for bad in (pos, np.array([5, 6, 7, 8, 9, 10, 5], np.int32)):
        o = np.full((2, 2, N), 77, np.int32)
        assert T.lib.tfhe_amd_pack_host(ctx.h, pkey.h, 2, P, T._p(in_a), T._p(in_b), T._p(bad), T._p(o)) == E_ARG
        assert (o == 77).all()
    # duplicates on the device: unspecified output, no fault, and the next call is right again
    ctx.pack_dev(pkey, _dev(in_a), _dev(in_b), out, _dev(np.array([5, 6, 7, 8, 9, 10, 5], np.int32)))
    ctx.sync()
    assert np.array_equal(ctx.pack_host(pkey, in_a[:, keep], in_b[:, keep], pos[keep]), want)


def test_argument_refusals(ctx):
    _, pkey = _random_key(ctx)
    lib, p = T.lib, T._p
    a, b, o = np.zeros((1, 1, n_lwe), np.int32), np.zeros((1, 1), np.int32), np.full((1, 2, N), 77, np.int32)
    call = lambda T_=1, P=1, pa=p(a), pb=p(b), po=p(o), c=ctx.h, k=pkey.h: lib.tfhe_amd_pack_host(c, k, T_, P, pa, pb, None, po)
    assert call(T_=-1) == E_ARG and call(P=0) == E_ARG and call(P=N + 1) == E_ARG
    assert call(pa=None) == E_ARG and call(pb=None) == E_ARG and call(po=None) == E_ARG
    assert call(c=None) == E_ARG and call(k=None) == E_ARG
    assert (o == 77).all()
    assert call(T_=0) == 0 and call(T_=0, P=0, pa=None, pb=None, po=None) == 0
    d = _zeros((1, 2, N))
    dev = lambda T_=1, P=1, pa=d.data_ptr(), po=d.data_ptr(): lib.tfhe_amd_pack_dev(ctx.h, pkey.h, T_, P, pa, pa, None, po, None)
    assert dev(T_=-1) == E_ARG and dev(P=0) == E_ARG and dev(P=N + 1) == E_ARG and dev(pa=None) == E_ARG
    assert dev(po=None) == E_ARG and dev(T_=0) == 0
    assert lib.tfhe_amd_pack_key_import(ctx.h, None, ctypes.byref(ctypes.c_void_p())) == E_ARG
    assert lib.tfhe_amd_pack_key_import(ctx.h, p(np.zeros(1, np.int32)), None) == E_ARG


def test_real_gates_pack_decrypt_and_noise(ctx, keyset):
    """1 024 NAND outputs of gate_host packed into one ciphertext: exact against the oracle, every
    coefficient of the client's phase has the sign of the truth table, and (packed phase - input
    phase under the LWE key) has the predicted size: r.m.s. within [0.5, 1.5] sigma_pack(1024),
    largest value below 8 sigma_pack(1024), sigma_pack(P) = sqrt(500 * 6 * 21.5 * P) * 7.18e-9.
    Measured on an MI355X: see DESIGN.md §3.7."""
    words, pkey, truth, g_a, g_b = _real_key(ctx, keyset)
    packed = ctx.pack_host(pkey, g_a, g_b)
    assert ctx.last_kernels() == SPLIT
    assert np.array_equal(packed, PO.pack_rows(words, g_a[None], g_b[None]))
    ph = keyset.tlwe_phase(packed)[0]
    assert np.array_equal((ph > 0).astype(np.int64), truth)
    diff = (ph.astype(np.int64) - keyset.phase(g_a, g_b).astype(np.int64) + 2**31) % 2**32 - 2**31
    sigma = PO.sigma_pack(N)
    rms, peak = np.sqrt(np.mean(diff.astype(np.float64) ** 2)) / 2**32, np.abs(diff).max() / 2**32
    print(f"pack noise at P = 1024: rms {rms:.3e}, max {peak:.3e}, predicted sigma {sigma:.3e}")
    assert 0.5 * sigma <= rms <= 1.5 * sigma, (rms, sigma)
    assert peak < 8 * sigma, (peak, sigma)


def test_packed_ciphertext_feeds_the_lookup(ctx, keyset):
    """the packed gate results as an encrypted table (tab_rows = 2) of tgsw_lookup_host under 10
    client-encrypted address bits: every output decrypts to the gate result at its address and
    equals the oracle's lookup on the packed words"""
    words, pkey, truth, g_a, g_b = _real_key(ctx, keyset)
    packed = ctx.pack_host(pkey, g_a, g_b)
    T.lib.tfhe_random_generator_setSeed((ctypes.c_uint32 * 2)(2025, 8), 2)
    bits = np.array([0, 1, 1, 0], np.int32)
    g = keyset.tgsw_encrypt(bits)
    tset = ctx.tgsw_import(g)
    try:
        rng = np.random.default_rng(10)
        addr = np.concatenate([[0, N - 1], rng.integers(0, N, 6)])
        sel = TO.pick(rng, bits, (addr[:, None] >> np.arange(10)) & 1)
        tab = packed.reshape(1, 1, 2, N)
        r_a, r_b = ctx.tgsw_lookup_host(tset, sel, tab)
        assert np.array_equal(keyset.decrypt(r_a[0], r_b[0]), truth[addr])
        want = TO.lookup(TO.key(g, keyset.ksk), sel, tab)
        assert np.array_equal(r_a, want[0]) and np.array_equal(r_b, want[1])
    finally:
        tset.close()


def test_many_lut_block_packs_in_place(ctx, keyset):
    """a (log_nu, n_out) = (1, 2) many-LUT result at B = 16 is already [T = 2][P = 16][500]"""
    words, pkey = _real_key(ctx, keyset)[:2]
    rng = np.random.default_rng(16)
    p, B = 4, 16
    f = rng.integers(0, p, (2, p))
    tv = T.lut_table_many(p, T.lut_encode(f, p), 1)
    msgs = rng.integers(0, p, B)
    x_a, x_b = keyset.encrypt_digits(msgs, p, rng)
    r_a, r_b = ctx.lut_many_bootstrap_host(tv, 1, 2, x_a, x_b)
    assert r_a.shape == (2, B, n_lwe) and r_a.flags["C_CONTIGUOUS"]
    packed = ctx.pack_host(pkey, r_a, r_b)
    assert np.array_equal(packed, PO.pack_rows(words, r_a, r_b))
    ph = keyset.tlwe_phase(packed)
    for k in range(2):
        assert np.array_equal(T.lut_decode(ph[k, :B], p), f[k][msgs]), k
        diff = (ph[k, :B].astype(np.int64) - keyset.phase(r_a[k], r_b[k]).astype(np.int64) + 2**31) % 2**32 - 2**31
        assert np.abs(diff).max() / 2**32 < 8 * PO.sigma_pack(B)
        assert np.abs(ph[k, B:].astype(np.int64)).max() / 2**32 < 8 * PO.sigma_pack(B)   # unoccupied: 0 plus noise


def test_host_and_device_forms_agree(ctx):
    words, pkey = _random_key(ctx)
    rng = np.random.default_rng(4243)
    in_a, in_b = _rand32(rng, (4, 9, n_lwe)), _rand32(rng, (4, 9))
    pos = rng.permutation(N)[:9].astype(np.int32)
    for ps in (None, pos):
        host = ctx.pack_host(pkey, in_a, in_b, ps)
        out = _zeros((4, 2, N))
        out += 5                                           # the call overwrites, it does not add
        import torch
        torch.cuda.synchronize()
        ctx.pack_dev(pkey, _dev(in_a), _dev(in_b), out, None if ps is None else _dev(ps))
        kern = ctx.last_kernels()
        ctx.sync()
        assert kern == SPLIT
        assert np.array_equal(out.cpu().numpy(), host)
    assert np.array_equal(host, PO.pack_inputs(words, in_a, in_b, pos))


def test_import_destroy_import_again(ctx):
    words, pkey = _random_key(ctx)
    rng = np.random.default_rng(98)
    in_a, in_b = _rand32(rng, (1, 3, n_lwe)), _rand32(rng, (1, 3))
    first = ctx.pack_host(pkey, in_a, in_b)
    for _ in range(2):
        again = ctx.pack_key_import(words)
        got = ctx.pack_host(again, in_a, in_b)
        again.close()
        assert again.h is None
        assert np.array_equal(got, first)
    assert np.array_equal(first, PO.pack_inputs(words, in_a, in_b))


def test_key_outlives_its_context(keyset):
    rng = np.random.default_rng(6)
    words = _rand32(rng, (n_lwe, 6, 2, N))
    a = T.Context(keyset.bk, keyset.ksk, device=0)
    pkey = a.pack_key_import(words)
    a.close()
    b = T.Context(keyset.bk, keyset.ksk, device=0)
    try:
        in_a, in_b = _rand32(rng, (1, 2, n_lwe)), _rand32(rng, (1, 2))
        assert np.array_equal(b.pack_host(pkey, in_a, in_b), PO.pack_inputs(words, in_a, in_b))
    finally:
        pkey.close()
        b.close()


def test_key_on_the_wrong_device_is_refused(ctx, keyset):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _, pkey = _random_key(ctx)
    other = T.Context(keyset.bk, keyset.ksk, device=1)
    try:
        with pytest.raises(T.TfheAmdError, match="-1"):
            other.pack_host(pkey, np.zeros((1, 1, n_lwe), np.int32), np.zeros((1, 1), np.int32))
    finally:
        other.close()


def test_two_streams_with_scratch_regrowth(ctx):
    """T = 1 on one stream, then T = 4 on another with no host sync in between: the second call
    regrows the key's scratch and is ordered behind the first"""
    import torch
    words = _rand32(np.random.default_rng(12), (n_lwe, 6, 2, N))
    pkey = ctx.pack_key_import(words)
    rng = np.random.default_rng(13)
    try:
        jobs = []
        for T_ in (1, 4):
            in_a, in_b = _rand32(rng, (T_, 6, n_lwe)), _rand32(rng, (T_, 6))
            jobs.append((in_a, in_b, _dev(in_a), _dev(in_b), _zeros((T_, 2, N)), torch.cuda.Stream()))
        torch.cuda.synchronize()
        for _, _, d_a, d_b, out, st in jobs:
            ctx.pack_dev(pkey, d_a, d_b, out, stream=st.cuda_stream)
        torch.cuda.synchronize()
        for in_a, in_b, _, _, out, _ in jobs:
            assert np.array_equal(out.cpu().numpy(), PO.pack_inputs(words, in_a, in_b))
    finally:
        pkey.close()
