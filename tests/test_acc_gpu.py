"""Bootstrap from encrypted accumulators on the GPU (tfhe_amd_tlwe_box_fill_*, tfhe_amd_bootstrap_acc_*,
tfhe_amd_select_*): every output word against the oracle of tests/acc_oracle.py, word
for word with no tolerance.  Bit-exactness does not need valid ciphertexts, so most accumulators,
candidates and pack keys are uniformly random words; the decode cases run real ciphertexts through a
generated packing key."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dev_arena as DA
import acc_oracle as AO
import guard_cases as G
import lut_oracle as LO
import oracle_ctypes as O
import tfhe_amd as T

pytestmark = pytest.mark.gpu

N, n_lwe = 1024, 500
E_ARG = -1
GUARD = "k_blind_rotate_v4(tlwe+guard)"
LDS, REG = "k_blind_rotate_v6(tlwe+lds-rotation)", "k_blind_rotate_v6(tlwe+reg-rotation)"
PAIRED = "k_blind_rotate_v6p(tlwe+paired+reg-rotation+pair-sync)"
KS_LARGE = {"k_keyswitch_v4", "k_keyswitch_v5(int8-mfma)", "k_keyswitch_v5(int8-mfma+split2)",
            "k_keyswitch_v5(int8-mfma+split4)", "k_keyswitch_v5(int8-mfma+split8)"}
SELECT_HEAD = ["k_pack_digits(function-major)", "k_pack_v4(split)", "k_tlwe_box_fill", LDS, GUARD]


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
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


_cache = {}


def _case(keyset):
    """5 random-word accumulators and two batches of 5 fresh selector samples, once per session"""
    if "case" not in _cache:
        rng = np.random.default_rng(3801)
        acc = _rand32(rng, (5, 2, N))
        x = keyset.encrypt_digits(rng.integers(0, 4, 5), 4, rng)
        y = keyset.encrypt_digits(rng.integers(0, 4, 5), 4, rng)
        _cache["case"] = (acc, x, y)
    return _cache["case"]


# ------------------------------------------------------------------ box fill

@pytest.mark.parametrize("T_", [1, 3])
def test_box_fill(ctx, T_):
    """log_w in {0, 1, 8, 10}: the host form, the device form out of place and in place, against the
    oracle's plain sums; one sample holds a single value at coefficient N - 1 (the wrap sign)"""
    rng = np.random.default_rng(70 + T_)
    x = _rand32(rng, (T_, 2, N))
    x[-1, 1] = 0
    x[-1, 1, N - 1] = 0x12345678
    for log_w in (0, 1, 8, 10):
        want = AO.box_fill(x, log_w)
        assert np.array_equal(ctx.box_fill_host(x, log_w), want), log_w
        assert ctx.last_kernels() == ["k_tlwe_box_fill"]
        d_in, d_out = _dev(x), _zeros((T_, 2, N))
        ctx.box_fill_dev(d_in, d_out, log_w)
        ctx.box_fill_dev(d_in, d_in, log_w)
        ctx.sync()
        assert np.array_equal(d_out.cpu().numpy(), want), log_w
        assert np.array_equal(d_in.cpu().numpy(), want), log_w
    lib, z = T.lib, np.full((1, 2, N), 77, np.int32)
    for bad in (-1, 11):
        assert lib.tfhe_amd_tlwe_box_fill_host(ctx.h, 1, bad, T._p(x), T._p(z)) == E_ARG
    assert lib.tfhe_amd_tlwe_box_fill_host(ctx.h, -1, 0, T._p(x), T._p(z)) == E_ARG
    assert lib.tfhe_amd_tlwe_box_fill_host(ctx.h, 1, 0, None, T._p(z)) == E_ARG
    assert lib.tfhe_amd_tlwe_box_fill_host(ctx.h, 0, 0, None, None) == 0
    assert (z == 77).all()


# ------------------------------------------------------------------ accumulator bootstrap

@pytest.mark.parametrize("B", [1, 5])
def test_acc_bootstrap_small_batches(ctx, okey, keyset, B):
    """woks and key-switched forms through the default fp64 kernel: one shared accumulator, one per
    ciphertext, an explicit permuted index with repeats, and a two-term selector; host forms, and the
    device form for the indexed case"""
    acc, x, y = _case(keyset)
    x = (x[0][:B], x[1][:B])
    y = (y[0][:B], y[1][:B])
    small = [LDS, GUARD]
    # n_acc = 1, shared
    got = ctx.acc_woks_host(acc[2], *x)
    assert ctx.last_kernels() == small, ctx.last_kernels()
    want_u = AO.woks_batch(okey, acc[2], *x)
    assert _same(got, want_u)
    got = ctx.acc_bootstrap_host(acc[2], *x)
    assert ctx.last_kernels() == small + ["k_keyswitch_small"], ctx.last_kernels()
    assert _same(got, okey.keyswitch_batch(*want_u, nthreads=AO.THREADS))
    # n_acc = B, identity
    assert _same(ctx.acc_woks_host(acc[:B], *x), AO.woks_batch(okey, acc[:B], *x))
    # explicit index with repeats, two-term selector (0, c) + sa X + sb Y
    idx = np.array([4, 0, 4, 2, 0][:B], np.int32)
    c, sa, sb = 1 << 27, 1, -1
    s_a, s_b = LO.lin(c, [(sa, x), (sb, y)], B)
    want_u = AO.woks_batch(okey, acc, s_a, s_b, idx)
    got = ctx.acc_woks_host(acc, *x, acc_index=idx, c=c, sa=sa, sb=sb, y_a=y[0], y_b=y[1])
    assert _same(got, want_u)
    d_acc, d_idx = _dev(acc), _dev(idx)
    u_a, u_b = _zeros((B, N)), _zeros((B,))
    ctx.acc_woks_dev(d_acc, u_a, u_b, _dev(x[0]), _dev(x[1]), d_idx, c, sa, sb, _dev(y[0]), _dev(y[1]))
    assert ctx.last_kernels() == small
    r_a, r_b = _zeros((B, n_lwe)), _zeros((B,))
    ctx.acc_bootstrap_dev(d_acc, r_a, r_b, _dev(x[0]), _dev(x[1]), d_idx, c, sa, sb, _dev(y[0]), _dev(y[1]))
    ctx.sync()
    assert _same((u_a.cpu().numpy(), u_b.cpu().numpy()), want_u)
    assert _same((r_a.cpu().numpy(), r_b.cpu().numpy()), okey.keyswitch_batch(*want_u, nthreads=AO.THREADS))


def _woks_dev(ctx, acc, idx, x):
    B = x[1].shape[0]
    u_a, u_b = _zeros((B, N)), _zeros((B,))
    ctx.acc_woks_dev(_dev(acc), u_a, u_b, _dev(x[0]), _dev(x[1]), _dev(idx))
    kern = ctx.last_kernels()
    ctx.sync()
    return (u_a.cpu().numpy(), u_b.cpu().numpy()), kern


@pytest.mark.parametrize("form", ["paired", "reg"])
def test_acc_bootstrap_larger_launch_forms(ctx, okey, keyset, form):
    """B = CUs + 1 (the paired kernel with its padding ciphertext) and B = 2 CUs + 1 (register
    rotation): all rows equal the exact kernel's (tfhe_amd_select_kernel(4)); the first row, the last
    row and 6 seeded rows equal the oracle"""
    B = _cus() + 1 if form == "paired" else 2 * _cus() + 1
    rng = np.random.default_rng(3802 + B)
    acc = _rand32(rng, (3, 2, N))
    idx = rng.integers(0, 3, B).astype(np.int32)
    x = keyset.encrypt_digits(rng.integers(0, 4, B), 4, rng)
    got, kern = _woks_dev(ctx, acc, idx, x)
    assert kern == [PAIRED if form == "paired" else REG, GUARD], kern
    try:
        T.select_kernel(4)
        exact, kern4 = _woks_dev(ctx, acc, idx, x)
    finally:
        T.select_kernel(0)
    assert kern4 == ["k_blind_rotate_v4(tlwe)"], kern4
    assert _same(got, exact)
    rows = np.unique(np.concatenate([[0, B - 1], rng.choice(B, 6, replace=False)]))
    want = AO.woks_batch(okey, acc, x[0][rows], x[1][rows], idx[rows])
    assert _same((got[0][rows], got[1][rows]), want)


def test_exact_kernel_against_the_oracle(ctx, okey, keyset):
    acc, x, _ = _case(keyset)
    idx = np.array([1, 3, 3, 0, 2], np.int32)
    try:
        T.select_kernel(4)
        got = ctx.acc_bootstrap_host(acc, *x, acc_index=idx)
        kern = ctx.last_kernels()
    finally:
        T.select_kernel(0)
    assert kern == ["k_blind_rotate_v4(tlwe)", "k_keyswitch_small"], kern
    assert _same(got, AO.bootstrap_batch(okey, acc, *x, idx))


def test_guard_threshold_zero_recomputes_everything(ctx, okey, keyset):
    """with the threshold at 0 every ciphertext is recomputed by the exact kernel from the same
    accumulator: same words, recomputed == B"""
    acc, x, _ = _case(keyset)
    B = 5
    want = AO.woks_batch(okey, acc, *x)
    try:
        assert T.lib.tfhe_amd_set_guard_threshold(0.0) == 0
        ctx.guard_stats(reset=True)
        got = ctx.acc_woks_host(acc, *x)
        kern = ctx.last_kernels()
        _, redo = ctx.guard_stats(reset=True)
    finally:
        T.lib.tfhe_amd_set_guard_threshold(0.125)
        T.select_kernel(0)
    assert GUARD in kern, kern
    assert redo == B, redo
    assert _same(got, want)


# ---- partly flagged batch: the hostile key of tests/guard_cases.py, candidates qualified the way
# tests/test_guard_partial_gpu.py does (its few lines restated for two-row accumulators)

def _start(acc, b):
    """X^{2N - barb} (acc_a, acc_b) for each candidate body b: [n][2][N]"""
    barb = LO.modswitch_2n(b)
    return np.stack([np.stack([O.mul_by_xai((2 * N - int(e)) % (2 * N), np.ascontiguousarray(acc[c])) for c in range(2)])
                     for e in barb])


def _oracle_acc(okey, start, bara):
    acc = np.array(start, dtype=np.int32, copy=True)
    bara = np.ascontiguousarray(bara)

    def one(k):   # ctypes releases the GIL
        O.lib().orc_blind_rotate(O._p(acc[k].reshape(2 * N)), ctypes.c_void_p(okey.h), O._p(bara[k]), n_lwe)
    with ThreadPoolExecutor(8) as tp:
        list(tp.map(one, range(bara.shape[0])))
    return acc


def _raw_acc(ctx, start, bara):
    """the raw fp64 CMux steps with no exactness guard (tfhe_amd_blind_rotate_dev)"""
    import torch
    d_acc = torch.from_numpy(np.array(start, dtype=np.int32, copy=True)).cuda()
    ctx.blind_rotate_dev(d_acc, torch.from_numpy(np.ascontiguousarray(bara)).cuda(), n_lwe)
    ctx.sync()
    return d_acc.cpu().numpy()


def test_guard_partly_flagged_batch(keyset):
    """B = 5 on the head-250 key, one shared accumulator of two constant polynomials: a dirty selector at slot 2 that
    the unguarded fp64 steps get wrong from this accumulator, clean real-step selectors at 0 and 4,
    fillers elsewhere.  Outputs equal the oracle and 0 < recomputed < B."""
    bk = G.head_key(keyset.bk)
    okey = O.OracleKey(bk, keyset.ksk, use_ntt=True)
    hctx = T.Context(bk, keyset.ksk, device=0)
    try:
        rng = np.random.default_rng(20251)
        # constant polynomials in both halves, as the gate's (mu, ..., mu): against the constant key
        # polynomials their digits add up coherently (a random-word accumulator's do not, and the
        # unguarded fp64 steps got 16 of 16 such candidates right on an MI355X)
        acc = np.empty((1, 2, N), np.int32)
        acc[0, 0], acc[0, 1] = -3 << 27, G.MU
        cand = G.dirty(rng, 16)
        start, bara = _start(acc[0], cand[1]), LO.modswitch_2n(cand[0])
        raw, exact = _raw_acc(hctx, start, bara), _oracle_acc(okey, start, bara)
        # extraction at 0 reads all of acc_a and acc_b[0]
        wrong = (raw[:, 0] != exact[:, 0]).any(axis=1) | (raw[:, 1, 0] != exact[:, 1, 0])
        print(f"qualified pool (tlwe accumulator): {int(wrong.sum())} of {wrong.size} candidates wrong unguarded")
        if 2 * int(wrong.sum()) < wrong.size:
            pytest.fail(f"{int(wrong.sum())} of {wrong.size} dirty candidates come out wrong unguarded: the pool is too thin")
        pool = (cand[0][wrong], cand[1][wrong])
        B, dirty_at, real_at = 5, [2], [0, 4]
        x = G.batch(np.random.default_rng(145), B, dirty_at, real_at, pool)
        hctx.guard_stats(reset=True)
        got = hctx.acc_woks_host(acc, *x)
        kern = hctx.last_kernels()
        dist, redo = hctx.guard_stats(reset=True)
        print(f"tlwe partly flagged: recomputed {redo} (dirty {len(dirty_at)}), distance {dist:.4f}, kernels {kern}")
        assert kern == [LDS, GUARD], kern
        assert _same(got, AO.woks_batch(okey, acc, *x))
        assert 0 < redo < B, redo
        assert dist >= 0.125
    finally:
        T.lib.tfhe_amd_set_guard_threshold(0.125)
        T.select_kernel(0)
        hctx.close()


def test_device_clamp_and_host_refusal(ctx, okey, keyset):
    """a device-side acc_index of -1 or n_acc reads accumulator 0 or n_acc - 1 and the call succeeds;
    the host form returns E_ARG and writes nothing; a null index needs n_acc in {1, B}"""
    acc, x, _ = _case(keyset)
    acc = acc[:3]
    idx = np.array([-1, 3, 1, 2**30, -2**31], np.int32)
    got, _ = _woks_dev(ctx, acc, idx, x)
    assert _same(got, AO.woks_batch(okey, acc, *x, np.clip(idx.astype(np.int64), 0, 2)))
    lib, p = T.lib, T._p
    u_a, u_b = np.full((5, N), 77, np.int32), np.full(5, 77, np.int32)
    for bad in (idx, np.array([0, 1, 2, 3, 0], np.int32)):
        assert lib.tfhe_amd_bootstrap_acc_woks_batch_host(ctx.h, 5, 3, p(acc), p(bad), 0, 1, p(x[0]), p(x[1]), 0, None,
                                                          None, p(u_a), p(u_b)) == E_ARG
    call = lambda B=5, n=3, a=p(acc), i=None, xa=p(x[0]), sb=0, ua=p(u_a): lib.tfhe_amd_bootstrap_acc_woks_batch_host(
        ctx.h, B, n, a, i, 0, 1, xa, p(x[1]), sb, None, None, ua, p(u_b))
    assert call() == E_ARG and call(n=0) == E_ARG and call(B=-1) == E_ARG and call(a=None, n=1) == E_ARG
    assert call(n=1, xa=None) == E_ARG and call(n=1, sb=1) == E_ARG and call(n=1, ua=None) == E_ARG
    assert call(B=0, n=1) == 0
    assert (u_a == 77).all() and (u_b == 77).all()


# ------------------------------------------------------------------ select

def _random_pack_key(ctx):
    if "rand" not in _cache:
        words = _rand32(np.random.default_rng(3803), (n_lwe, 6, 2, N))
        _cache["rand"] = (words, ctx.pack_key_import(words))
    return _cache["rand"]


def _real_pack_key(ctx, keyset):
    if "real" not in _cache:
        words = AO.chain_pack_key(keyset)
        _cache["real"] = (words, ctx.pack_key_import(words))
    return _cache["real"]


def _select_dev(ctx, pkey, cand_a, cand_b, y, c, sa, stream=None):
    B = y[1].shape[0]
    r_a, r_b = _zeros((B, n_lwe)), _zeros((B,))
    ctx.select_dev(pkey, _dev(cand_a), _dev(cand_b), _dev(y[0]), _dev(y[1]), r_a, r_b, c, sa, stream)
    return r_a, r_b


@pytest.mark.parametrize("p,B", [(2, 5), (4, 5), (4, 1)])
def test_select_random_words(ctx, okey, keyset, p, B):
    """random-word candidates and pack key, fresh selectors: all words equal the composed oracle, the
    host form equals the device form, and the trace lists the launches in order"""
    words, pkey = _random_pack_key(ctx)
    rng = np.random.default_rng(100 * p + B)
    cand_a, cand_b = _rand32(rng, (p, B, n_lwe)), _rand32(rng, (p, B))
    y = keyset.encrypt_digits(rng.integers(0, p, B), p, rng)
    c, sa = (1 << 30, 1) if p == 2 else (0, 1)
    want = AO.select(okey, words, cand_a, cand_b, c, sa, *y)
    host = ctx.select_host(pkey, cand_a, cand_b, *y, c=c, sa=sa)
    assert ctx.last_kernels() == SELECT_HEAD + ["k_keyswitch_small"], ctx.last_kernels()
    assert _same(host, want)
    r_a, r_b = _select_dev(ctx, pkey, cand_a, cand_b, y, c, sa)
    assert ctx.last_kernels() == SELECT_HEAD + ["k_keyswitch_small"], ctx.last_kernels()
    ctx.sync()
    assert _same((r_a.cpu().numpy(), r_b.cpu().numpy()), host)


def test_select_argument_refusals(ctx):
    _, pkey = _random_pack_key(ctx)
    lib, p = T.lib, T._p
    ca, cb = np.zeros((2, 1, n_lwe), np.int32), np.zeros((2, 1), np.int32)
    y_a, y_b = np.zeros((1, n_lwe), np.int32), np.zeros(1, np.int32)
    r_a, r_b = np.full((1, n_lwe), 77, np.int32), np.full(1, 77, np.int32)
    call = lambda B=1, P=2, k=pkey.h, a=p(ca), ya=p(y_a), ra=p(r_a): lib.tfhe_amd_select_batch_host(
        ctx.h, k, B, P, a, p(cb), 0, 1, ya, p(y_b), ra, p(r_b))
    assert call(P=1) == E_ARG and call(P=3) == E_ARG and call(P=2048) == E_ARG and call(P=0) == E_ARG
    assert call(B=-1) == E_ARG and call(k=None) == E_ARG and call(a=None) == E_ARG and call(ya=None) == E_ARG
    assert call(ra=None) == E_ARG and call(B=0) == 0
    assert (r_a == 77).all() and (r_b == 77).all()


def test_select_gate_bit_chooses_between_digits(ctx, okey, keyset):
    """p = 2 driven by a NAND output bit (+-1/8; c = 1/4, sa = 1): it chooses between two fresh p = 8
    digit ciphertexts and the result decodes to the chosen digit; words equal the composed oracle"""
    words, pkey = _real_pack_key(ctx, keyset)
    rng = np.random.default_rng(3805)
    B = 5
    u, v = rng.integers(0, 2, B), rng.integers(0, 2, B)
    bit = ctx.gate_host("NAND", *keyset.encrypt(u, rng), *keyset.encrypt(v, rng))
    d = rng.integers(0, 8, (2, B))
    cand = [keyset.encrypt_digits(d[m], 8, rng) for m in range(2)]
    cand_a, cand_b = np.stack([c[0] for c in cand]), np.stack([c[1] for c in cand])
    got = ctx.select_host(pkey, cand_a, cand_b, *bit, c=1 << 30, sa=1)
    assert _same(got, AO.select(okey, words, cand_a, cand_b, 1 << 30, 1, *bit))
    chosen = 1 - (u & v)
    assert np.array_equal(T.lut_decode(keyset.phase(*got), 8), d[chosen, np.arange(B)])


def test_select_reproduces_the_cpu_decode_chain(ctx, okey, keyset):
    """the case of tests/test_acc.py (B = 32, p = 4, bootstrapped candidates and selector): the GPU's
    words are the oracle's, so it decodes to f(x, y) as well"""
    c = AO.decode_chain(keyset, okey)
    _, pkey = _real_pack_key(ctx, keyset)
    got = ctx.select_host(pkey, c["cand_a"], c["cand_b"], c["sel_a"], c["sel_b"])
    assert _same(got, c["res"])
    assert np.array_equal(T.lut_decode(keyset.phase(*got), c["p"]), c["f"][c["x"], c["y"]])


def test_select_two_streams_with_scratch_regrowth(ctx, okey, keyset):
    """B = 1 on one stream, then B = 4 on another with no host sync in between: the second call
    regrows the key's digit and accumulator scratch and is ordered behind the first"""
    import torch
    words = _rand32(np.random.default_rng(3806), (n_lwe, 6, 2, N))
    pkey = ctx.pack_key_import(words)
    rng = np.random.default_rng(3807)
    try:
        jobs = []
        for B in (1, 4):
            cand_a, cand_b = _rand32(rng, (4, B, n_lwe)), _rand32(rng, (4, B))
            y = keyset.encrypt_digits(rng.integers(0, 4, B), 4, rng)
            jobs.append((cand_a, cand_b, y, torch.cuda.Stream()))
        dev = [(_dev(a), _dev(b), _dev(y[0]), _dev(y[1]), _zeros((y[1].shape[0], n_lwe)), _zeros(y[1].shape))
               for a, b, y, _ in jobs]
        torch.cuda.synchronize()
        for (d_a, d_b, d_ya, d_yb, r_a, r_b), job in zip(dev, jobs):
            ctx.select_dev(pkey, d_a, d_b, d_ya, d_yb, r_a, r_b, stream=job[3].cuda_stream)
        torch.cuda.synchronize()
        for (_, _, _, _, r_a, r_b), (cand_a, cand_b, y, _) in zip(dev, jobs):
            assert _same((r_a.cpu().numpy(), r_b.cpu().numpy()), AO.select(okey, words, cand_a, cand_b, 0, 1, *y))
    finally:
        pkey.close()
