"""One-rotation adder cells on the GPU (tfhe_amd_full_add_batch_*, the circuit builders on them,
DESIGN.md §3.4): every output word against the oracle composition of tests/fa_oracle.py — the
three-input prologue of the batch kernels in every launch form of both kernel generations, the
guard's exact recompute, and the circuits word for word and decoded."""
import numpy as np
import pytest

import dev_arena as DA
import fa_oracle as FO
import many_lut_oracle as MO
import tfhe_amd as T

pytestmark = pytest.mark.gpu

N, n_lwe = 1024, 500
ENCS = [(s, c) for s in (T.ENC_GATE, T.ENC_HALF) for c in (T.ENC_GATE, T.ENC_HALF)]


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same(got, want):
    return (got[0].shape == want[0].shape and got[1].shape == want[1].shape and
            np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


def _dev(x):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in x)


_cache = {}


def _bits8(keyset):
    """B = 8 fresh half-torus bits a, b, c covering all eight combinations"""
    if "bits8" not in _cache:
        rng = np.random.default_rng(8101)
        k = np.arange(8)
        m = (k & 1, (k >> 1) & 1, k >> 2)
        _cache["bits8"] = (m, tuple(keyset.encrypt_digits(v, 4, rng) for v in m))
    return _cache["bits8"]


def _random8(okey):
    """B = 8 uniformly random words in all three inputs and the oracle's results for the (H, G)
    table: shared by the guard and the exact-mode tests"""
    if "random8" not in _cache:
        rng = np.random.default_rng(8202)
        x = tuple((_rand32(rng, (8, n_lwe)), _rand32(rng, 8)) for _ in range(3))
        _cache["random8"] = (x, FO.cell(okey, FO.H, FO.G, *x))
    return _cache["random8"]


# ---------------------------------------------------------------- the batch form

@pytest.mark.parametrize("enc_sum,enc_carry", ENCS)
def test_batch_decoded(ctx, okey, keyset, enc_sum, enc_carry):
    """all eight (a, b, c) and the half adder, host and device arrays: word-exact and decoded"""
    import torch
    (ma, mb, mc), (a, b, c) = _bits8(keyset)
    for third, m in ((c, ma + mb + mc), (None, ma + mb)):
        want = FO.cell(okey, enc_sum, enc_carry, a, b, third)
        got = ctx.full_add_host(enc_sum, enc_carry, a, b, third)
        kern = ctx.last_kernels()
        assert _same(got, want)
        assert "k_blind_rotate_v6(lut-many+lds-rotation)" in kern and "k_blind_rotate_v4(lut-many+guard)" in kern, kern
        s, co = FO.cell_truth(m)
        assert np.array_equal(FO.decode(keyset, enc_sum, (got[0][0], got[1][0])), s)
        assert np.array_equal(FO.decode(keyset, enc_carry, (got[0][1], got[1][1])), co)
        r_a = DA.poisoned((2, 8, n_lwe))
        r_b = DA.poisoned((2, 8))
        ctx.full_add_dev(enc_sum, enc_carry, r_a, r_b, _dev(a), _dev(b), None if third is None else _dev(third))
        ctx.sync()
        assert _same((r_a.cpu().numpy(), r_b.cpu().numpy()), want)


def test_batch_random_words_and_rotation_edges(ctx, okey):
    """uniformly random words in all three inputs (nothing decodes: bit-exactness at arbitrary
    phases); the third input's body is chosen so that the summed body lands on every edge of the
    negacyclic rotation and on the rounding boundaries of the coarse switch; host, device, and the
    device result written over an input"""
    import torch
    rng = np.random.default_rng(8303)
    theta, nu = 1, 2
    edges = [0, nu, N - nu, N, N + nu, 2 * N - nu]
    half = (nu * 5 + nu // 2) << 21
    words = [k << 21 for k in edges] + [half - 1, half, 2**32 - (1 << (20 + theta))]
    B = 12
    a, b = (_rand32(rng, (B, n_lwe)), _rand32(rng, B)), (_rand32(rng, (B, n_lwe)), _rand32(rng, B))
    c_b = _rand32(rng, B)
    tgt = np.array(words, dtype=np.int64)
    c_b[:9] = FO.wrap(tgt + 2 * FO.E16 - a[1][:9].astype(np.int64) - b[1][:9].astype(np.int64))
    c = (_rand32(rng, (B, n_lwe)), c_b)
    x = FO.cell_input(a, b, c)
    assert [int(v) for v in MO.bar(x[1][:9], theta)] == edges + [nu * 5, nu * 6, 0]
    for enc_sum, enc_carry in ((FO.H, FO.H), (FO.G, FO.H)):
        want = FO.cell(okey, enc_sum, enc_carry, a, b, c)
        assert _same(ctx.full_add_host(enc_sum, enc_carry, a, b, c), want)
        for alias in (0, 1, 2):   # the result's first block is the storage of a, b or c
            ins = [_dev(a), _dev(b), _dev(c)]
            r_a = DA.poisoned((2, B, n_lwe))
            r_b = DA.poisoned((2, B))
            r_a[0].copy_(ins[alias][0])
            r_b[0].copy_(ins[alias][1])
            ins[alias] = (r_a[0], r_b[0])
            ctx.full_add_dev(enc_sum, enc_carry, r_a, r_b, *ins)
            ctx.sync()
            assert _same((r_a.cpu().numpy(), r_b.cpu().numpy()), want), alias
    # the half adder on the same words
    assert _same(ctx.full_add_host(FO.H, FO.H, a, b), FO.cell(okey, FO.H, FO.H, a, b))


def test_batch_every_launch_form(ctx, okey):
    """B = CUs + 1: the paired kernel (pair sync) with its padding ciphertext; B = 2 CUs + 1: the
    register rotation (the small batches ran the LDS rotation); three inputs, all outputs"""
    cus = _cus()
    rng = np.random.default_rng(8404)
    for B, variant in ((cus + 1, "k_blind_rotate_v6p(lut-many+paired+reg-rotation+pair-sync)"),
                       (2 * cus + 1, "k_blind_rotate_v6(lut-many+reg-rotation)")):
        a, b, c = ((_rand32(rng, (B, n_lwe)), _rand32(rng, B)) for _ in range(3))
        got = ctx.full_add_host(FO.H, FO.G, a, b, c)
        kern = ctx.last_kernels()
        assert _same(got, FO.cell(okey, FO.H, FO.G, a, b, c)), B   # parity first, then which kernel
        assert variant in kern and "k_blind_rotate_v4(lut-many+guard)" in kern, (B, kern)


def test_batch_exact_kernel(ctx, okey):
    (a, b, c), want = _random8(okey)
    try:
        T.select_kernel(4)
        got = ctx.full_add_host(FO.H, FO.G, a, b, c)
        kern = ctx.last_kernels()
    finally:
        T.select_kernel(0)
    assert _same(got, want)
    assert "k_blind_rotate_v4(lut-many)" in kern and not any("v6" in k for k in kern), kern


def test_batch_guard_recomputes_with_all_three_inputs(ctx, okey):
    """threshold 0: every ciphertext is flagged and recomputed by the exact kernel from the same
    three inputs, both outputs rewritten; the counter counts ciphertexts"""
    (a, b, c), want = _random8(okey)
    default = ctx.full_add_host(FO.H, FO.G, a, b, c)
    try:
        T.set_guard_threshold(0.0)
        ctx.guard_stats(reset=True)
        got = ctx.full_add_host(FO.H, FO.G, a, b, c)
        kern = ctx.last_kernels()
        _, recomputed = ctx.guard_stats(reset=True)
    finally:
        T.set_guard_threshold(0.125)
    assert recomputed == 8
    assert _same(got, default) and _same(got, want)
    assert "k_blind_rotate_v4(lut-many+guard)" in kern, kern


def test_batch_argument_errors(ctx):
    import torch
    lib, p = T.lib, T._p
    B = 4
    z, zb = np.zeros((B, n_lwe), np.int32), np.zeros(B, np.int32)
    r_a, r_b = np.zeros((2, B, n_lwe), np.int32), np.zeros((2, B), np.int32)

    def host(Bv=B, es=1, ec=1, a=(z, zb), b=(z, zb), c=(None, None), r=(r_a, r_b)):
        return lib.tfhe_amd_full_add_batch_host(ctx.h, Bv, es, ec, p(a[0]), p(a[1]), p(b[0]), p(b[1]), p(c[0]), p(c[1]),
                                                p(r[0]), p(r[1]))
    for es, ec in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert host(es=es, ec=ec) == -1
    assert host(Bv=-1) == -1 and host(a=(None, zb)) == -1 and host(b=(z, None)) == -1 and host(r=(None, r_b)) == -1
    assert host(c=(z, None)) == -1 and host(c=(None, zb)) == -1
    assert host(Bv=0) == 0 and host() == 0 and host(c=(z, zb)) == 0
    d = torch.zeros((B, n_lwe), dtype=torch.int32, device="cuda")
    db = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_r = torch.zeros((2, B, n_lwe), dtype=torch.int32, device="cuda")
    d_rb = torch.zeros((2, B), dtype=torch.int32, device="cuda")

    def dev(Bv=B, es=1, ec=1, a=d.data_ptr(), c_a=None, c_b=None, r=d_r.data_ptr()):
        return lib.tfhe_amd_full_add_batch_dev(ctx.h, Bv, es, ec, a, db.data_ptr(), d.data_ptr(), db.data_ptr(), c_a, c_b,
                                               r, d_rb.data_ptr(), None)
    for es, ec in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert dev(es=es, ec=ec) == -1
    assert dev(Bv=-1) == -1 and dev(a=None) == -1 and dev(r=None) == -1
    assert dev(c_a=d.data_ptr()) == -1 and dev(c_b=db.data_ptr()) == -1
    assert dev() == 0 and dev(c_a=d.data_ptr(), c_b=db.data_ptr()) == 0
    ctx.sync()
    with pytest.raises(T.TfheAmdError):   # a result of the wrong shape never reaches the GPU
        ctx.full_add_dev(1, 1, d_r[0], d_rb, (d, db), (d, db))


# ---------------------------------------------------------------- circuits

def _run(ctx, C, enc, B):
    import torch
    n_w = C.info()["wires"]
    wa = DA.poisoned((n_w, B, n_lwe))      # every wire the run does not write stays poison
    wb = DA.poisoned((n_w, B))
    for w, (a, b) in enc.items():
        wa[w] = torch.from_numpy(a).cuda()
        wb[w] = torch.from_numpy(b).cuda()
    C.run_dev(ctx, B, wa, wb)
    ctx.sync()
    return wa.cpu().numpy(), wb.cpu().numpy(), ctx.last_kernels()


def _check_wires(W, ha, hb):
    assert len(W) == ha.shape[0]
    for w, (a, b) in W.items():
        assert np.array_equal(ha[w], a) and np.array_equal(hb[w], b), w


def test_circuit_mul_fa(ctx, okey, keyset):
    """mul_fa 4 x 4: B = 5 (LDS rotation) and B = CUs / 2 + 2 (register rotation in the wide levels);
    every wire against the oracle's node-by-node evaluation, the products decoded"""
    for B, variant in ((5, "k_blind_rotate_v6_rows(lut-many+lds-rotation)"),
                       (_cus() // 2 + 2, "k_blind_rotate_v6_rows(lut-many+reg-rotation)")):
        C, a, b, prod, x, y, enc, W = FO.mul_case(keyset, okey, 4, B)
        ha, hb, kern = _run(ctx, C, enc, B)
        _check_wires(W, ha, hb)
        assert np.array_equal(T.int_of([keyset.decrypt(ha[w], hb[w]) for w in prod]), x * y)
        assert variant in kern and "k_blind_rotate_v4_rows(lut-many+guard)" in kern, (B, kern)


def test_circuit_dot_fa_and_add_half(ctx, okey, keyset):
    B = 5
    C, a, b, out, x, y, enc, W = FO.dot_case(keyset, okey, B)
    ha, hb, kern = _run(ctx, C, enc, B)
    _check_wires(W, ha, hb)
    assert np.array_equal(T.int_of([keyset.decrypt(ha[w], hb[w]) for w in out]), (x * y).sum(axis=1) % 256)
    C, info, x, y, enc, W = FO.add_half_case(keyset, okey, B)
    ha, hb, kern = _run(ctx, C, enc, B)
    _check_wires(W, ha, hb)
    bits = lambda ws, e: [FO.decode(keyset, e, (ha[w], hb[w])) for w in ws]
    assert np.array_equal(T.int_of(bits(info["sum_g"] + [info["carry_g"]], FO.G)), x + y)
    assert np.array_equal(T.int_of(bits(info["sum_h"] + [info["carry_h"]], FO.H)), x + y)
    assert np.array_equal(T.int_of(bits(info["sum2"] + [info["carry2"]], FO.G)), (x + y) % 16 + x + ((x + y) >> 4))


def test_circuit_exact_kernel(ctx, okey, keyset):
    C, a, b, prod, x, y, enc, W = FO.mul_case(keyset, okey, 4, 5)
    try:
        T.select_kernel(4)
        ha, hb, kern = _run(ctx, C, enc, 5)
    finally:
        T.select_kernel(0)
    _check_wires(W, ha, hb)
    assert "k_blind_rotate_v4_rows(lut-many)" in kern and not any("v6" in k for k in kern), kern


def test_multi_circuit(okey, keyset):
    """tfhe_amd_multi_circuit_run_host with mul_fa 3 x 3 on two slots of one GPU"""
    B = 5
    C, a, b, prod, x, y, enc, W = FO.mul_case(keyset, okey, 3, B)
    ins = a + b
    wires = [w for w in range(C.info()["wires"]) if w not in ins]
    m = T.MultiContext(keyset.bk, keyset.ksk, [0, 0])
    try:
        in_a = np.stack([enc[w][0] for w in ins])
        in_b = np.stack([enc[w][1] for w in ins])
        out_a, out_b = m.circuit_host(C, B, ins, in_a, in_b, wires)
    finally:
        m.close()
    for j, w in enumerate(wires):
        assert np.array_equal(out_a[j], W[w][0]) and np.array_equal(out_b[j], W[w][1]), w
    got = {w: (out_a[j], out_b[j]) for j, w in enumerate(wires)}
    assert np.array_equal(T.int_of([keyset.decrypt(*got[w]) for w in prod]), x * y)
