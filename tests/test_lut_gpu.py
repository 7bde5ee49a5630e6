"""Programmable bootstrapping on the GPU (tfhe_amd_bootstrap_lut_*, LUT circuit nodes): every
output word of every launch form of both kernel generations against the oracle composition of
tests/lut_oracle.py (blind rotation from a caller's test vector, extraction, key switch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dev_arena as DA
import lut_oracle as LO
import tfhe_amd as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
N, n_lwe = 1024, 500
E_ARG = -1


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


_cache = {}


def _case8(okey):
    """B = 8 uniformly random inputs through two random tables, and the oracle's extracted samples:
    shared by the guard and the exact-mode tests"""
    if "case8" not in _cache:
        rng = np.random.default_rng(808)
        tvs = _rand32(rng, (2, N))
        idx = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.int32)
        x_a, x_b = _rand32(rng, (8, n_lwe)), _rand32(rng, 8)
        _cache["case8"] = (tvs, idx, x_a, x_b, LO.woks_batch(okey, tvs, x_a, x_b, idx))
    return _cache["case8"]


def test_constant_table_is_the_sign_bootstrap(ctx, okey, keyset):
    rng = np.random.default_rng(501)
    x_a, x_b = keyset.encrypt(rng.integers(0, 2, 8), rng)
    tv = np.full(N, T.MU, np.int32)
    got = ctx.lut_woks_host(tv, x_a, x_b)
    kern = ctx.last_kernels()
    assert _same(got, ctx.woks_host(T.MU, x_a, x_b))
    assert _same(got, LO.woks_batch(okey, tv, x_a, x_b))
    assert _same(got, okey.woks_batch(T.MU, x_a, x_b, nthreads=LO.THREADS))
    assert "k_blind_rotate_v6(lut+lds-rotation)" in kern and "k_blind_rotate_v4(lut+guard)" in kern, kern


def test_random_tables_rotation_edges_host_and_dev(ctx, okey):
    """three tables of uniformly random words (the worst case for the sign wrap), a table index per
    ciphertext, barb at every edge of the negacyclic rotation; woKS and key-switched, host and
    device arrays, the device results written over the inputs"""
    import torch
    rng = np.random.default_rng(606)
    tvs = _rand32(rng, (3, N))
    edges = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    x_b = np.array([np.int64(k) << 21 for k in edges + edges], dtype=np.int64).astype(np.uint32).view(np.int32)
    B = x_b.shape[0]
    x_a = _rand32(rng, (B, n_lwe))
    idx = np.array([0, 1, 2, 2, 1, 0, 1, 2, 0, 0, 2, 1], np.int32)
    assert [int(v) for v in LO.modswitch_2n(x_b)] == edges + edges
    want_u = LO.woks_batch(okey, tvs, x_a, x_b, idx)
    want_r = okey.keyswitch_batch(*want_u, nthreads=LO.THREADS)

    assert _same(ctx.lut_woks_host(tvs, x_a, x_b, idx), want_u)
    assert _same(ctx.lut_bootstrap_host(tvs, x_a, x_b, idx), want_r)

    d = {k: torch.from_numpy(v).cuda() for k, v in (("tv", tvs), ("idx", idx), ("x_a", x_a), ("x_b", x_b))}
    u_a = DA.poisoned((B, N))
    u_b = DA.poisoned(B)
    ctx.lut_woks_dev(d["tv"], u_a, u_b, d["x_a"], d["x_b"], d["idx"])
    ctx.sync()
    assert _same((u_a.cpu().numpy(), u_b.cpu().numpy()), want_u)
    ctx.lut_bootstrap_dev(d["tv"], d["x_a"], d["x_b"], d["x_a"], d["x_b"], d["idx"])   # res aliases x
    ctx.sync()
    assert _same((d["x_a"].cpu().numpy(), d["x_b"].cpu().numpy()), want_r)
    # no index array: table 0 for all
    assert _same(ctx.lut_woks_host(tvs, x_a, x_b), LO.woks_batch(okey, tvs[0], x_a, x_b))


def test_device_index_is_clamped(ctx, okey):
    """the _dev forms take lut_index from device memory unchecked by the host: the kernels (the
    fp64 one and, here with every ciphertext recomputed, the guard's exact one) clamp it into
    [0, n_lut) — documented in include/tfhe_amd.h"""
    import torch
    tvs, _, x_a, x_b, _ = _case8(okey)
    idx = np.array([0, 1, -1, 2, -2**31, 2**31 - 1, 1, 0], np.int32)
    want = LO.woks_batch(okey, tvs, x_a, x_b, np.clip(idx, 0, 1))
    d = [torch.from_numpy(v).cuda() for v in (tvs, x_a, x_b, idx)]
    u_a = DA.poisoned((8, N))
    u_b = DA.poisoned(8)
    for threshold in (0.125, 0.0):
        try:
            T.set_guard_threshold(threshold)
            u_a.fill_(DA.POISON_I32)
            ctx.lut_woks_dev(d[0], u_a, u_b, d[1], d[2], d[3])
            ctx.sync()
        finally:
            T.set_guard_threshold(0.125)
        assert _same((u_a.cpu().numpy(), u_b.cpu().numpy()), want), threshold


def test_prologue_constant_and_two_inputs(ctx, okey):
    rng = np.random.default_rng(707)
    B = 8
    tvs = _rand32(rng, (2, N))
    idx = rng.integers(0, 2, B).astype(np.int32)
    x_a, x_b, y_a, y_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B), _rand32(rng, (B, n_lwe)), _rand32(rng, B)
    c, sa, sb = 0x12345678, 2, -1
    lx = LO.lin(c, [(sa, (x_a, x_b)), (sb, (y_a, y_b))], B)
    want = LO.woks_batch(okey, tvs, lx[0], lx[1], idx)
    assert _same(ctx.lut_woks_host(tvs, x_a, x_b, idx, c=c, sa=sa, sb=sb, y_a=y_a, y_b=y_b), want)
    assert _same(ctx.lut_bootstrap_host(tvs, x_a, x_b, idx, c=c, sa=sa, sb=sb, y_a=y_a, y_b=y_b),
                 okey.keyswitch_batch(*want, nthreads=LO.THREADS))


def test_every_launch_form(ctx, okey):
    """B = CUs + 1: the paired kernel (pair sync) with its padding ciphertext; B = 2 CUs + 1: the
    register rotation (the B = 8 tests ran the LDS rotation); all outputs against the oracle"""
    cus = _cus()
    rng = np.random.default_rng(808)
    tvs = _rand32(rng, (2, N))
    for B, variant in ((cus + 1, "k_blind_rotate_v6p(lut+paired+reg-rotation+pair-sync)"),
                       (2 * cus + 1, "k_blind_rotate_v6(lut+reg-rotation)")):
        x_a, x_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B)
        idx = rng.integers(0, 2, B).astype(np.int32)
        got = ctx.lut_woks_host(tvs, x_a, x_b, idx)
        kern = ctx.last_kernels()
        assert _same(got, LO.woks_batch(okey, tvs, x_a, x_b, idx)), B   # parity first, then which kernel
        assert variant in kern and "k_blind_rotate_v4(lut+guard)" in kern, (B, kern)


def test_paired_barrier_variant_subprocess():
    """TFHE_AMD_V6P_PAIRSYNC=0 (read once per process): the paired LUT kernel with the workgroup
    barrier, an odd batch (one padding ciphertext), against the oracle"""
    code = r"""
import sys, numpy as np, torch
sys.path[:0] = [%r, %r]
import tfhe_amd as T, oracle_ctypes as O, lut_oracle as LO
K = T.SecretKeyset(); c = T.Context(K.bk, K.ksk, device=0); o = O.OracleKey(K.bk, K.ksk)
rng = np.random.default_rng(909)
B = torch.cuda.get_device_properties(0).multi_processor_count + 1
r32 = lambda shape: rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)
tvs, x_a, x_b, idx = r32((2, 1024)), r32((B, 500)), r32(B), rng.integers(0, 2, B).astype(np.int32)
u = c.lut_woks_host(tvs, x_a, x_b, idx)
kern = c.last_kernels()
w = LO.woks_batch(o, tvs, x_a, x_b, idx)
assert np.array_equal(u[0], w[0]) and np.array_equal(u[1], w[1])
assert "k_blind_rotate_v6p(lut+paired+reg-rotation)" in kern, kern
print("lut barrier ok")
""" % (os.path.join(REPO, "cpu-gpu-tfhe_amd"), HERE)
    env = dict(os.environ, TFHE_AMD_V6P_PAIRSYNC="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lut barrier ok" in r.stdout


def test_guard_recomputes_with_the_same_table(ctx, okey):
    tvs, idx, x_a, x_b, want = _case8(okey)
    try:
        T.set_guard_threshold(0.0)
        ctx.guard_stats(reset=True)
        got = ctx.lut_woks_host(tvs, x_a, x_b, idx)
        kern = ctx.last_kernels()
        _, recomputed = ctx.guard_stats(reset=True)
    finally:
        T.set_guard_threshold(0.125)
    assert recomputed == 8
    assert _same(got, want)
    assert "k_blind_rotate_v4(lut+guard)" in kern, kern


def test_exact_kernel(ctx, okey):
    tvs, idx, x_a, x_b, want = _case8(okey)
    try:
        T.select_kernel(4)
        got = ctx.lut_woks_host(tvs, x_a, x_b, idx)
        kern = ctx.last_kernels()
        got_r = ctx.lut_bootstrap_host(tvs, x_a, x_b, idx)
    finally:
        T.select_kernel(0)
    assert _same(got, want)
    assert _same(got_r, okey.keyswitch_batch(*want, nthreads=LO.THREADS))
    assert kern == ["k_blind_rotate_v4(lut)"], kern


@pytest.mark.parametrize("p", [4, 8])
def test_decode(ctx, okey, keyset, p):
    msgs, f, tv, x_a, x_b = LO.decode_case(keyset, p)
    got = ctx.lut_bootstrap_host(tv, x_a, x_b)
    assert _same(got, LO.decode_expected(keyset, okey, p))
    assert np.array_equal(T.lut_decode(keyset.phase(*got), p), f[msgs])


def test_argument_errors(ctx):
    import torch
    lib = T.lib
    B = 4
    tv = np.zeros((2, N), np.int32)
    x_a, x_b = np.zeros((B, n_lwe), np.int32), np.zeros(B, np.int32)
    u_a, u_b = np.zeros((B, N), np.int32), np.zeros(B, np.int32)
    p = T._p
    for fn in (lib.tfhe_amd_bootstrap_lut_woks_batch_host, lib.tfhe_amd_bootstrap_lut_batch_host):
        def call(Bv=B, n_lut=2, tvp=p(tv), idx=None):
            return fn(ctx.h, Bv, n_lut, tvp, idx, 0, 1, p(x_a), p(x_b), 0, None, None, p(u_a), p(u_b))
        assert call(n_lut=0) == E_ARG and call(n_lut=-3) == E_ARG
        assert call(tvp=None) == E_ARG
        assert call(Bv=-1) == E_ARG
        for bad in (-1, 2):
            idx = np.array([0, 1, bad, 0], np.int32)
            assert call(idx=p(idx)) == E_ARG, bad
        assert call(idx=p(np.array([0, 1, 1, 0], np.int32))) == 0
        assert call(Bv=0) == 0
    d_tv = torch.zeros((2, N), dtype=torch.int32, device="cuda")
    d_x_a = torch.zeros((B, n_lwe), dtype=torch.int32, device="cuda")
    d_x_b = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_u_a = torch.zeros((B, N), dtype=torch.int32, device="cuda")
    d_u_b = torch.zeros(B, dtype=torch.int32, device="cuda")
    for fn in (lib.tfhe_amd_bootstrap_lut_woks_batch_dev, lib.tfhe_amd_bootstrap_lut_batch_dev):
        def call(Bv=B, n_lut=2, tvp=d_tv.data_ptr()):
            return fn(ctx.h, Bv, n_lut, tvp, None, 0, 1, d_x_a.data_ptr(), d_x_b.data_ptr(), 0, None, None,
                      d_u_a.data_ptr(), d_u_b.data_ptr(), None)
        assert call(n_lut=0) == E_ARG and call(tvp=None) == E_ARG and call(Bv=-1) == E_ARG
        assert call() == 0
    ctx.sync()
    with pytest.raises(T.TfheAmdError):
        ctx.lut_woks_host(tv, x_a, x_b, sb=1)   # sb != 0 without Y


# ---------------------------------------------------------------- circuits

P = 8
Q27 = 1 << 27   # 1/(4p) of the torus for p = 8


def _adder():
    """2-digit radix-4 adder on p = 8 digit ciphertexts: per digit x = A + B (+ carry) — each
    added term shifts the centre by 1/(4p), taken back by c0 — feeds a sum table (x & 3) and a
    carry table (x >> 2) in one level; level 1 also holds a plain NAND row on two bit inputs"""
    C = T.Circuit()
    a0, a1, b0, b1, e0, e1 = C.inputs(6)
    x = np.arange(P)
    t_sum = C.lut_table(T.lut_table(P, T.lut_encode(x & 3, P)))
    t_car = C.lut_table(T.lut_table(P, T.lut_encode(x >> 2, P)))
    s0 = C.lut(t_sum, -Q27, 1, a0, 1, b0)
    c0 = C.lut(t_car, -Q27, 1, a0, 1, b0)
    nand = C.gate("NAND", e0, e1)
    s1 = C.lut(t_sum, -2 * Q27, 1, a1, 1, b1, 1, c0)
    c1 = C.lut(t_car, -2 * Q27, 1, a1, 1, b1, 1, c0)
    assert C.level_sizes() == [0, 3, 2]
    return C, (a0, a1, b0, b1, e0, e1), (s0, c0, nand, s1, c1)


def _adder_case(keyset, okey, B):
    """inputs and the node-by-node oracle evaluation of the adder for B instances (once per B)"""
    key = ("adder", B)
    if key not in _cache:
        rng = np.random.default_rng(1200 + B)
        C, ins, outs = _adder()
        digits = [rng.integers(0, 4, B) for _ in range(4)]
        bits = [rng.integers(0, 2, B) for _ in range(2)]
        enc = [keyset.encrypt_digits(d, P, rng) for d in digits] + [keyset.encrypt(b, rng) for b in bits]
        W = LO.eval_circuit(C, okey, dict(zip(ins, enc)), B)
        _cache[key] = (C, ins, outs, digits, bits, enc, W)
    return _cache[key]


def _check_adder(keyset, case, got_a, got_b, wires):
    C, ins, outs, digits, bits, enc, W = case
    for j, w in enumerate(wires):
        assert np.array_equal(got_a[j], W[w][0]) and np.array_equal(got_b[j], W[w][1]), w
    s0, c0, nand, s1, c1 = (T.lut_decode(keyset.phase(got_a[wires.index(w)], got_b[wires.index(w)]), P)
                            if w != outs[2] else keyset.decrypt(got_a[wires.index(w)], got_b[wires.index(w)])
                            for w in outs)
    a = digits[0] + 4 * digits[1]
    b = digits[2] + 4 * digits[3]
    assert np.array_equal(s0 + 4 * s1 + 16 * c1, a + b)
    assert np.array_equal(c0, (digits[0] + digits[2]) >> 2)
    assert np.array_equal(nand, 1 - (bits[0] & bits[1]))


def _run_adder(ctx, case, B):
    import torch
    C, ins, outs, digits, bits, enc, W = case
    n_w = C.info()["wires"]
    wa = DA.poisoned((n_w, B, n_lwe))      # every wire the run does not write stays poison
    wb = DA.poisoned((n_w, B))
    for w, (a, b) in zip(ins, enc):
        wa[w] = torch.from_numpy(a).cuda()
        wb[w] = torch.from_numpy(b).cuda()
    C.run_dev(ctx, B, wa, wb)
    ctx.sync()
    kern = ctx.last_kernels()
    return wa.cpu().numpy(), wb.cpu().numpy(), kern


def test_circuit_radix4_adder(ctx, okey, keyset):
    """LUT rows of two tables and a gate row in one launch; B = 5 (LDS rotation) and rows x B above
    one workgroup per CU on every level (register rotation); every wire against the oracle"""
    big = _cus() // 2 + 2   # 2 rows (the smaller level) x B > CUs
    for B, variant in ((5, "k_blind_rotate_v6_rows(lut+lds-rotation)"), (big, "k_blind_rotate_v6_rows(lut+reg-rotation)")):
        case = _adder_case(keyset, okey, B)
        ha, hb, kern = _run_adder(ctx, case, B)
        _check_adder(keyset, case, ha, hb, list(range(ha.shape[0])))
        assert variant in kern and "k_blind_rotate_v4_rows(lut+guard)" in kern, (B, kern)
        assert not any(k.startswith("k_blind_rotate_v6_rows(") and "lut" not in k for k in kern), kern


def test_circuit_radix4_adder_exact_kernel(ctx, okey, keyset):
    case = _adder_case(keyset, okey, 5)
    try:
        T.select_kernel(4)
        ha, hb, kern = _run_adder(ctx, case, 5)
    finally:
        T.select_kernel(0)
    _check_adder(keyset, case, ha, hb, list(range(ha.shape[0])))
    assert "k_blind_rotate_v4_rows(lut)" in kern, kern


def test_gate_only_levels_keep_the_constant_kernels(ctx, keyset):
    """a level without LUT rows of a circuit that has LUT rows elsewhere launches the constant rows
    kernel, a level with them the LUT one"""
    rng = np.random.default_rng(77)
    C = T.Circuit()
    a, b = C.inputs(2)
    g = C.gate("AND", a, b)
    t = C.lut_table(np.full(N, -T.MU, np.int32))          # the negated sign: a NOT through a table
    x = C.lut(t, 0, 1, g)
    bits = {a: rng.integers(0, 2, 3), b: rng.integers(0, 2, 3)}
    out = C.run(ctx, 3, bits, [g, x], keyset, rng)
    kern = ctx.last_kernels()
    assert np.array_equal(out[g], bits[a] & bits[b]) and np.array_equal(out[x], 1 - (bits[a] & bits[b]))
    assert "k_blind_rotate_v6_rows(lds-rotation)" in kern and "k_blind_rotate_v6_rows(lut+lds-rotation)" in kern, kern
    C.close()


def test_multi_circuit(okey, keyset):
    B = 5
    case = _adder_case(keyset, okey, B)
    C, ins, outs, digits, bits, enc, W = case
    m = T.MultiContext(keyset.bk, keyset.ksk, [0, 0])
    try:
        in_a = np.stack([e[0] for e in enc])
        in_b = np.stack([e[1] for e in enc])
        out_a, out_b = m.circuit_host(C, B, list(ins), in_a, in_b, list(outs))
    finally:
        m.close()
    _check_adder(keyset, case, out_a, out_b, list(outs))
