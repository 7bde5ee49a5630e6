"""Many-LUT bootstrapping on the GPU (tfhe_amd_bootstrap_lut_many_*, many-LUT circuit nodes,
DESIGN.md §3.3): every output word of every launch form of both kernel generations against the
oracle composition of tests/many_lut_oracle.py (coarse modulus switch, ONE blind rotation per
sample, extraction at the indices 0 .. n_out - 1, key switch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dev_arena as DA
import lut_oracle as LO
import many_lut_oracle as MO
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
    return (got[0].shape == want[0].shape and got[1].shape == want[1].shape and
            np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


_cache = {}


def _case8(okey):
    """B = 8 uniformly random inputs through two random tables at theta = 2, n_out = 4, and the
    oracle's extracted samples: shared by the guard and the exact-mode tests"""
    if "case8" not in _cache:
        rng = np.random.default_rng(1808)
        tvs = _rand32(rng, (2, N))
        idx = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.int32)
        x_a, x_b = _rand32(rng, (8, n_lwe)), _rand32(rng, 8)
        _cache["case8"] = (tvs, idx, x_a, x_b, MO.woks_batch(okey, tvs, x_a, x_b, 2, 4, idx))
    return _cache["case8"]


def test_theta_0_is_the_single_table_path(ctx, okey):
    rng = np.random.default_rng(1501)
    tvs = _rand32(rng, (2, N))
    x_a, x_b = _rand32(rng, (8, n_lwe)), _rand32(rng, 8)
    idx = rng.integers(0, 2, 8).astype(np.int32)
    got = ctx.lut_many_woks_host(tvs, 0, 1, x_a, x_b, idx)
    kern = ctx.last_kernels()
    single = ctx.lut_woks_host(tvs, x_a, x_b, idx)
    assert got[0].shape == (1, 8, N) and got[1].shape == (1, 8)
    assert _same((got[0][0], got[1][0]), single)
    assert _same(got, MO.woks_batch(okey, tvs, x_a, x_b, 0, 1, idx))
    assert "k_blind_rotate_v6(lut-many+lds-rotation)" in kern and "k_blind_rotate_v4(lut-many+guard)" in kern, kern


@pytest.mark.parametrize("theta,n_out", [(1, 2), (2, 4), (3, 8), (4, 16), (2, 3)])
def test_random_tables_rotation_edges_host_and_dev(ctx, okey, theta, n_out):
    """three tables of uniformly random words, a table index per ciphertext, barb at every edge of
    the negacyclic rotation and at the rounding boundaries of the coarse switch; woKS and
    key-switched, host and device arrays, the function-major layout, the device result written over
    the inputs"""
    import torch
    rng = np.random.default_rng(1606 + theta)
    nu = 1 << theta
    tvs = _rand32(rng, (3, N))
    edges = [0, nu, N - nu, N, N + nu, 2 * N - nu]
    q = 5
    half = ((nu * q + nu // 2) << 21)
    words = [k << 21 for k in edges] + [half - 1, half, 2**32 - (1 << (20 + theta))]
    x_b = np.concatenate([np.array(words, dtype=np.int64).astype(np.uint32).view(np.int32), _rand32(rng, 3)])
    B = x_b.shape[0]
    assert B == 12
    assert [int(v) for v in MO.bar(x_b[:9], theta)] == edges + [nu * q, nu * (q + 1), 0]
    x_a = _rand32(rng, (B, n_lwe))
    idx = np.array([0, 1, 2, 2, 1, 0, 1, 2, 0, 0, 2, 1], np.int32)
    want_u = MO.woks_batch(okey, tvs, x_a, x_b, theta, n_out, idx)
    want_r = MO.keyswitch(okey, want_u)
    assert want_u[0].shape == (n_out, B, N) and want_r[0].shape == (n_out, B, n_lwe)

    got_u = ctx.lut_many_woks_host(tvs, theta, n_out, x_a, x_b, idx)
    assert _same(got_u, want_u)
    # function-major: block f is the batch of function f, an ordinary batch for the next call
    one = MO.woks_one(okey, tvs[idx[3]], x_a[3], x_b[3], theta, n_out)
    for f in range(n_out):
        assert np.array_equal(got_u[0][f, 3], one[0][f]) and got_u[1][f, 3] == one[1][f], f
    assert _same(ctx.lut_many_bootstrap_host(tvs, theta, n_out, x_a, x_b, idx), want_r)

    d = {k: torch.from_numpy(v).cuda() for k, v in (("tv", tvs), ("idx", idx), ("x_a", x_a), ("x_b", x_b))}
    u_a = DA.poisoned((n_out, B, N))
    u_b = DA.poisoned((n_out, B))
    ctx.lut_many_woks_dev(d["tv"], theta, n_out, u_a, u_b, d["x_a"], d["x_b"], d["idx"])
    ctx.sync()
    assert _same((u_a.cpu().numpy(), u_b.cpu().numpy()), want_u)
    # the key-switched result over the inputs: X is the first block of the result's storage
    r_a = DA.poisoned((n_out, B, n_lwe))
    r_b = DA.poisoned((n_out, B))
    r_a[0].copy_(d["x_a"])
    r_b[0].copy_(d["x_b"])
    ctx.lut_many_bootstrap_dev(d["tv"], theta, n_out, r_a, r_b, r_a[0], r_b[0], d["idx"])
    ctx.sync()
    assert _same((r_a.cpu().numpy(), r_b.cpu().numpy()), want_r)
    # no index array: table 0 for all
    assert _same(ctx.lut_many_woks_host(tvs, theta, n_out, x_a, x_b), MO.woks_batch(okey, tvs[0], x_a, x_b, theta, n_out))


def test_prologue_constant_and_two_inputs(ctx, okey):
    rng = np.random.default_rng(1707)
    B = 8
    tvs = _rand32(rng, (2, N))
    idx = rng.integers(0, 2, B).astype(np.int32)
    x_a, x_b, y_a, y_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B), _rand32(rng, (B, n_lwe)), _rand32(rng, B)
    c, sa, sb = 0x12345678, 2, -1
    lx = LO.lin(c, [(sa, (x_a, x_b)), (sb, (y_a, y_b))], B)
    want = MO.woks_batch(okey, tvs, lx[0], lx[1], 1, 2, idx)
    assert _same(ctx.lut_many_woks_host(tvs, 1, 2, x_a, x_b, idx, c=c, sa=sa, sb=sb, y_a=y_a, y_b=y_b), want)
    assert _same(ctx.lut_many_bootstrap_host(tvs, 1, 2, x_a, x_b, idx, c=c, sa=sa, sb=sb, y_a=y_a, y_b=y_b),
                 MO.keyswitch(okey, want))


def test_every_launch_form(ctx, okey):
    """B = CUs + 1: the paired kernel (pair sync) with its padding ciphertext; B = 2 CUs + 1: the
    register rotation (the small-batch tests ran the LDS rotation); all outputs against the oracle"""
    cus = _cus()
    rng = np.random.default_rng(1808)
    tvs = _rand32(rng, (2, N))
    for B, variant in ((cus + 1, "k_blind_rotate_v6p(lut-many+paired+reg-rotation+pair-sync)"),
                       (2 * cus + 1, "k_blind_rotate_v6(lut-many+reg-rotation)")):
        x_a, x_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B)
        idx = rng.integers(0, 2, B).astype(np.int32)
        got = ctx.lut_many_woks_host(tvs, 1, 2, x_a, x_b, idx)
        kern = ctx.last_kernels()
        assert _same(got, MO.woks_batch(okey, tvs, x_a, x_b, 1, 2, idx)), B   # parity first, then which kernel
        assert variant in kern and "k_blind_rotate_v4(lut-many+guard)" in kern, (B, kern)


def test_paired_barrier_variant_subprocess():
    """TFHE_AMD_V6P_PAIRSYNC=0 (read once per process): the paired many-LUT kernel with the
    workgroup barrier, an odd batch (one padding ciphertext), against the oracle"""
    code = r"""
import sys, numpy as np, torch
sys.path[:0] = [%r, %r]
import tfhe_amd as T, oracle_ctypes as O, many_lut_oracle as MO
K = T.SecretKeyset(); c = T.Context(K.bk, K.ksk, device=0); o = O.OracleKey(K.bk, K.ksk)
rng = np.random.default_rng(1909)
B = torch.cuda.get_device_properties(0).multi_processor_count + 1
r32 = lambda shape: rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)
tvs, x_a, x_b, idx = r32((2, 1024)), r32((B, 500)), r32(B), rng.integers(0, 2, B).astype(np.int32)
u = c.lut_many_woks_host(tvs, 1, 2, x_a, x_b, idx)
kern = c.last_kernels()
w = MO.woks_batch(o, tvs, x_a, x_b, 1, 2, idx)
assert u[0].shape == w[0].shape and np.array_equal(u[0], w[0]) and np.array_equal(u[1], w[1])
assert "k_blind_rotate_v6p(lut-many+paired+reg-rotation)" in kern, kern
print("lut-many barrier ok")
""" % (os.path.join(REPO, "cpu-gpu-tfhe_amd"), HERE)
    env = dict(os.environ, TFHE_AMD_V6P_PAIRSYNC="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lut-many barrier ok" in r.stdout


def test_guard_recomputes_every_output(ctx, okey):
    """threshold 0: every ciphertext is flagged and the exact kernel rewrites all its n_out = 4
    outputs with the same theta and table; the counter counts ciphertexts, not outputs"""
    tvs, idx, x_a, x_b, want = _case8(okey)
    default = ctx.lut_many_woks_host(tvs, 2, 4, x_a, x_b, idx)
    try:
        T.set_guard_threshold(0.0)
        ctx.guard_stats(reset=True)
        got = ctx.lut_many_woks_host(tvs, 2, 4, x_a, x_b, idx)
        kern = ctx.last_kernels()
        _, recomputed = ctx.guard_stats(reset=True)
    finally:
        T.set_guard_threshold(0.125)
    assert recomputed == 8
    assert _same(got, default) and _same(got, want)
    assert "k_blind_rotate_v4(lut-many+guard)" in kern, kern


def test_exact_kernel(ctx, okey):
    tvs, idx, x_a, x_b, want = _case8(okey)
    try:
        T.select_kernel(4)
        got = ctx.lut_many_woks_host(tvs, 2, 4, x_a, x_b, idx)
        kern = ctx.last_kernels()
        got_r = ctx.lut_many_bootstrap_host(tvs, 2, 4, x_a, x_b, idx)
    finally:
        T.select_kernel(0)
    assert _same(got, want)
    assert _same(got_r, MO.keyswitch(okey, want))
    assert kern == ["k_blind_rotate_v4(lut-many)"], kern


@pytest.mark.parametrize("p,theta,n_out", MO.DECODE_CASES)
def test_decode(ctx, okey, keyset, p, theta, n_out):
    msgs, f, tv, x_a, x_b = MO.decode_case(keyset, p, theta, n_out)
    got = ctx.lut_many_bootstrap_host(tv, theta, n_out, x_a, x_b)
    assert _same(got, MO.decode_expected(keyset, okey, p, theta, n_out))
    for r in range(n_out):
        assert np.array_equal(T.lut_decode(keyset.phase(got[0][r], got[1][r]), p), f[r][msgs]), r


def test_argument_errors(ctx):
    import torch
    lib = T.lib
    B = 4
    tv = np.zeros((2, N), np.int32)
    x_a, x_b = np.zeros((B, n_lwe), np.int32), np.zeros(B, np.int32)
    u_a, u_b = np.zeros((4, B, N), np.int32), np.zeros((4, B), np.int32)
    p = T._p
    for fn in (lib.tfhe_amd_bootstrap_lut_many_woks_batch_host, lib.tfhe_amd_bootstrap_lut_many_batch_host):
        def call(Bv=B, n_lut=2, tvp=p(tv), idx=None, theta=1, n_out=2):
            return fn(ctx.h, Bv, n_lut, tvp, idx, theta, n_out, 0, 1, p(x_a), p(x_b), 0, None, None, p(u_a), p(u_b))
        for theta, n_out in ((-1, 1), (5, 1), (1, 0), (1, 3), (0, 0), (0, 2), (2, 5), (4, 17)):
            assert call(theta=theta, n_out=n_out) == E_ARG, (theta, n_out)
        assert call(n_lut=0) == E_ARG and call(n_lut=-3) == E_ARG
        assert call(tvp=None) == E_ARG
        assert call(Bv=-1) == E_ARG
        for bad in (-1, 2):
            idx = np.array([0, 1, bad, 0], np.int32)
            assert call(idx=p(idx)) == E_ARG, bad
        assert call(idx=p(np.array([0, 1, 1, 0], np.int32))) == 0
        assert call(Bv=0) == 0
        assert call(theta=2, n_out=4) == 0
    d_tv = torch.zeros((2, N), dtype=torch.int32, device="cuda")
    d_x_a = torch.zeros((B, n_lwe), dtype=torch.int32, device="cuda")
    d_x_b = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_u_a = torch.zeros((4, B, N), dtype=torch.int32, device="cuda")
    d_u_b = torch.zeros((4, B), dtype=torch.int32, device="cuda")
    for fn in (lib.tfhe_amd_bootstrap_lut_many_woks_batch_dev, lib.tfhe_amd_bootstrap_lut_many_batch_dev):
        def call(Bv=B, n_lut=2, tvp=d_tv.data_ptr(), theta=1, n_out=2):
            return fn(ctx.h, Bv, n_lut, tvp, None, theta, n_out, 0, 1, d_x_a.data_ptr(), d_x_b.data_ptr(), 0, None,
                      None, d_u_a.data_ptr(), d_u_b.data_ptr(), None)
        for theta, n_out in ((-1, 1), (5, 1), (1, 0), (1, 3), (0, 0), (0, 2), (2, 5), (4, 17)):
            assert call(theta=theta, n_out=n_out) == E_ARG, (theta, n_out)
        assert call(n_lut=0) == E_ARG and call(tvp=None) == E_ARG and call(Bv=-1) == E_ARG
        assert call() == 0
    ctx.sync()
    with pytest.raises(T.TfheAmdError):
        ctx.lut_many_woks_host(tv, 1, 2, x_a, x_b, sb=1)   # sb != 0 without Y
    with pytest.raises(T.TfheAmdError):
        ctx.lut_many_woks_host(tv, 1, 3, x_a, x_b)         # n_out > nu
    with pytest.raises(T.TfheAmdError):                    # outputs of the wrong shape never reach the GPU
        ctx.lut_many_woks_dev(d_tv, 1, 2, d_u_a, d_u_b, d_x_a, d_x_b)


# ---------------------------------------------------------------- circuits

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


def _check_adder(keyset, case, got):
    """got = {wire: (a, b)}: every wire against the oracle's node-by-node evaluation, then the sums"""
    W = case[6]
    for w, (a, b) in got.items():
        assert np.array_equal(a, W[w][0]) and np.array_equal(b, W[w][1]), w
    for g, t in zip(MO.adder_decoded(keyset, case, got), MO.adder_truth(case)):
        assert np.array_equal(g, t)


def test_circuit_radix4_adder(ctx, okey, keyset):
    """one many-LUT row per digit; level 1 also holds a NAND row, a plain LUT row and a many-LUT row
    of another theta, all in one launch; B = 5 (LDS rotation) and B = CUs / 2 + 2 (level 1: register
    rotation); every wire against the oracle"""
    big = _cus() // 2 + 2
    for B, variant in ((5, "k_blind_rotate_v6_rows(lut-many+lds-rotation)"),
                       (big, "k_blind_rotate_v6_rows(lut-many+reg-rotation)")):
        case = MO.adder_case(keyset, okey, B)
        assert case[0].level_sizes() == [0, 4, 1]   # test_lut_gpu.py's adder: two rows per digit
        ha, hb, kern = _run_adder(ctx, case, B)
        _check_adder(keyset, case, {w: (ha[w], hb[w]) for w in range(ha.shape[0])})
        assert variant in kern and "k_blind_rotate_v4_rows(lut-many+guard)" in kern, (B, kern)
        assert not any(k.startswith("k_blind_rotate_v6_rows(") and "lut-many" not in k for k in kern), kern


def test_circuit_radix4_adder_exact_kernel(ctx, okey, keyset):
    case = MO.adder_case(keyset, okey, 5)
    try:
        T.select_kernel(4)
        ha, hb, kern = _run_adder(ctx, case, 5)
    finally:
        T.select_kernel(0)
    _check_adder(keyset, case, {w: (ha[w], hb[w]) for w in range(ha.shape[0])})
    assert "k_blind_rotate_v4_rows(lut-many)" in kern, kern


def test_circuit_guard_recomputes_every_output(ctx, okey, keyset):
    """threshold 0 in a circuit: the exact rows kernel rewrites all outputs of every many-LUT row"""
    case = MO.adder_case(keyset, okey, 5)
    try:
        T.set_guard_threshold(0.0)
        ha, hb, kern = _run_adder(ctx, case, 5)
    finally:
        T.set_guard_threshold(0.125)
    _check_adder(keyset, case, {w: (ha[w], hb[w]) for w in range(ha.shape[0])})
    assert "k_blind_rotate_v4_rows(lut-many+guard)" in kern, kern


def test_gate_only_levels_keep_the_constant_kernels(ctx, keyset):
    """a gate-only level of a circuit that has many-LUT rows elsewhere launches the constant rows
    kernel, a LUT-only level the LUT one, the level with the many-LUT row the many-LUT one"""
    rng = np.random.default_rng(177)
    C = T.Circuit()
    a, b = C.inputs(2)
    g = C.gate("AND", a, b)
    t = C.lut_table(np.full(N, -T.MU, np.int32))          # the negated sign: a NOT through a table
    x = C.lut_many(t, 1, 2, 0, 1, g)                      # both outputs: NOT g (tv is constant)
    y = C.lut(t, 0, 1, x + 1)
    bits = {a: rng.integers(0, 2, 3), b: rng.integers(0, 2, 3)}
    out = C.run(ctx, 3, bits, [g, x, x + 1, y], keyset, rng)
    kern = ctx.last_kernels()
    ab = bits[a] & bits[b]
    assert np.array_equal(out[g], ab) and np.array_equal(out[x], 1 - ab) and np.array_equal(out[x + 1], 1 - ab)
    assert np.array_equal(out[y], ab)
    for k in ("k_blind_rotate_v6_rows(lds-rotation)", "k_blind_rotate_v6_rows(lut+lds-rotation)",
              "k_blind_rotate_v6_rows(lut-many+lds-rotation)"):
        assert k in kern, kern
    C.close()


def test_multi_circuit(okey, keyset):
    B = 5
    case = MO.adder_case(keyset, okey, B)
    C, ins, outs, digits, bits, enc, W = case
    wires = list(range(6, C.info()["wires"]))
    m = T.MultiContext(keyset.bk, keyset.ksk, [0, 0])
    try:
        in_a = np.stack([e[0] for e in enc])
        in_b = np.stack([e[1] for e in enc])
        out_a, out_b = m.circuit_host(C, B, list(ins), in_a, in_b, wires)
    finally:
        m.close()
    got = {w: (out_a[j], out_b[j]) for j, w in enumerate(wires)}
    _check_adder(keyset, case, got)
