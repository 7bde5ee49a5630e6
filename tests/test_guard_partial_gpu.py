"""Partly flagged batches through every launch form of the exactness guard.

The fp64 blind rotation writes two flag words per ciphertext slot and the exact kernel in guard
mode reads them back; each computes the slot on its own, per launch form.  Here a chosen subset of
a batch's blind rotations must be recomputed (tests/guard_cases.py: the head-250 key, dirty samples
among clean ones), and every dirty sample placed is one the unguarded fp64 kernel gets wrong on this
GPU (the qualified pool below), so a flag written to or read from another slot, or one left over
from an earlier launch, shows as a wrong output word or a wrong recomputed count.

Each case asserts: (a) every output word of every ciphertext equals the oracle's
(O.OracleKey(bk_head250, ksk, use_ntt=True), nothing decrypted); (b) tfhe_amd_guard_stats counts
exactly the dirty blind rotations (a MUX half counts 1); (c) the reported distance is >= 1/8 when
anything is dirty; (d) tfhe_amd_last_kernels names the form the case is meant to reach."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import dev_arena as DA
import circuit_oracle
import guard_cases as G
import lut_oracle as LO
import many_lut_oracle as MLO
import oracle_ctypes as O
import tfhe_amd as T

pytestmark = pytest.mark.gpu

NT = 8   # oracle threads
GUARD = "k_blind_rotate_v4(guard)"
ROWS = ["k_blind_rotate_v6_rows(lds-rotation)", "k_blind_rotate_v4_rows(guard)"]
LDS, REG = "k_blind_rotate_v6(lds-rotation)", "k_blind_rotate_v6(reg-rotation)"
PAIRED = "k_blind_rotate_v6p(paired+reg-rotation+pair-sync)"
POOL = 32
MOST_DIRTY = 5   # the most dirty samples one case places: each slot gets its own


@pytest.fixture(scope="module")
def cus():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def P(cus):
    return G.placements(cus)


@pytest.fixture(scope="module")
def hkey(keyset):
    bk = G.head_key(keyset.bk)
    return bk, O.OracleKey(bk, keyset.ksk, use_ntt=True)


@pytest.fixture(scope="module")
def hctx(keyset, hkey):
    c = T.Context(hkey[0], keyset.ksk, device=0)
    yield c
    c.close()


def _oracle_acc(okey, tv_rot, bara):
    """the exact accumulators [n][2][N] of ACC = (0, tv_rot[k]) after the 500 steps bara[k]"""
    acc = np.zeros((bara.shape[0], 2, G.N), np.int32)
    acc[:, 1] = tv_rot
    bara = np.ascontiguousarray(bara)

    def one(k):   # ctypes releases the GIL
        O.lib().orc_blind_rotate(O._p(acc[k].reshape(2 * G.N)), ctypes.c_void_p(okey.h), O._p(bara[k]), G.n_lwe)
    with ThreadPoolExecutor(NT) as tp:
        list(tp.map(one, range(bara.shape[0])))
    return acc


def _raw_acc(ctx, tv_rot, bara):
    """the same through the raw fp64 CMux steps (tfhe_amd_blind_rotate_dev: the fp64 step kernel with
    no exactness guard, as test_guard._raw_fp64_woks): what the fp64 kernel computes unchecked"""
    import torch
    acc = np.zeros((bara.shape[0], 2, G.N), np.int32)
    acc[:, 1] = tv_rot
    d_acc = torch.from_numpy(acc).cuda()
    ctx.blind_rotate_dev(d_acc, torch.from_numpy(np.ascontiguousarray(bara)).cuda(), G.n_lwe)
    ctx.sync()
    return d_acc.cpu().numpy()


def _qualify(ctx, okey, cand, what, tv=None, theta=0, n_out=1):
    """The candidates whose unguarded fp64 result is wrong on this GPU: ACC = X^{2N - barb} tv (tv:
    the constant mu, or a table), the 500 raw steps and the extractions at 0 .. n_out - 1, against
    the same from the oracle's exact accumulator.  At least half must differ (the fp64 CPU port:
    56 of 64): with fewer the placements could pass vacuously, so that fails — it does not skip.
    Some wrong extractions differ only in bits the key switch drops (it reads the top 16 of each
    word), and every form here is key-switched: the candidates returned, the only ones placed, are
    those of the wrong ones whose key-switched output differs as well (the CPU port: 20 of 32)."""
    a, b = cand
    n = b.shape[0]
    tv = np.full(G.N, G.MU, np.int32) if tv is None else tv
    bara, barb = MLO.bar(a, theta), MLO.bar(b, theta)
    rot = np.stack([O.mul_by_xai((2 * G.N - int(e)) % (2 * G.N), tv) for e in barb])
    wrong, wrong_ks = np.zeros(n, bool), np.zeros(n, bool)
    raw, exact = _raw_acc(ctx, rot, bara), _oracle_acc(okey, rot, bara)
    for f in range(n_out):
        u = [[MLO.extract(acc[k, 0], acc[k, 1], f) for k in range(n)] for acc in (raw, exact)]
        u = [(np.stack([x[0] for x in v]), np.array([x[1] for x in v], np.int32)) for v in u]
        ks = [okey.keyswitch_batch(*v, nthreads=NT) for v in u]
        wrong |= (u[0][0] != u[1][0]).any(axis=1) | (u[0][1] != u[1][1])
        wrong_ks |= (ks[0][0] != ks[1][0]).any(axis=1) | (ks[0][1] != ks[1][1])
    print(f"qualified pool ({what}): {int(wrong.sum())} of {n} candidates wrong unguarded, "
          f"{int(wrong_ks.sum())} still wrong after the key switch")
    if 2 * int(wrong.sum()) < n or int(wrong_ks.sum()) < MOST_DIRTY:
        pytest.fail(f"{int(wrong.sum())} of {n} dirty candidates come out wrong unguarded, {int(wrong_ks.sum())} "
                    f"after the key switch: the pool is too thin")
    return a[wrong_ks], b[wrong_ks]


@pytest.fixture(scope="module")
def cand():
    return G.dirty(np.random.default_rng(20250), POOL)


@pytest.fixture(scope="module")
def pool(hctx, hkey, cand):
    """the dirty candidates the raw fp64 gate rotation (constant test vector mu) gets wrong"""
    return _qualify(hctx, hkey[1], cand, "constant mu")


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _bad_rows(got, want):
    return np.flatnonzero((got[0] != want[0]).any(axis=-1) | (got[1] != want[1]))


def _stats(ctx, name, n_dirty, kern):
    dist, redo = ctx.guard_stats(reset=True)
    print(f"{name}: recomputed {redo} (dirty {n_dirty}), distance {dist:.4f}, kernels {kern}")
    assert redo == n_dirty, (name, redo, n_dirty)
    if n_dirty:
        assert dist >= 0.125, (name, dist)
    else:
        assert dist < 0.125, (name, dist)


def _nand_host(ctx, okey, x, name, n_dirty, want_kern):
    ins = G.gate_inputs("NAND", *x)
    ctx.guard_stats(reset=True)
    got = ctx.gate_host("NAND", *ins)
    kern = ctx.last_kernels()
    _stats(ctx, name, n_dirty, kern)
    want = okey.gate_batch("NAND", *ins, nthreads=NT)
    bad = _bad_rows(got, want)
    assert bad.size == 0, (name, bad[:8])
    for k in want_kern:
        assert k in kern, (name, kern)
    return kern


def test_one_ciphertext_lds_rotation(hctx, hkey, pool, P):
    """case 1: bootstrap_host, B = 6, dirty {1, 4}"""
    p = P["lds"]
    x = G.batch(np.random.default_rng(101), p["B"], p["dirty"], p["real"], pool)
    hctx.guard_stats(reset=True)
    got = hctx.bootstrap_host(G.MU, *x)
    kern = hctx.last_kernels()
    _stats(hctx, "lds", len(p["dirty"]), kern)
    want = hkey[1].keyswitch_batch(*hkey[1].woks_batch(G.MU, *x, nthreads=NT), nthreads=NT)
    assert _bad_rows(got, want).size == 0
    assert kern == [LDS, GUARD, "k_keyswitch_small"], kern


def test_paired_kernel_and_stale_flags(hctx, hkey, pool, P):
    """cases 2 and 9: NAND, B = CUs + 45 through the paired kernel — an even and an odd slot with a
    clean partner, both slots of a pair, and the last slot beside the padding ciphertext; then, on
    the same context (the flags are never cleared), an all-clean batch of the same shape: nothing
    recomputed; then B = CUs + 44 with its last slot dirty."""
    for name, seed in (("paired", 102), ("paired_clean", 109), ("paired_even", 119)):
        p = P[name]
        x = G.batch(np.random.default_rng(seed), p["B"], p["dirty"], p["real"], pool)
        kern = _nand_host(hctx, hkey[1], x, name, len(p["dirty"]), [PAIRED, GUARD])
        assert kern[:2] == [PAIRED, GUARD], kern


def test_one_ciphertext_reg_rotation(hctx, hkey, pool, P):
    """case 3: NAND, B = 2 CUs + 8, dirty {0, B / 2, B - 1}"""
    p = P["reg"]
    x = G.batch(np.random.default_rng(103), p["B"], p["dirty"], p["real"], pool)
    kern = _nand_host(hctx, hkey[1], x, "reg", len(p["dirty"]), [REG, GUARD])
    assert kern[:2] == [REG, GUARD], kern


def test_chunked_launch_with_a_base(hctx, hkey, pool, P):
    """case 4: tfhe_amd_gate_batch_dev, B = 5 CUs + 3: a launch of 4 CUs, then the paired kernel with
    base = 4 CUs; dirty on both sides of the base, both slots of the first pair behind it, and the
    last slot beside the padding ciphertext"""
    import torch
    p = P["chunked"]
    B = p["B"]
    x = G.batch(np.random.default_rng(104), B, p["dirty"], p["real"], pool)
    ins = G.gate_inputs("NAND", *x)
    d = [torch.from_numpy(v).cuda() for v in ins]
    r_a = torch.empty((B, T.n_lwe), dtype=torch.int32, device="cuda")
    r_b = torch.empty(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hctx.guard_stats(reset=True)
    hctx.gate_dev("NAND", r_a, r_b, *d)
    kern = hctx.last_kernels()
    hctx.sync()
    _stats(hctx, "chunked", len(p["dirty"]), kern)
    want = hkey[1].gate_batch("NAND", *ins, nthreads=NT)
    bad = _bad_rows((r_a.cpu().numpy(), r_b.cpu().numpy()), want)
    assert bad.size == 0, bad[:8]
    assert kern[:3] == [REG, PAIRED, GUARD], kern


def _mux_host(ctx, okey, name, p, seed, pool, want_kern):
    x0, x1 = G.mux_batch(np.random.default_rng(seed), p["B"], p["dirty"], p["real"], pool)
    ins = G.mux_inputs(*x0, *x1)
    ctx.guard_stats(reset=True)
    got = ctx.gate_host("MUX", *ins)
    kern = ctx.last_kernels()
    _stats(ctx, name, len(p["dirty"]), kern)
    want = okey.gate_batch("MUX", *ins, nthreads=NT)
    bad = _bad_rows(got, want)
    assert bad.size == 0, (name, bad[:8])
    assert kern[:len(want_kern)] == want_kern, (name, kern)


def test_mux_halves_small(hctx, hkey, pool, P):
    """case 5: B = 5; half 0 of ciphertext 1, half 1 of ciphertext 3, both halves of ciphertext 4"""
    _mux_host(hctx, hkey[1], "mux_small", P["mux_small"], 105, pool, [LDS, GUARD, "k_keyswitch_small"])


def test_mux_half_boundary_inside_a_pair(hctx, hkey, pool, P):
    """case 6: odd B with CUs < 2 B <= 2 CUs: rotations B - 1 (the last ciphertext's half 0) and B
    (ciphertext 0's half 1) share a workgroup of the paired kernel; one of them dirty, then the other"""
    _mux_host(hctx, hkey[1], "mux_seam_a", P["mux_seam_a"], 106, pool, [PAIRED, GUARD])
    _mux_host(hctx, hkey[1], "mux_seam_b", P["mux_seam_b"], 116, pool, [PAIRED, GUARD])


def test_mux_second_half_crosses_the_base(hctx, hkey, pool, P):
    """case 7: host MUX, B = 2 CUs + 88: 2 B > 4 CUs, the second launch starts inside half 1; one dirty
    sample on each side of the base, in half 1"""
    _mux_host(hctx, hkey[1], "mux_chunked", P["mux_chunked"], 107, pool, [REG, LDS, GUARD])


def test_sliced_host_pipeline(hctx, hkey, pool, P):
    """case 8: gate_host, B = 4 CUs + 40: two slices reuse the same flag slots; slot 3 dirty in slice 0
    and clean in slice 1, slot 20 dirty in slice 1 and clean in slice 0"""
    p = P["sliced"]
    x = G.batch(np.random.default_rng(108), p["B"], p["dirty"], p["real"], pool)
    _nand_host(hctx, hkey[1], x, "sliced", len(p["dirty"]), [REG, LDS, GUARD])


def test_circuit_level_slots(hctx, hkey, pool, P):
    """case 10: a depth-1 circuit of three gate rows on their own input wires, B = 7: dirty (row 0,
    k = 2), (row 1, k = 6), (row 2, k = 0), slot r B + k of the circuit state's own flags; then the
    same level with one more gate behind it that reads row 2's output, whose instances all ran real
    steps: every instance of the new gate has random a, so that level recomputes all B.  The counts are the circuit route's (the
    context's counters, as test_guard_forced_fallback_bit_exact)."""
    import torch
    p = P["circuit"]
    B, gates = p["B"], p["gates"]
    x = G.batch(np.random.default_rng(110), len(gates) * B, [r * B + k for r, k in p["dirty"]],
                [r * B + k for r, k in p["real"]], pool)

    def build(second):
        C = T.Circuit()
        inputs, outs = {}, []
        for r, gate in enumerate(gates):
            wa, wb = C.inputs(2)
            ins = G.gate_inputs(gate, x[0][r * B:(r + 1) * B], x[1][r * B:(r + 1) * B])
            inputs[wa], inputs[wb] = ins[:2], ins[2:]
            outs.append(C.gate(gate, wa, wb))
        if second:
            outs.append(C.gate("NAND", outs[2], wb))   # wb: row 2's second input, the zero sample
        return C, inputs, outs

    def run(C, inputs):
        n_w = C.info()["wires"]
        wa = DA.poisoned((n_w, B, T.n_lwe))      # every wire the run does not write stays poison
        wb = DA.poisoned((n_w, B))
        for w, (e_a, e_b) in inputs.items():
            wa[w] = torch.from_numpy(e_a).cuda()
            wb[w] = torch.from_numpy(e_b).cuda()
        torch.cuda.synchronize()   # the wires are filled on torch's stream, the circuit runs on the context's
        hctx.guard_stats(reset=True)
        C.run_dev(hctx, B, wa, wb)
        kern = hctx.last_kernels()
        hctx.sync()
        return wa.cpu().numpy(), wb.cpu().numpy(), kern

    C2, inputs, outs2 = build(True)
    W = circuit_oracle.eval_circuit(C2, hkey[1], inputs, B, nthreads=NT)
    C1, _, outs1 = build(False)
    assert C1.info()["depth"] == 1 and C2.info()["depth"] == 2
    ha, hb, kern = run(C1, inputs)
    _stats(hctx, "circuit level 1", len(p["dirty"]), kern)
    for w in outs1:
        assert _bad_rows((ha[w], hb[w]), W[w]).size == 0, w
    assert kern[:2] == ROWS and kern[2].startswith("k_keyswitch"), kern
    ha, hb, kern = run(C2, inputs)
    _stats(hctx, "circuit levels 1 + 2", len(p["dirty"]) + B, kern)
    for w in outs2:
        assert _bad_rows((ha[w], hb[w]), W[w]).size == 0, w
    assert kern[:2] == ROWS, kern
    C1.close()
    C2.close()


def test_mixed_host_batch_rows(hctx, hkey, pool, P):
    """case 11: tfhe_amd_gate_batch_mixed_host, gates [NAND, MUX, XOR, MUX] = rows NAND | MUX, MUX |
    XOR | MUX, MUX with B = 1: dirty are the second row of the first MUX and the XOR (every pool
    sample has even words, so the XOR prologue 2 (a + b) + (0, 2^30) inverts for all of them).
    Those are rows 2 and 3; a second batch, [MUX, NAND, XOR, MUX], has the same two dirty rows at
    1 and 3, each with a clean neighbour."""
    for name, seed in (("mixed", 111), ("mixed_b", 121)):
        p = P[name]
        gates = p["gates"]
        n = len(gates)
        x0, x1 = G.mux_batch(np.random.default_rng(seed), n, p["dirty"], p["real"], pool)   # (gate, row of the gate)
        ca, cb, cc = G.zero(n), G.zero(n), G.zero(n)
        for i, gate in enumerate(gates):
            sl = slice(i, i + 1)
            if gate == "MUX":
                ins = G.mux_inputs(x0[0][sl], x0[1][sl], x1[0][sl], x1[1][sl])
            else:
                ins = G.gate_inputs(gate, x0[0][sl], x0[1][sl]) + G.zero(1)
            for dst, k in ((ca, 0), (cb, 2), (cc, 4)):
                dst[0][i], dst[1][i] = ins[k][0], ins[k + 1][0]
        hctx.guard_stats(reset=True)
        got = hctx.gate_mixed_host(gates, *ca, *cb, *cc)
        kern = hctx.last_kernels()
        _stats(hctx, name, len(p["dirty"]), kern)
        for i, gate in enumerate(gates):
            sl = slice(i, i + 1)
            args = [v[sl] for v in ca + cb] + ([v[sl] for v in cc] if gate == "MUX" else [])
            want = hkey[1].gate_batch(gate, *args)
            assert _same((got[0][sl], got[1][sl]), want), (name, i, gate)
        assert kern[:2] == ROWS and kern[2].startswith("k_keyswitch"), kern


def _lut_case(B, seed):
    """one random table per ciphertext, in shuffled order"""
    rng = np.random.default_rng(seed)
    tvs = rng.integers(-2**31, 2**31, (B, G.N), dtype=np.int64).astype(np.int32)
    idx = rng.permutation(B).astype(np.int32)
    return tvs, idx


def test_lut_batch_per_ciphertext_tables(hctx, hkey, cand, P):
    """case 12, single table per ciphertext: tfhe_amd_bootstrap_lut_batch_host, B = 5, dirty {2}; the
    pool is qualified through the raw steps from the dirty ciphertext's own rotated table"""
    p = P["lut"]
    tvs, idx = _lut_case(p["B"], 112)
    ok = _qualify(hctx, hkey[1], cand, "lut", tv=tvs[idx[p["dirty"][0]]])
    x = G.batch(np.random.default_rng(1120), p["B"], p["dirty"], p["real"], ok)
    hctx.guard_stats(reset=True)
    got = hctx.lut_bootstrap_host(tvs, *x, lut_index=idx)
    kern = hctx.last_kernels()
    _stats(hctx, "lut", len(p["dirty"]), kern)
    want = LO.bootstrap_batch(hkey[1], tvs, *x, idx)
    assert _bad_rows(got, want).size == 0
    assert kern[:2] == ["k_blind_rotate_v6(lut+lds-rotation)", "k_blind_rotate_v4(lut+guard)"], kern


def test_lut_many_batch_per_ciphertext_tables(hctx, hkey, cand, P):
    """case 12, many-LUT: tfhe_amd_bootstrap_lut_many_batch_host, (theta, n_out) = (2, 4), B = 5, dirty
    {2}: all four outputs of the dirty ciphertext are the oracle's and it counts once; the pool is
    qualified through the raw steps with the modulus switch to multiples of 4 and the extractions
    at 0 .. 3 (a candidate qualifies when any of its four outputs is wrong)"""
    p = P["lut"]
    theta, n_out = 2, 4
    tvs, idx = _lut_case(p["B"], 113)
    ok = _qualify(hctx, hkey[1], cand, "lut-many 2, 4", tv=tvs[idx[p["dirty"][0]]], theta=theta, n_out=n_out)
    x = G.batch(np.random.default_rng(1130), p["B"], p["dirty"], p["real"], ok)
    hctx.guard_stats(reset=True)
    got = hctx.lut_many_bootstrap_host(tvs, theta, n_out, *x, lut_index=idx)
    kern = hctx.last_kernels()
    _stats(hctx, "lut-many", len(p["dirty"]), kern)
    want = MLO.bootstrap_batch(hkey[1], tvs, *x, theta, n_out, idx)
    assert got[0].shape == want[0].shape == (n_out, p["B"], T.n_lwe)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert kern[:2] == ["k_blind_rotate_v6(lut-many+lds-rotation)", "k_blind_rotate_v4(lut-many+guard)"], kern
