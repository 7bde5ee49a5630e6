"""The HIP path against the reference's OWN functions, directly: every expected value here comes
from tests/golden/ref_hotpath_vectors.npz (the reference's code, compiled and run where the
reference is; tests/ref_fixture.py has the layout), none from the CPU oracle.  Exact equality
throughout; hashed cases compare sha256 and the stored words.

The batched families run once at their own size (a handful of ciphertexts: the latency kernels and
the small-batch key switch) and once tiled by repetition to B = 640 (the register-rotation kernel
and the int8-MFMA key switch, the kernels of the headline batch); every copy must equal the file."""
import numpy as np
import pytest

import dev_arena as DA
import ref_fixture as RF
import tfhe_amd as T

pytestmark = pytest.mark.gpu

G = RF.load()
N, n = RF.N, RF.n_lwe
BIG = 640


def _torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def _host(t):
    return t.cpu().numpy()


def _zeros(shape):
    """an output tensor: every word the constant poison of tests/dev_arena.py, not a plausible 0"""
    _torch()
    return DA.poisoned(shape)


@pytest.fixture(scope="module", autouse=True)
def fixture_key(keyset):
    """the file's outputs belong to this bk / ksk"""
    assert RF.sha(keyset.bk) == str(G["key_bk_sha"]) and RF.sha(keyset.ksk) == str(G["key_ksk_sha"])


def _tiling(C, B):
    """case index of every row of a batch of B made by repeating the C cases"""
    return np.arange(B if B else C) % C


def _all_same(idx, name_a, name_b, got_a, got_b, cases=None):
    """row j of the batch equals case cases[idx[j]] of the file, for every j"""
    C = int(idx.max()) + 1
    cases = np.arange(C) if cases is None else np.asarray(cases)
    got_a, got_b = np.asarray(got_a), np.asarray(got_b)
    assert got_a.shape[0] == len(idx) == got_b.shape[0]
    assert np.array_equal(got_a, got_a[idx]) and np.array_equal(got_b, got_b[idx]), "copies of one case differ"
    for j in range(C):
        assert RF.same(G, name_a, cases[j], got_a[j]) and got_b[j] == G[name_b][cases[j]], (name_a, int(cases[j]))


def _ran(kern, B, rotation=True, keyswitch=True):
    """the kernel set the batch size is meant to take really ran"""
    if rotation:
        want = "reg-rotation" if B else "lds-rotation"
        assert any(want in k and "paired" not in k for k in kern), (want, kern)
    if keyswitch:
        assert any(k.startswith("k_keyswitch_v5(int8-mfma") for k in kern) if B else "k_keyswitch_small" in kern, kern


def test_cmux_chains_both_generations(ctx):
    """tfhe_blindRotate over key rows 0 .. 7 (rotation edges, skipped steps, saturated digits)
    through blind_rotate_dev, under the exact-NTT and the fp64-FFT generation"""
    acc0, bara = G["cm_acc"], G["cm_bara"]
    default = T.version()
    kern = {}
    got = {}
    try:
        for v in (4, 6):
            T.select_kernel(v)
            d_acc = _dev(acc0)
            ctx.blind_rotate_dev(d_acc, _dev(bara), bara.shape[1])
            kern[v] = ctx.last_kernels()
            ctx.sync()
            got[v] = _host(d_acc)
    finally:
        tag = default.split("br-v")[1].split(" ")[0]
        T.select_kernel(int(tag) if tag.isdigit() else 0)
    for v in (4, 6):
        for i in range(len(bara)):
            assert RF.same(G, "cm_out", i, got[v][i]), (v, i)
    assert all("v4" in k for k in kern[4]) and any("v6" in k for k in kern[6]), kern


def test_external_products(ctx, keyset):
    """tGswExternMulToTLwe on the key's own rows (random and digit-saturating accumulators)
    through tgsw_cmux_dev with d0 = None"""
    kset = ctx.tgsw_import(keyset.bk[:8])
    try:
        out = _zeros((len(G["xp_row"]), 2, N))
        ctx.tgsw_cmux_dev(kset, _dev(G["xp_row"]), _dev(G["xp_acc"]), None, out)
        ctx.sync()
        got = _host(out)
    finally:
        kset.close()
    for i in range(len(G["xp_row"])):
        assert RF.same(G, "xp_out", i, got[i]), i


@pytest.mark.parametrize("B", [0, BIG], ids=["own-size", "B640"])
def test_woks_keyswitch_bootstrap(ctx, B):
    x_a, x_b = G["bs_x_a"], G["bs_x_b"]
    idx = _tiling(len(x_b), B)
    u_a, u_b = ctx.woks_host(RF.MU, x_a[idx], x_b[idx])
    _ran(ctx.last_kernels(), B, keyswitch=False)
    _all_same(idx, "bs_woks_a", "bs_woks_b", u_a, u_b)
    r_a, r_b = ctx.bootstrap_host(RF.MU, x_a[idx], x_b[idx])
    _ran(ctx.last_kernels(), B)
    _all_same(idx, "bs_full_a", "bs_full_b", r_a, r_b)
    kdx = _tiling(len(G["ks_u_b"]), B)
    k_a, k_b = ctx.keyswitch_host(G["ks_u_a"][kdx], G["ks_u_b"][kdx])
    _ran(ctx.last_kernels(), B, rotation=False)
    _all_same(kdx, "ks_out_a", "ks_out_b", k_a, k_b)


@pytest.mark.parametrize("B", [0, BIG], ids=["own-size", "B640"])
@pytest.mark.parametrize("code", [RF.NAND, RF.XOR, RF.MUX], ids=["NAND", "XOR", "MUX"])
def test_gates(ctx, code, B):
    cases = np.flatnonzero(G["gate_code"] == code)
    idx = _tiling(len(cases), B)
    a, b = G["gate_in_a"][cases][idx], G["gate_in_b"][cases][idx]
    ins = sum(((a[:, k], b[:, k]) for k in range(3 if code == RF.MUX else 2)), ())
    r_a, r_b = ctx.gate_host(RF.GATE_NAME[code], *(np.ascontiguousarray(v) for v in ins))
    _ran(ctx.last_kernels(), B)
    _all_same(idx, "gate_out_a", "gate_out_b", r_a, r_b, cases)


def test_blind_rotate_and_extract_with_test_vectors(ctx):
    """tfhe_blindRotateAndExtract with the constant and the table test vector, barb = 0 and != 0,
    through lut_woks_host; the constant cases also through woks_host"""
    x_a, x_b, which = G["bre_x_a"], G["bre_x_b"], G["bre_tv"]
    u_a, u_b = ctx.lut_woks_host(G["bre_tvs"], x_a, x_b, lut_index=which)
    _all_same(np.arange(len(which)), "bre_out_a", "bre_out_b", u_a, u_b)
    const = np.flatnonzero(which == 0)
    u_a, u_b = ctx.woks_host(RF.MU, x_a[const], x_b[const])
    _all_same(np.arange(len(const)), "bre_out_a", "bre_out_b", u_a, u_b, const)


def test_extraction_at_indices(ctx):
    """tLweExtractLweSampleIndex at 0, 1 and 15 of one blind rotation, through lut_many_woks_host
    (log_nu = 4, 16 outputs; the table's 128 words are all different)"""
    u_a, u_b = ctx.lut_many_woks_host(G["ml_tv"], 4, 16, G["ml_x_a"][None], G["ml_x_b"].reshape(1))
    assert u_a.shape == (16, 1, N)
    for i, f in enumerate(G["ml_index"]):
        assert RF.same(G, "ml_out_a", i, u_a[f, 0]) and u_b[f, 0] == G["ml_out_b"][i], f
