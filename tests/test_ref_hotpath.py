"""The oracle's hot path pinned against the reference's OWN functions (CPU, no GPU).

tests/golden/ref_hotpath_vectors.npz was produced by tests/golden/make_golden.py from
oracle/_ref/libtfheref.so: the reference's rotations, decomposition, sample extraction, key switch,
external product, CMux, blind rotation and bootstraps, cut out of gpuParallel/*.cu by name
(oracle/extract_ref.py) and compiled unmodified, with its exact Karatsuba product in the place of
the FFT one.  Every comparison is exact equality; hashed cases compare sha256 and the stored words."""
import ctypes
import os

import numpy as np
import pytest

import lut_oracle as LO
import many_lut_oracle as MO
import oracle_ctypes as O
import ref_fixture as RF
import tgsw_oracle as TO

G = RF.load()
N, n = RF.N, RF.n_lwe


@pytest.fixture(scope="module", params=[1, 0], ids=["ntt", "schoolbook"])
def key(request, keyset):
    """the oracle over the seeded keyset, on both product routes"""
    return O.OracleKey(keyset.bk, keyset.ksk, use_ntt=bool(request.param))


def test_seeded_keyset_is_the_fixtures_key(keyset):
    """the fixture's outputs were computed under this bk / ksk: a keygen that drifts fails here"""
    assert RF.sha(keyset.bk) == str(G["key_bk_sha"])
    assert RF.sha(keyset.ksk) == str(G["key_ksk_sha"])


def test_fixture_covers_what_it_claims():
    a = set(int(v) for v in G["rot_a"])
    assert {0, 1, N - 1, N, N + 1, 2 * N - 1} <= a and max(a) < 2 * N and len(a) > 8
    for name in ("rot_xai", "rot_xai_m1", "dec_out", "ext_out_a", "ks_out_a", "xp_out", "cm_out", "bre_out_a",
                 "bs_woks_a", "bs_full_a", "gate_out_a"):
        assert RF.full(G, name) >= 4, name
    assert list(G["ext_index"]) == [0, 1, 15, N - 1] and list(G["ml_index"]) == [0, 1, 15]
    assert not G["ks_u_a"][4].any()
    aibar = (G["ks_u_a"][5].astype(np.int64) + (1 << 15)) & 0xFFFFFFFF
    assert (aibar >> 16 == 0xFFFF).all()
    d = G["dec_out"]
    assert d.min() == -512 and d.max() == 511
    assert (O.decompose(G["xp_acc"][2][0]) == -512).all() and (O.decompose(G["xp_acc"][3][1]) == 511).all()
    step = np.stack([O.mul_by_xai_minus_one(N, G["cm_acc"][4][c]) for c in range(2)])
    assert (O.decompose(step[0]) == -512).all() and (O.decompose(step[1]) == 511).all()
    assert list(G["cm_bara"][0]) == [0, 1, N - 1, N, N + 1, 2 * N - 1, 5, 0] and not G["cm_bara"][1, :4].any()
    assert G["cm_bara"].min() >= 0 and G["cm_bara"].max() < 2 * N
    assert list(G["bre_barb"] == 0) == [True, False, True, False] and list(G["bre_tv"]) == [0, 0, 1, 1]
    assert len(set(G["bre_tvs"][0])) == 1 and len(set(G["bre_tvs"][1])) == 8
    assert G["bs_x_b"][3] == -2**20 + 5 and not G["bs_x_a"][4, :25].any() and (G["bs_x_a"][4, 25:50] == -2**20).all()
    assert sorted(G["gate_code"]) == [RF.NAND] * 4 + [RF.XOR] * 4 + [RF.MUX] * 2
    assert os.path.getsize(RF.PATH) < 1000000


def test_rotations_match_reference():
    x = G["rot_in"]
    for i, a in enumerate(G["rot_a"]):
        assert RF.same(G, "rot_xai", i, O.mul_by_xai(a, x)), a
        assert RF.same(G, "rot_xai_m1", i, O.mul_by_xai_minus_one(a, x)), a


def test_decomposition_matches_reference():
    for i, x in enumerate(G["dec_in"]):
        assert RF.same(G, "dec_out", i, O.decompose(x)), i


def test_extraction_matches_reference():
    """lwe.cu:41-56 at an index == many_lut_oracle.extract (numpy), and at index 0 the extraction
    the C oracle's woKS bootstrap ends with (checked through the bootstrap cases below)"""
    acc = G["ext_acc"]
    for i, f in enumerate(G["ext_index"]):
        u_a, u_b = MO.extract(acc[0], acc[1], int(f))
        assert RF.same(G, "ext_out_a", i, u_a) and u_b == G["ext_out_b"][i], f


def test_keyswitch_matches_reference(key):
    for i in range(len(G["ks_u_b"])):
        r_a, r_b = key.keyswitch(G["ks_u_a"][i], G["ks_u_b"][i])
        assert RF.same(G, "ks_out_a", i, r_a) and r_b == G["ks_out_b"][i], i


def test_external_product_matches_reference(key, keyset):
    """tGswExternMulToTLwe == orc_external_product == tgsw_oracle.cmux on the key's own rows"""
    for i, row in enumerate(G["xp_row"]):
        assert RF.same(G, "xp_out", i, key.external_product(G["xp_acc"][i], int(row))), i
    for use_ntt in (True, False):
        tk = TO.key(keyset.bk[:8], keyset.ksk, use_ntt=use_ntt)
        for i, row in enumerate(G["xp_row"]):
            assert RF.same(G, "xp_out", i, TO.cmux(tk, int(row), G["xp_acc"][i])), (use_ntt, i)


def test_cmux_chain_matches_reference(key):
    """tfhe_blindRotate over key rows 0 .. 7 == orc_mux_rotate step by step == orc_blind_rotate"""
    for i in range(len(G["cm_bara"])):
        acc = G["cm_acc"][i].copy()
        for step, a in enumerate(G["cm_bara"][i]):
            if a != 0:
                acc = key.mux_rotate(acc, step, int(a))
        assert RF.same(G, "cm_out", i, acc), i
        acc = np.ascontiguousarray(G["cm_acc"][i]).reshape(2 * N).copy()
        O.lib().orc_blind_rotate(O._p(acc), ctypes.c_void_p(key.h), O._p(np.ascontiguousarray(G["cm_bara"][i])), 8)
        assert RF.same(G, "cm_out", i, acc.reshape(2, N)), i


def test_blind_rotate_and_extract_matches_reference(key):
    """tfhe_blindRotateAndExtract with a caller's test vector == lut_oracle.woks_one; with the
    constant one also == orc_bootstrap_woKS.  bara / barb of the file are the oracle's modswitch."""
    for i in range(len(G["bre_tv"])):
        x_a, x_b, tv = G["bre_x_a"][i], int(G["bre_x_b"][i]), G["bre_tvs"][G["bre_tv"][i]]
        assert np.array_equal(LO.modswitch_2n(x_a), G["bre_bara"][i]) and O.modswitch_from(x_b, 2 * N) == G["bre_barb"][i]
        u_a, u_b = LO.woks_one(key, tv, x_a, x_b)
        assert RF.same(G, "bre_out_a", i, u_a) and u_b == G["bre_out_b"][i], i
        if G["bre_tv"][i] == 0:
            u_a, u_b = key.bootstrap_woks(RF.MU, x_a, x_b)
            assert RF.same(G, "bre_out_a", i, u_a) and u_b == G["bre_out_b"][i], i


def test_many_lut_extraction_matches_reference(key):
    """one blind rotation at log_nu = 4, extracted at 0, 1 and 15 == many_lut_oracle.woks_one"""
    u_a, u_b = MO.woks_one(key, G["ml_tv"], G["ml_x_a"], int(G["ml_x_b"]), 4, 16)
    for i, f in enumerate(G["ml_index"]):
        assert RF.same(G, "ml_out_a", i, u_a[f]) and u_b[f] == G["ml_out_b"][i], f
    assert len({RF.sha(u_a[f]) for f in (0, 1, 15)}) == 3


def test_bootstraps_match_reference(key):
    x_a, x_b = G["bs_x_a"], G["bs_x_b"]
    u_a, u_b = key.woks_batch(RF.MU, x_a, x_b)
    lib = O.lib()
    for i in range(len(x_b)):
        assert RF.same(G, "bs_woks_a", i, u_a[i]) and u_b[i] == G["bs_woks_b"][i], i
        r_a = np.zeros(n, np.int32)
        r_b = ctypes.c_int32(0)
        lib.orc_bootstrap(O._p(r_a), ctypes.byref(r_b), ctypes.c_void_p(key.h), ctypes.c_int32(RF.MU),
                          O._p(np.ascontiguousarray(x_a[i])), ctypes.c_int32(int(x_b[i])))
        assert RF.same(G, "bs_full_a", i, r_a) and r_b.value == G["bs_full_b"][i], i


def test_gates_match_reference(key, keyset):
    """boot-gates.cu's NAND / XOR / MUX composed from the reference's LWE ops and its bootstrap"""
    code, a, b = G["gate_code"], G["gate_in_a"], G["gate_in_b"]
    for c in (RF.NAND, RF.XOR, RF.MUX):
        sel = np.flatnonzero(code == c)
        ins = sum(((a[sel, k], b[sel, k]) for k in range(3 if c == RF.MUX else 2)), ())
        r_a, r_b = key.gate_batch(RF.GATE_NAME[c], *(np.ascontiguousarray(v) for v in ins))
        for j, i in enumerate(sel):
            assert RF.same(G, "gate_out_a", i, r_a[j]) and r_b[j] == G["gate_out_b"][i], i
        x, y, z = (G["gate_bits"][sel, k] for k in range(3))
        truth = {RF.NAND: 1 - (x & y), RF.XOR: x ^ y, RF.MUX: np.where(x == 1, y, z)}[c]
        assert np.array_equal(keyset.decrypt(G["gate_out_a"][sel], G["gate_out_b"][sel]), truth), c


def test_fixture_is_fresh(keyset):
    """recompute the component families and one woKS bootstrap from the reference's compiled code:
    a fixture that no longer matches the recipe (or the reference) fails here.  Skips only where
    the library is absent: the reference is not on this machine, or what oracle/_ref/ holds was
    built without the hot-path functions and cannot be rebuilt for the same reason."""
    if not RF.ref_library():
        pytest.skip("oracle/_ref/libtfheref.so with the hot-path functions absent (the reference is not on this machine)")
    R = RF.Ref(keyset.bk, keyset.ksk)
    try:
        for i, a in enumerate(G["rot_a"]):
            assert RF.same(G, "rot_xai", i, R.mul_by_xai(a, G["rot_in"]))
            assert RF.same(G, "rot_xai_m1", i, R.mul_by_xai(a, G["rot_in"], minus_one=True))
        avx2 = ctypes.CDLL(RF.REF_AVX2_SO)
        for i, x in enumerate(G["dec_in"]):
            assert RF.same(G, "dec_out", i, R.decompose(x)) and RF.same(G, "dec_out", i, RF.decompose(avx2, x))
        for i, f in enumerate(G["ext_index"]):
            u_a, u_b = R.extract(G["ext_acc"], f)
            assert RF.same(G, "ext_out_a", i, u_a) and u_b == G["ext_out_b"][i]
        for i in range(len(G["ks_u_b"])):
            r_a, r_b = R.keyswitch(G["ks_u_a"][i], G["ks_u_b"][i])
            assert RF.same(G, "ks_out_a", i, r_a) and r_b == G["ks_out_b"][i]
        for i, row in enumerate(G["xp_row"]):
            assert RF.same(G, "xp_out", i, R.external_product(G["xp_acc"][i], row))
        for i in range(len(G["cm_bara"])):
            assert RF.same(G, "cm_out", i, R.blind_rotate(G["cm_acc"][i], G["cm_bara"][i]))
            acc = G["cm_acc"][i]
            for step, a in enumerate(G["cm_bara"][i]):
                if a != 0:
                    acc = R.mux_rotate(acc, step, a)
            assert RF.same(G, "cm_out", i, acc)
        u_a, u_b = R.bootstrap_woks(RF.MU, G["bs_x_a"][3], G["bs_x_b"][3])
        assert RF.same(G, "bs_woks_a", 3, u_a) and u_b == G["bs_woks_b"][3]
    finally:
        R.close()
