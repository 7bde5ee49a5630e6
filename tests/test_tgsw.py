"""Leveled table lookup, the parts that need no GPU: the client-side encryptions
(tfhe_amd_tgsw_encrypt_bits, tfhe_amd_tlwe_encrypt_polys), the oracle composition of
tests/tgsw_oracle.py on the library's own encryptions, and the argument checks of the device
entry points that return before they touch a device."""
import ctypes

import numpy as np
import pytest

import tfhe_amd as T
import tgsw_oracle as TO

N, n_lwe = 1024, 500
E_ARG = -1
SIGMA = 7.180961047225788e-09 * 2.0**32    # the TGSW key's alpha_min in Torus32 units (params.h kBkStdev)
H = (1 << 22, 1 << 12)                      # gadget values h[l] = 2^(32 - 10 (l + 1))
E8 = 1 << 29


def _seed(*values):
    s = (ctypes.c_uint32 * len(values))(*values)
    T.lib.tfhe_random_generator_setSeed(s, len(values))


def test_tgsw_rows_are_zero_encryptions_plus_the_gadget(keyset):
    """every row's phase under the exported TLWE key is within 6 sigma of 0 (bit 0) or of the
    gadget value: -bit h[l] s(X) in the mask rows (bloc 0), bit h[l] at coefficient 0 in the body
    rows (bloc 1); the layout [n][4 rows][a, b][1024] of one bootstrapping-key entry"""
    _seed(11, 22)
    bits = np.array([0, 1, 1, 0, 1], np.int32)
    g = keyset.tgsw_encrypt(bits)
    assert g.shape == (5, 4, 2, N) and g.dtype == np.int32
    s = keyset.tlwe_key.astype(np.int64)
    for i, bit in enumerate(bits):
        for bloc in range(2):
            for l in range(2):
                row = g[i, bloc * 2 + l]
                want = np.zeros(N, np.int64)
                if bloc == 0:
                    want -= int(bit) * H[l] * s
                else:
                    want[0] = int(bit) * H[l]
                err = TO.wrap(TO.tlwe_phase(keyset.tlwe_key, row[0], row[1]).astype(np.int64) - want)
                assert np.abs(err).max() < 6 * SIGMA, (i, bloc, l, np.abs(err).max())
                assert np.abs(err).max() > 0          # a fresh encryption, not the bare gadget


def test_tlwe_polys_encrypt_their_message(keyset, rng):
    _seed(33)
    mu = rng.integers(-2**31, 2**31, (3, N), dtype=np.int64).astype(np.int32)
    c = keyset.tlwe_encrypt(mu)
    assert c.shape == (3, 2, N)
    for i in range(3):
        err = TO.wrap(TO.tlwe_phase(keyset.tlwe_key, c[i, 0], c[i, 1]).astype(np.int64) - mu[i])
        assert 0 < np.abs(err).max() < 6 * SIGMA
    one = keyset.tlwe_encrypt(mu[0])
    assert one.shape == (1, 2, N)


def test_oracle_cmux_on_library_samples_selects_the_branch(keyset, rng):
    """the layout is the bootstrapping key's: the oracle's external product, run on the library's
    TGSW samples in a key's place, selects d1 under a 1 and d0 under a 0"""
    _seed(44)
    g = keyset.tgsw_encrypt([0, 1])
    m = (rng.integers(0, 2, (2, N)) * 2 - 1) * E8
    d = keyset.tlwe_encrypt(m)
    ok = TO.key(g, keyset.ksk)
    for i in (0, 1):
        out = TO.cmux(ok, i, d[1], d[0])
        err = TO.wrap(TO.tlwe_phase(keyset.tlwe_key, out[0], out[1]).astype(np.int64) - m[i])
        assert np.abs(err).max() < 2**32 / 64, (i, np.abs(err).max())
        assert not np.array_equal(out, d[i])          # a product, not a copy
    # the external product alone: C (x) d1 encrypts bit * m1
    out = TO.cmux(ok, 0, d[1])
    assert np.abs(TO.tlwe_phase(keyset.tlwe_key, out[0], out[1])).max() < 2**32 / 64


def test_encryptions_are_deterministic_under_the_seed(keyset):
    mu = np.arange(2 * N, dtype=np.int32).reshape(2, N)
    runs = []
    for _ in range(2):
        _seed(5, 6, 7)
        runs.append((keyset.tgsw_encrypt([1, 0, 1]), keyset.tlwe_encrypt(mu)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    _seed(5, 6, 8)
    assert not np.array_equal(keyset.tgsw_encrypt([1, 0, 1]), runs[0][0])


def test_encrypt_argument_errors(keyset):
    L = T.lib
    bits = np.array([0, 1], np.int32)
    out = np.zeros((2, 4, 2, N), np.int32)
    p = T._p
    assert L.tfhe_amd_tgsw_encrypt_bits(None, 2, p(bits), p(out)) == E_ARG
    assert L.tfhe_amd_tgsw_encrypt_bits(keyset.h, -1, p(bits), p(out)) == E_ARG
    assert L.tfhe_amd_tgsw_encrypt_bits(keyset.h, 2, None, p(out)) == E_ARG
    assert L.tfhe_amd_tgsw_encrypt_bits(keyset.h, 2, p(bits), None) == E_ARG
    for bad in (2, -1):
        assert L.tfhe_amd_tgsw_encrypt_bits(keyset.h, 2, p(np.array([1, bad], np.int32)), p(out)) == E_ARG
    assert not out.any()                              # refused before anything is written
    assert L.tfhe_amd_tgsw_encrypt_bits(keyset.h, 0, p(bits), p(out)) == 0
    mu = np.zeros((1, N), np.int32)
    o2 = np.zeros((1, 2, N), np.int32)
    assert L.tfhe_amd_tlwe_encrypt_polys(None, 1, p(mu), p(o2)) == E_ARG
    assert L.tfhe_amd_tlwe_encrypt_polys(keyset.h, -1, p(mu), p(o2)) == E_ARG
    assert L.tfhe_amd_tlwe_encrypt_polys(keyset.h, 1, None, p(o2)) == E_ARG
    assert L.tfhe_amd_tlwe_encrypt_polys(keyset.h, 1, p(mu), None) == E_ARG
    with pytest.raises(T.TfheAmdError):
        keyset.tgsw_encrypt([0, 3])


def _pool(keyset, seed, count=24):
    """a pool of `count` TGSW samples on random bits (both values present), shared by the queries"""
    _seed(seed)
    bits = np.random.default_rng(seed).integers(0, 2, count).astype(np.int32)
    bits[:2] = (0, 1)
    return bits, keyset.tgsw_encrypt(bits)


def _report(name, keyset, u, want):
    """the phase error of the extracted samples against the expected torus values: printed (DESIGN.md
    §3.6 records it), asserted below 1/64"""
    err = TO.wrap(keyset.phase_extracted(u[0].reshape(-1, N), u[1].reshape(-1)).astype(np.int64) -
                  np.asarray(want, dtype=np.int64).reshape(-1)).astype(np.float64) / 2.0**32
    print(f"{name}: {err.size} samples, largest error {np.abs(err).max():.5f}, r.m.s. {np.sqrt(np.mean(err**2)):.5f}")
    assert np.abs(err).max() < 1.0 / 64
    return err


def test_lookup_d10_every_query_decodes(keyset, capsys):
    """a 1024-entry +-1/8 table, d = 10 TGSW address bits, stride 1: all 24 queries decode after the
    key switch, none left out; the error before the key switch is printed and stays below 1/64"""
    rng = np.random.default_rng(1010)
    bits, g = _pool(keyset, 1010)
    ok = TO.key(g, keyset.ksk)
    table = (rng.integers(0, 2, N) * 2 - 1) * E8
    addr = np.concatenate([[0, 1, N - 1, N // 2], rng.integers(0, N, 20)])
    B, d = addr.shape[0], 10
    want_bits = (addr[:, None] >> np.arange(d)) & 1
    sel = TO.pick(rng, bits, want_bits)
    tab = table.astype(np.int32).reshape(1, 1, 1, N)
    u = TO.lookup_woks(ok, sel, tab)
    assert u[0].shape == (1, B, N)
    with capsys.disabled():
        _report("tgsw lookup d=10 stride 1 (before the key switch)", keyset, u, table[addr])
    r_a, r_b = TO.MO.keyswitch(ok, u)
    assert np.array_equal(keyset.decrypt(r_a[0], r_b[0]), (table[addr] > 0).astype(np.int32))


def test_lookup_d7_stride8_every_output_decodes(keyset, capsys):
    """a 128 x 8-bit table, one bit per word at stride 8, n_out = 8: all 8 x 8 outputs decode"""
    rng = np.random.default_rng(707)
    bits, g = _pool(keyset, 707)
    ok = TO.key(g, keyset.ksk)
    table = (rng.integers(0, 2, N) * 2 - 1) * E8
    addr = np.concatenate([[0, 127], rng.integers(0, 128, 6)])
    B, d = addr.shape[0], 7
    sel = TO.pick(rng, bits, (addr[:, None] >> np.arange(d)) & 1)
    u = TO.lookup_woks(ok, sel, table.astype(np.int32).reshape(1, 1, 1, N), log_stride=3, n_out=8)
    want = np.stack([table[addr * 8 + f] for f in range(8)])          # [n_out][B]
    with capsys.disabled():
        _report("tgsw lookup d=7 stride 8 n_out=8 (before the key switch)", keyset, u, want)
    r_a, r_b = TO.MO.keyswitch(ok, u)
    assert r_a.shape == (8, B, n_lwe)
    assert np.array_equal(keyset.decrypt(r_a.reshape(-1, n_lwe), r_b.reshape(-1)),
                          (want.reshape(-1) > 0).astype(np.int32))


def test_lookup_tree_over_encrypted_polynomials_decodes(keyset, capsys):
    """vertical packing: 8 TLWE-encrypted polynomials, a depth-3 CMux tree on the address bits
    d_h .. d - 1, then d_h = 2 rotation steps at stride 1"""
    rng = np.random.default_rng(303)
    bits, g = _pool(keyset, 303)
    ok = TO.key(g, keyset.ksk)
    _seed(304)
    polys = (rng.integers(0, 2, (8, N)) * 2 - 1) * E8
    tab = keyset.tlwe_encrypt(polys).reshape(1, 8, 2, N)
    addr = np.concatenate([[0, 31], rng.integers(0, 32, 6)])
    sel = TO.pick(rng, bits, (addr[:, None] >> np.arange(5)) & 1)
    u = TO.lookup_woks(ok, sel, tab)
    want = polys[addr >> 2, addr & 3]
    with capsys.disabled():
        _report("tgsw lookup depth-3 tree + d_h=2 (before the key switch)", keyset, u, want)
    r_a, r_b = TO.MO.keyswitch(ok, u)
    assert np.array_equal(keyset.decrypt(r_a[0], r_b[0]), (want > 0).astype(np.int32))


def test_device_entry_points_refuse_bad_arguments_without_a_device():
    """every new entry point returns TFHE_AMD_E_ARG for a null context or set before it touches a
    device; count and destroy take NULL"""
    L = T.lib
    buf = np.zeros(4 * 2 * N, np.int32)
    p = buf.ctypes.data
    h = ctypes.c_void_p(1234)
    assert L.tfhe_amd_tgsw_count(None) == E_ARG
    assert L.tfhe_amd_tgsw_destroy(None) == 0
    assert L.tfhe_amd_tgsw_import(None, 1, T._p(buf), ctypes.byref(h)) == E_ARG and h.value is None
    assert L.tfhe_amd_tgsw_cmux_dev(None, None, 1, p, p, p, p, None) == E_ARG
    for f in ("tfhe_amd_tgsw_lookup_woks_dev", "tfhe_amd_tgsw_lookup_dev"):
        assert getattr(L, f)(None, None, 1, 1, p, 1, 1, 1, p, None, 0, 1, p, p, None) == E_ARG
    for f in ("tfhe_amd_tgsw_lookup_woks_host", "tfhe_amd_tgsw_lookup_host"):
        assert getattr(L, f)(None, None, 1, 1, T._p(buf), 1, 1, 1, T._p(buf), None, 0, 1, T._p(buf), T._p(buf)) == E_ARG
