"""Packing key switch, host side: the oracle's two routes against each other, the
digit decomposition, the generated key and the client's phase function.  No GPU."""
import ctypes

import numpy as np
import pytest

import pack_oracle as PO
import tfhe_amd as T
import tgsw_oracle as TO

N, n_lwe = 1024, 500
E_ARG = -1


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _seed(a, b):
    T.lib.tfhe_random_generator_setSeed((ctypes.c_uint32 * 2)(a, b), 2)


@pytest.fixture(scope="module")
def pack_key(keyset):
    _seed(37, 1)
    return keyset.pack_key()


@pytest.mark.parametrize("pos", [[0], [1023], [0, 1, 511, 512, 1023]])
def test_oracle_routes_agree(pos):
    """row by row through the oracle's exact polynomial product == input by input through an integer
    matrix product, on random words as key and inputs; two outputs per case"""
    rng = np.random.default_rng(len(pos) + pos[0])
    key = _rand32(rng, (n_lwe, 6, 2, N))
    P = len(pos)
    in_a, in_b = _rand32(rng, (2, P, n_lwe)), _rand32(rng, (2, P))
    a = PO.pack_rows(key, in_a, in_b, pos)
    assert a.shape == (2, 2, N) and a.dtype == np.int32
    assert np.array_equal(a, PO.pack_inputs(key, in_a, in_b, pos))
    # pos = None is pos[p] = p; a position outside [0, 1024) drops its input in both routes
    if P == 5:
        assert np.array_equal(PO.pack_rows(key, in_a, in_b), PO.pack_inputs(key, in_a, in_b, np.arange(5)))
        bad = np.array([0, -1, 511, 1024, 1 << 30])
        keep = [0, 2]
        want = PO.pack_inputs(key, in_a[:, keep], in_b[:, keep], bad[keep])
        assert np.array_equal(PO.pack_rows(key, in_a, in_b, bad), want)
        assert np.array_equal(PO.pack_inputs(key, in_a, in_b, bad), want)


def test_decomposition_identity():
    """sum_j d_j 2^(32 - 4 j) is within 2^7 of the word, digits in [-8, 7], zero has zero digits"""
    rng = np.random.default_rng(4)
    edge = np.array([0, 1, -1, 0x77777800, 0x77777777, 2**31 - 1, -2**31, 0x777777FF, 0x77777780, 0x7777777F - 2**32])
    words = np.concatenate([edge, rng.integers(-2**31, 2**31, 100000)]).astype(np.int64)
    d = PO.digits(words)
    assert d.shape == (words.shape[0], 6) and d.min() >= -8 and d.max() <= 7
    approx = sum(d[:, j - 1] << (32 - 4 * j) for j in range(1, 7))
    err = ((approx - words + 2**31) % 2**32) - 2**31       # centred mod 2^32
    assert np.abs(err).max() <= 2**7
    assert not d[0].any()
    assert np.array_equal(d[3], [-8] * 6)                   # 0x77777800: every digit -8
    assert np.array_equal(PO.digits(np.int64(0x77777700)), [7] * 6)   # every digit +7
    assert T.PACK_T == PO.T_DIG


def test_key_rows_encrypt_the_key_bits(keyset, pack_key):
    """row (i, j): phase s_i 2^(32 - 4 j) at coefficient 0 and 0 elsewhere, within 8 sigma_bk"""
    assert pack_key.shape == (n_lwe, 6, 2, N) and pack_key.dtype == np.int32
    ph = keyset.tlwe_phase(pack_key.reshape(-1, 2, N)).astype(np.int64).reshape(n_lwe, 6, N)
    want = np.zeros((n_lwe, 6, N), np.int64)
    for j in range(1, 7):
        want[:, j - 1, 0] = keyset.lwe_key.astype(np.int64) << (32 - 4 * j)
    err = ((ph - want + 2**31) % 2**32) - 2**31
    bound = 8 * PO.SIGMA_BK * 2**32
    assert np.abs(err).max() <= bound, (np.abs(err).max(), bound)
    rms = np.sqrt(np.mean(err.astype(np.float64) ** 2)) / 2**32
    assert 0.9 * PO.SIGMA_BK < rms < 1.1 * PO.SIGMA_BK, rms
    assert keyset.lwe_key.any() and not keyset.lwe_key.all()


def test_generation_is_reproducible_from_a_seed(keyset, pack_key):
    _seed(37, 1)
    again = keyset.pack_key()
    assert again.tobytes() == pack_key.tobytes()
    _seed(37, 2)
    other = np.zeros((n_lwe, 6, 2, N), np.int32)
    assert T.lib.tfhe_amd_pack_key_generate(keyset.h, T._p(other)) == 0
    assert other.tobytes() != pack_key.tobytes()


def test_tlwe_phase_equals_the_numpy_oracle(keyset):
    rng = np.random.default_rng(11)
    x = _rand32(rng, (3, 2, N))
    x[2] = [np.full(N, -2**31), np.full(N, 2**31 - 1)]
    got = keyset.tlwe_phase(x)
    assert got.shape == (3, N)
    for k in range(3):
        assert np.array_equal(got[k], TO.tlwe_phase(keyset.tlwe_key, x[k, 0], x[k, 1])), k
    assert np.array_equal(keyset.tlwe_phase(x[1]), got[1:2])
    # a fresh encryption decrypts to its message
    mu = _rand32(rng, (1, N))
    err = (keyset.tlwe_phase(keyset.tlwe_encrypt(mu)).astype(np.int64) - mu + 2**31) % 2**32 - 2**31
    assert np.abs(err).max() <= 8 * PO.SIGMA_BK * 2**32


def test_host_only_argument_refusals(keyset):
    lib, p = T.lib, T._p
    key = np.zeros((n_lwe, 6, 2, N), np.int32)
    x, ph = np.zeros((1, 2, N), np.int32), np.zeros((1, N), np.int32)
    assert lib.tfhe_amd_pack_key_generate(None, p(key)) == E_ARG
    assert lib.tfhe_amd_pack_key_generate(keyset.h, None) == E_ARG
    assert not key.any()
    assert lib.tfhe_amd_tlwe_phase_polys(None, 1, p(x), p(ph)) == E_ARG
    assert lib.tfhe_amd_tlwe_phase_polys(keyset.h, -1, p(x), p(ph)) == E_ARG
    assert lib.tfhe_amd_tlwe_phase_polys(keyset.h, 1, None, p(ph)) == E_ARG
    assert lib.tfhe_amd_tlwe_phase_polys(keyset.h, 1, p(x), None) == E_ARG
    assert lib.tfhe_amd_tlwe_phase_polys(keyset.h, 0, p(x), p(ph)) == 0
    # the device entry points refuse null handles before they touch a device
    assert lib.tfhe_amd_pack_key_import(None, p(key), ctypes.byref(ctypes.c_void_p())) == E_ARG
    assert lib.tfhe_amd_pack_host(None, None, 1, 1, p(x), p(x), None, p(x)) == E_ARG
    assert lib.tfhe_amd_pack_dev(None, None, 1, 1, None, None, None, None, None) == E_ARG
    assert lib.tfhe_amd_pack_key_destroy(None) == 0
