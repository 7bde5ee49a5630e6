"""Bootstrap from encrypted accumulators, host side: the oracle of tests/acc_oracle.py
against second routes, the argument rules that need no GPU, and the measurements the design quotes —
the decode chain of a bootstrapped 2-bit selector reading bootstrapped candidates, and the noise of
the box-filled pack.  No GPU."""
import numpy as np
import pytest

import acc_oracle as AO
import lut_oracle as LO
import oracle_ctypes as O
import pack_oracle as PO
import tfhe_amd as T

N, n_lwe = 1024, 500
E_ARG = -1


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _centred(d):
    return (np.asarray(d).astype(np.int64) + 2**31) % 2**32 - 2**31


@pytest.mark.parametrize("log_w", [0, 1, 8, 10])
def test_box_fill_oracle_against_shifts(log_w):
    """second route: sum_k X^k in through orc_mul_by_xai, on random words and on a single value at
    coefficient N - 1 (every term but k = 0 wraps and changes sign)"""
    rng = np.random.default_rng(40 + log_w)
    x = _rand32(rng, (3, N))
    x[2] = 0
    x[2, N - 1] = 0x12345678
    got = AO.box_fill(x, log_w)
    for t in range(3):
        want = np.zeros(N, np.int64)
        for k in range(1 << log_w):
            want += O.mul_by_xai(k, np.ascontiguousarray(x[t])).astype(np.int64)
        assert np.array_equal(got[t], LO.wrap(want)), (t, log_w)
    w = 1 << log_w
    assert got[2, N - 1] == 0x12345678 and np.all(got[2, :w - 1] == -0x12345678) and not got[2, w - 1:N - 1].any()
    if log_w == 0:
        assert np.array_equal(got, x)


def test_trivial_accumulator_is_the_lut_bootstrap(keyset, okey):
    """with (0, tv) the accumulator oracle equals lut_oracle.woks_batch word for word; so does a
    shared accumulator picked through an explicit index"""
    rng = np.random.default_rng(41)
    tvs = _rand32(rng, (2, N))
    x_a, x_b = keyset.encrypt_digits(rng.integers(0, 4, 3), 4, rng)
    acc = np.zeros((2, 2, N), np.int32)
    acc[:, 1] = tvs
    idx = np.array([1, 0, 1])
    got = AO.woks_batch(okey, acc, x_a, x_b, idx)
    want = LO.woks_batch(okey, tvs, x_a, x_b, idx)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    one = AO.woks_batch(okey, acc[1], x_a, x_b)
    want = LO.woks_batch(okey, tvs[1], x_a, x_b)
    assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[1])


def test_argument_rules_without_gpu():
    """every refusal that is decided before a context is touched: a null context with every form"""
    lib, p = T.lib, T._p
    z = np.zeros(2 * N, np.int32)
    assert lib.tfhe_amd_tlwe_box_fill_host(None, 1, 0, p(z), p(z)) == E_ARG
    assert lib.tfhe_amd_tlwe_box_fill_dev(None, 1, 0, None, None, None) == E_ARG
    for f in ("tfhe_amd_bootstrap_acc_woks_batch_host", "tfhe_amd_bootstrap_acc_batch_host"):
        assert getattr(lib, f)(None, 1, 1, p(z), None, 0, 1, p(z), p(z), 0, None, None, p(z), p(z)) == E_ARG
    for f in ("tfhe_amd_bootstrap_acc_woks_batch_dev", "tfhe_amd_bootstrap_acc_batch_dev"):
        assert getattr(lib, f)(None, 1, 1, None, None, 0, 1, None, None, 0, None, None, None, None, None) == E_ARG
    assert lib.tfhe_amd_select_batch_host(None, None, 1, 2, p(z), p(z), 0, 1, p(z), p(z), p(z), p(z)) == E_ARG
    assert lib.tfhe_amd_select_batch_dev(None, None, 1, 2, None, None, 0, 1, None, None, None, None, None) == E_ARG
    assert not z.any()


def test_acc_of_null_index_rule():
    assert np.array_equal(AO.acc_of(1, 3, None), [0, 0, 0]) and np.array_equal(AO.acc_of(3, 3, None), [0, 1, 2])
    with pytest.raises(AssertionError):
        AO.acc_of(2, 3, None)


def test_decode_chain_bootstrapped_selector_reads_bootstrapped_candidates(keyset, okey):
    """Two fresh p = 4 digits x, y (B = 32, fixed seed); the four LUT outputs f(x, r) as candidates, a
    bootstrapped copy of y as selector, select, decode: every query must equal f(x, y).  Prints the
    deviations from the box centres that DESIGN.md §3.8 quotes (margin 1/16 = 0.0625).
    Measured on the oracle: selector largest 0.0085, r.m.s. 0.0041; output largest 0.0133, r.m.s. 0.0065."""
    c = AO.decode_chain(keyset, okey)
    p = c["p"]
    want = c["f"][c["x"], c["y"]]

    def deviation(ph, m):
        d = _centred(ph.astype(np.int64) - T.lut_encode(m, p).astype(np.int64)).astype(np.float64) / 2**32
        return np.abs(d).max(), np.sqrt(np.mean(d * d))

    sel = deviation(keyset.phase(c["sel_a"], c["sel_b"]), c["y"])
    out = deviation(keyset.phase(*c["res"]), want)
    print(f"decode chain B = {c['B']}, p = {p}: selector largest {sel[0]:.4f} r.m.s. {sel[1]:.4f}; "
          f"output largest {out[0]:.4f} r.m.s. {out[1]:.4f}; margin {1 / (4 * p):.4f}")
    for r in range(p):   # the candidates themselves decode (else the chain would test nothing)
        assert np.array_equal(T.lut_decode(keyset.phase(c["cand_a"][r], c["cand_b"][r]), p), c["f"][c["x"], r]), r
    assert np.array_equal(T.lut_decode(keyset.phase(c["sel_a"], c["sel_b"]), p), c["y"])
    assert np.array_equal(T.lut_decode(keyset.phase(*c["res"]), p), want)


def test_box_fill_noise(keyset):
    """T = 16 outputs of p = 4 fresh digit encryptions packed at m N / 4 and box-filled: at every
    coefficient of box m, (box-filled phase - phase of input m) has r.m.s. within [0.5, 1.5] sigma and
    largest value below 8 sigma, sigma = sqrt(500 * 6 * 21.5 * N) * 7.18e-9 = 5.84e-5 (the windows of
    neighbouring coefficients overlap, so the 16 384 values are correlated: hence T = 16)."""
    T_, p = 16, 4
    w = N // p
    rng = np.random.default_rng(3816)
    in_a, in_b = keyset.encrypt_digits(rng.integers(0, p, T_ * p), p, rng)
    key = AO.chain_pack_key(keyset)
    cand_a = np.ascontiguousarray(in_a.reshape(T_, p, n_lwe).transpose(1, 0, 2))
    cand_b = np.ascontiguousarray(in_b.reshape(T_, p).T)
    filled = AO.packed_boxes(key, cand_a, cand_b)
    # the same through the row-by-row pack route on one output
    packed0 = PO.pack_rows(key, in_a[:p][None], in_b[:p][None], np.arange(p) * w)
    assert np.array_equal(AO.box_fill(packed0, 8)[0], filled[0])
    ph = keyset.tlwe_phase(filled).astype(np.int64)                     # [T][N]
    src = keyset.phase(in_a, in_b).astype(np.int64).reshape(T_, p)      # [T][p]
    diff = _centred(ph - np.repeat(src, w, axis=1)).astype(np.float64) / 2**32
    sigma = PO.sigma_pack(N)
    rms, peak = np.sqrt(np.mean(diff * diff)), np.abs(diff).max()
    print(f"box-fill noise T = {T_}, p = {p}: rms {rms:.3e}, max {peak:.3e}, predicted sigma {sigma:.3e}")
    assert abs(sigma - 5.84e-5) < 1e-7
    assert 0.5 * sigma <= rms <= 1.5 * sigma, (rms, sigma)
    assert peak < 8 * sigma, (peak, sigma)
