"""The exact NTT path and the exactness guard at the points where their arithmetic is tight.

The exact kernel (csrc/blind_rotate_v4.hip, ntt_wave.h) runs a reduction-free lazy NTT whose
comments state the bounds < 22q (forward), < 3.75q (MAC), < 31.75q (inverse; 2^32 is 32.0006q), and
a centred CRT over two 27-bit primes whose M/2 = 0.99988 * 2^53 covers the product's |c| <= 2^52
only because k_bk_to_ntt reduces the key words SIGNED.  Random data and real keys never come near
any of these, so everything below is driven by structured keys and saturated digits:

CPU: the oracle's NTT product, its schoolbook product and an integer convolution agree on every
key pattern x digit pattern, and the set reaches |c| = 2^52 exactly; scripts/emu_v4.py (the Python
restatement of the kernel's arithmetic, key reduced as the kernel does) is exact on them with all
its bound assertions live, and goes wrong when the key word is taken unsigned; the comments'
bounds are recomputed from the primes; the int8 key-switch data flow is restated on a KSK of
carry-chain words.
GPU: the exact kernel against the SCHOOLBOOK oracle (every other GPU parity test compares with the
oracle's own NTT route) on one external product and on CMux steps; the guarded default path on the
structured key; the guard on keys whose magnitude sweeps across its threshold; the key switch on
the structured KSK.

Every generator is seeded with a literal so that a failure reproduces in another process."""
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle_ctypes as O
import tfhe_amd as T
from test_ks5_design import keyswitch_v5

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import emu_v4 as E  # noqa: E402

N, n = 1024, 500
Q0, Q1 = 134215681, 134203393          # csrc/modarith.h kQ0, kQ1
MIN, MAX = -2**31, 2**31 - 1

# ---------------------------------------------------------------- shared patterns

_J = np.arange(N)
KEY_PATTERNS = {
    # name -> [4][2][1024] int64 (None: leave the random fill), key index = position in this dict
    "min": lambda: np.full((4, 2, N), MIN),
    "max": lambda: np.full((4, 2, N), MAX),
    "m1": lambda: np.full((4, 2, N), -1),
    "zero": lambda: np.zeros((4, 2, N), np.int64),
    "one": lambda: np.ones((4, 2, N), np.int64),
    "q0": lambda: np.full((4, 2, N), Q0),
    "negq1": lambda: np.full((4, 2, N), -Q1),
    "15q0": lambda: np.full((4, 2, N), 15 * Q0),
    "q_edges": lambda: np.broadcast_to(np.where(_J % 2 == 0, Q0 - 1, Q1 + 1), (4, 2, N)),
    "alt": lambda: np.broadcast_to(np.where(_J % 2 == 0, MIN, MAX), (4, 2, N)),
    "mono_last": lambda: np.broadcast_to(np.where(_J == N - 1, MIN, 0), (4, 2, N)),
    "rowsign": lambda: np.broadcast_to((MAX * (-1) ** (np.arange(4)[:, None] + np.arange(2)[None, :]))[:, :, None],
                                       (4, 2, N)),
    "random": None,
}
KEYS = list(KEY_PATTERNS)
assert 15 * Q0 == 2013235215 and 15 * Q0 <= MAX


def _digit_pairs():
    """name -> ([2][1024] first digits, [2][1024] second digits) of the accumulator patterns that
    are built from digits"""
    lo, hi = -512, 511
    full = lambda v: np.full((2, N), v, np.int64)
    alt = np.broadcast_to(np.where(_J % 2 == 0, lo, hi), (2, N)).astype(np.int64)
    half = np.broadcast_to(np.where(_J < 512, lo, hi), (2, N)).astype(np.int64)
    ab = np.stack([np.full(N, lo), np.full(N, hi)]).astype(np.int64)
    one0 = np.zeros((2, N), np.int64); one0[:, 0] = lo
    one1023 = np.zeros((2, N), np.int64); one1023[:, N - 1] = hi
    return {"all_lo": (full(lo), full(lo)), "all_hi": (full(hi), full(hi)), "alt": (alt, alt),
            "half": (half, half), "a_lo_b_hi": (ab, ab), "zero": (full(0), full(0)),
            "single_0": (one0, one0), "single_1023": (one1023, one1023),
            "word_min": (full(lo), full(0))}        # every word -2^31: digits (-512, 0)


SATURATED = ["all_lo", "all_hi", "alt", "half"]     # one polynomial of digits, every |d| >= 511


def accumulators():
    """name -> acc [2][1024] int32 = (d1 2^22 + d2 2^12) mod 2^32, digits checked with the oracle's
    decomposition; plus the uniform random control"""
    out = {}
    for name, (d1, d2) in _digit_pairs().items():
        acc = O.i32((d1 * 2**22 + d2 * 2**12) & 0xFFFFFFFF)
        for c in range(2):
            dec = O.decompose(acc[c])
            assert np.array_equal(dec[0], d1[c]) and np.array_equal(dec[1], d2[c]), name
        out[name] = acc
    assert np.all(out["word_min"] == MIN)
    out["random"] = np.random.default_rng(1001).integers(MIN, MAX + 1, (2, N), dtype=np.int64).astype(np.int32)
    return out


def structured_bk():
    bk = np.random.default_rng(1002).integers(MIN, MAX + 1, (n, 4, 2, N), dtype=np.int64)
    for k, name in enumerate(KEYS):
        if KEY_PATTERNS[name] is not None:
            bk[k] = KEY_PATTERNS[name]()
    return bk.astype(np.int32)


KSK_WORDS = [0x80808080, 0x7F7F7F7F, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x00000080, 0x0000007F, 0x00008000]


def structured_ksk(seed=1003, h0_seed=1004):
    """[1024][8][4][501]: random; rows h = 1..3 of i = 0..7 mod 16 one carry-chain word of the
    balanced-byte split (k_ksk_to_v5) each; rows h = 0 random NON-ZERO words (no path may read
    them: the reference skips digit 0)"""
    ksk = np.random.default_rng(seed).integers(0, 2**32, (N, 8, 4, n + 1), dtype=np.uint64).astype(np.uint32)
    for r, w in enumerate(KSK_WORDS):
        ksk[r::16, :, 1:, :] = w
    ksk[:, :, 0, :] = np.random.default_rng(h0_seed).integers(1, 2**32, (N, 8, n + 1), dtype=np.uint64)
    return ksk.view(np.int32)


def ks_inputs(B, seed):
    """rows of every digit 0 / 1 / 2 / 3 (of u + 2^15, 8 digits of 2 bits from the top), then random"""
    r = np.random.default_rng(seed)
    u_a = r.integers(MIN, MAX + 1, (B, N), dtype=np.int64)
    for d in range(min(4, B)):
        u_a[d] = ((d * 0x5555) << 16) - 2**15
    u_a = O.i32(u_a & 0xFFFFFFFF)
    aibar = (u_a[:min(4, B)].astype(np.int64) + 2**15) & 0xFFFFFFFF
    for j in range(8):
        assert np.all(((aibar >> (30 - 2 * j)) & 3) == np.arange(min(4, B))[:, None])
    u_b = r.integers(MIN, MAX + 1, B, dtype=np.int64).astype(np.int32)
    return u_a, u_b


def negacyclic_int(d, b, dtype=object):
    """d * b mod X^1024 + 1 over the integers (no reduction).  dtype=object: Python integers;
    np.int64 is exact too while sum |d| |b| < 2^63 (here <= 1024 * 512 * 2^31 = 2^50 per product)."""
    full = np.convolve(np.asarray(d).astype(dtype), np.asarray(b).astype(dtype))
    out = full[:N].copy()
    out[:N - 1] -= full[N:]
    return out


def _u32(x):
    return np.asarray(x).astype(np.int64) & 0xFFFFFFFF


_CACHE = {}


def fixture_set():
    """bk, the accumulators and, for every (key pattern, accumulator), the external product three
    ways: integer convolution (exact c, before the reduction mod 2^32), schoolbook oracle, NTT
    oracle.  Computed once per process and never modified."""
    if not _CACHE:
        bk = structured_bk()
        accs = accumulators()
        school = O.OracleKey(bk, None, use_ntt=False)
        ntt = O.OracleKey(bk, None, use_ntt=True)
        exact, want_s, want_n = {}, {}, {}
        for a, acc in accs.items():
            dec = np.concatenate([O.decompose(acc[0]), O.decompose(acc[1])]).astype(np.int64)   # [4][N]
            for k, key in enumerate(KEYS):
                c = np.zeros((2, N), np.int64)
                for p in range(4):
                    for col in range(2):        # |sum| <= 4 * 2^50 = 2^52: int64 is exact
                        c[col] += negacyclic_int(dec[p], bk[k, p, col], np.int64)
                exact[key, a] = c
                want_s[key, a] = school.external_product(acc, k)
                want_n[key, a] = ntt.external_product(acc, k)
        for v in list(want_s.values()) + list(want_n.values()) + list(exact.values()) + list(accs.values()) + [bk]:
            v.setflags(write=False)
        _CACHE.update(bk=bk, accs=accs, school=school, ntt=ntt, exact=exact, want_s=want_s, want_n=want_n)
    return _CACHE


# ---------------------------------------------------------------- CPU

def test_oracle_products_at_the_extremes():
    """One digit polynomial x one key polynomial: NTT route = schoolbook route = Python-integer
    convolution mod 2^32, on every key pattern x every saturated digit pattern."""
    bk = structured_bk()
    digs = {a: _digit_pairs()[a][0][0] for a in SATURATED}
    worst = 0
    for k, key in enumerate(KEYS):
        for p, c in (((0, 0), (0, 1)) if key == "rowsign" else ((0, 0),)):     # rowsign: both signs
            poly = bk[k, p, c]
            for a, d in digs.items():
                big = negacyclic_int(d, poly, object)
                worst = max(worst, max(abs(int(v)) for v in big))
                want = np.array([int(v) % 2**32 for v in big], dtype=np.int64)
                zero = np.zeros(N, np.int32)
                got_n = O.negacyclic_addmul(zero, d, poly, ntt=True)
                got_s = O.negacyclic_addmul(zero, d, poly, ntt=False)
                assert np.array_equal(_u32(got_s), want), (key, a, "schoolbook")
                assert np.array_equal(_u32(got_n), want), (key, a, "ntt")
                assert np.array_equal(negacyclic_int(d, poly, np.int64).astype(object), big), (key, a, "int64")
    assert worst == 2**50, worst                  # 1024 * 512 * 2^31: (min, all -512)


def test_oracle_external_products_reach_the_crt_extreme():
    """OracleKey.external_product on the structured key, NTT and schoolbook, against the integer
    product for every (key pattern, accumulator pattern); the set's largest |c| is 2^52 exactly —
    the most the four rows can give, and what the kernel's centred CRT (M/2 = 0.99988 * 2^53) and
    the guard's binade check are sized for."""
    F = fixture_set()
    worst = {}
    for (key, a), c in F["exact"].items():
        want = c & 0xFFFFFFFF
        assert np.array_equal(_u32(F["want_s"][key, a]), want), (key, a, "schoolbook")
        assert np.array_equal(_u32(F["want_n"][key, a]), want), (key, a, "ntt")
        worst[key, a] = int(np.max(np.abs(c)))
    assert max(worst.values()) == 2**52, max(worst.values())
    assert worst["min", "all_lo"] == 2**52
    assert worst["alt", "alt"] > 2**52 - 2**43      # 4 * 512 * (512 (2^31 - 1) + 511 * 2^31) = 2^52 - 2^42 - 2^20
    assert 2**52 < Q0 * Q1 // 2


def _emu_rows(key, k, bk):
    """the 4 rows of column c = 0 as Python integers, as the kernel reads them (int32)"""
    return [[int(v) for v in bk[k, p, 0]] for p in range(4)]


def test_emu_v4_exact_and_within_bounds_at_the_extremes():
    """scripts/emu_v4.py (the kernel's lazy arithmetic, key reduced signed as k_bk_to_ntt does) on
    saturated digits x extreme keys: no mismatch against the integer product, and none of its
    bound assertions (forward < 22q, MAC < 3.75q, x < 2^61, inverse < 31.75q, no 32-bit wrap in any
    butterfly, CRT difference positive) fires."""
    bk = structured_bk()
    pairs = _digit_pairs()
    peaks = {"fwd": 0.0, "mac": 0.0, "inv": 0.0}
    for key in ("min", "max", "m1", "alt", "15q0", "random"):
        k = KEYS.index(key)
        rows = _emu_rows(key, k, bk)
        for a in SATURATED:
            D = [[int(v) for v in pairs[a][0][0]]] * 4
            got, pk = E.external_product(D, rows)
            c = sum(negacyclic_int(D[p], rows[p], np.int64) for p in range(4))
            assert np.array_equal(np.array(got, dtype=np.int64), c & 0xFFFFFFFF), (key, a)
            print(f"emu_v4 {key:>6} x {a:<7}: forward {pk['fwd']:.2f}q  MAC {pk['mac']:.2f}q  inverse {pk['inv']:.2f}q")
            peaks = {s: max(peaks[s], pk[s]) for s in peaks}
    print(f"emu_v4 peaks: forward {peaks['fwd']:.2f}q (< 22q)  MAC {peaks['mac']:.2f}q (< 3.75q)  "
          f"inverse {peaks['inv']:.2f}q (< 31.75q)")
    assert peaks["fwd"] < 22 and peaks["mac"] < 3.75 and peaks["inv"] < 31.75


def test_emu_v4_unsigned_key_reduction_goes_wrong():
    """Why the sign matters: the key word -1 read as 0xFFFFFFFF gives the same product mod 2^32 but
    |c| = 4 * 1024 * 512 * (2^32 - 1) = 2^53 - 2^21 > q0 q1 / 2, which the centred CRT cannot
    return; read signed, |c| = 2^21 and the result is exact."""
    D = [[-512] * N] * 4
    signed, _ = E.external_product(D, [[-1] * N] * 4)
    unsigned, _ = E.external_product(D, [[0xFFFFFFFF] * N] * 4)
    c = sum(negacyclic_int(D[p], [-1] * N, np.int64) for p in range(4))
    want = [int(v) for v in c & 0xFFFFFFFF]
    assert signed == want
    bad = sum(1 for g, w in zip(unsigned, want) if g != w)
    print("unsigned key words: mismatches", bad)
    assert bad >= 1
    assert 4 * N * 512 * 0xFFFFFFFF == 2**53 - 2**21 > Q0 * Q1 // 2


def test_lazy_bounds_follow_from_the_primes():
    """The bounds the kernel comments state, recomputed from the primes alone (exact rational
    arithmetic in integers): a change of primes or one more lazy stage fails here."""
    assert E.Q == [Q0, Q1]
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "cpu-gpu-tfhe_amd", "csrc", "modarith.h")).read()
    assert f"kQ0 = {Q0}u" in src and f"kQ1 = {Q1}u" in src
    W = 2**32
    for q in (Q0, Q1):
        assert q % 2048 == 1 and q < 2**27
        fwd = 2 * q + 10 * 2 * q                   # digits enter < 2q, each of 10 butterflies adds 2q
        assert fwd == 22 * q and fwd < W
        assert 4 * fwd * q == 88 * q * q and 88 * q * q < 2**61           # the MAC's 64-bit sum (bk < q)
        # REDC (x + m q) >> 32 with x < 88 q^2 and m < 2^32 is < q (88 q / 2^32 + 1), which is < 3.75 q
        assert ((88 * q * q - 1) + (W - 1) * q) // W < (q * (88 * q + W)) // W + 1
        assert 4 * q * (88 * q + W) < 15 * q * W
        # inverse, in units of q / 4 (3.75q = 15): the twiddle-1 stages give (u + v, u + K - v)
        mac, K0, K1 = 15, 4 * 4, 4 * 8
        assert mac < K0                            # K - v stays positive
        s0 = max(mac + mac, mac + K0)
        assert s0 == 31 and s0 < K1                # < 7.75 q after stage 0
        s1 = max(s0 + s0, s0 + K1)
        assert s1 == 63                            # < 15.75 q after stage 1
        inv = s1 + 8 * 4 * 2                       # the 8 Shoup stages add 2q each
        assert inv == 127 and inv * q < 4 * W      # 31.75 q < 2^32
        assert (inv + 4 * 2) * q > 4 * W           # and a ninth lazy stage would not fit
    assert 31.75 * Q0 == 4261347871.75             # the figure quoted for the tighter prime
    assert 2**52 < Q0 * Q1 // 2 < 2**53            # centred CRT holds |c| <= 2^52, not 2^53 - 2^21
    # crt_lazy: d = x1 + 3 q1 - x0 with lazy x0 in [0, 2 q0), x1 in [0, 2 q1).  Since q0 > q1 its lower
    # end is 3 q1 - 2 q0 = q1 - 2 (q0 - q1), a little BELOW q1: the interval is (3 q1 - 2 q0, 5 q1),
    # not the (q1, 5 q1) the kernel comment used to state.  What the lift needs is 0 < d < 2^32 (no
    # wrap; shoup_lazy takes any 32-bit value), and that holds.
    lo, hi = 0 + 3 * Q1 - (2 * Q0 - 1), (2 * Q1 - 1) + 3 * Q1 - 0
    assert 0 < 3 * Q1 - 2 * Q0 < lo and hi < 5 * Q1 < W
    assert lo < Q1
    assert Q0 < 2 * Q1                             # x0 mod q1 needs one conditional subtraction


def test_keyswitch_v5_dataflow_on_carry_chain_words():
    """The int8 key switch's data flow (test_ks5_design.keyswitch_v5) against the oracle on a KSK of
    carry-chain words (0x80808080: every byte -128 with a carry into the next, ...), inputs of
    every digit 0, 3, 1 and random; the h = 0 rows are garbage in one run and zero in the other and
    the results do not depend on them."""
    ksk = structured_ksk()
    u_a, u_b = ks_inputs(6, 1005)
    u_a = u_a[[0, 3, 1, 4, 5]]; u_b = u_b[[0, 3, 1, 4, 5]]
    zeroed = ksk.copy()
    zeroed[:, :, 0, :] = 0
    o_a, o_b = O.OracleKey(None, ksk).keyswitch_batch(u_a, u_b)
    z_a, z_b = O.OracleKey(None, zeroed).keyswitch_batch(u_a, u_b)
    assert np.array_equal(o_a, z_a) and np.array_equal(o_b, z_b)
    assert np.all(o_a[0] == 0) and o_b[0] == u_b[0]         # every digit 0: nothing subtracted
    for k in (ksk, zeroed):
        r_a, r_b = keyswitch_v5(k, u_a, u_b)
        assert np.array_equal(r_a, o_a) and np.array_equal(r_b, o_b)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def xctx():
    c = T.Context(fixture_set()["bk"], structured_ksk(), device=0)
    yield c
    c.close()


@pytest.mark.gpu
def test_exact_kernel_one_step_vs_schoolbook(xctx):
    """One tfhe_amd_external_product_dev launch over every (key pattern, accumulator pattern) pair,
    word for word against the schoolbook oracle.  (m1, all_lo) separates signed from unsigned key
    reduction; (min, all_lo) is |c| = 2^52; the saturated digits drive the lazy NTT's peaks."""
    import torch
    F = fixture_set()
    pairs = [(key, a) for key in KEYS for a in F["accs"]]
    acc = np.stack([F["accs"][a] for _, a in pairs])
    idx = np.array([KEYS.index(key) for key, _ in pairs], np.int32)
    d_acc = torch.from_numpy(acc.copy()).cuda()
    d_idx = torch.from_numpy(idx).cuda()
    rc = T.lib.tfhe_amd_external_product_dev(xctx.h, len(pairs), ctypes.c_void_p(d_idx.data_ptr()),
                                             ctypes.c_void_p(d_acc.data_ptr()), None)
    assert rc == 0
    xctx.sync()
    got = d_acc.cpu().numpy()
    bad = [p for b, p in enumerate(pairs) if not np.array_equal(got[b], F["want_s"][p])]
    assert not bad, bad


@pytest.mark.gpu
def test_exact_kernel_cmux_steps_vs_schoolbook(xctx):
    """13 CMux steps of the exact kernel (one per key pattern) on one accumulator per pattern, with
    the rotations 1, N - 1, N (the decomposed polynomial is -2 ACC), N + 1, 2N - 1 and random ones,
    against the schoolbook oracle's tfhe_MuxRotate."""
    import torch
    F = fixture_set()
    names = list(F["accs"])
    B, iters = len(names), len(KEYS)
    assert (B, iters) == (10, 13)
    acc0 = np.stack([F["accs"][a] for a in names])
    bara = np.random.default_rng(1006).integers(1, 2048, (B, iters), dtype=np.int64).astype(np.int32)
    edges = [1, 1023, 1024, 1025, 2047]
    for b in range(B):
        for t in range(iters):
            if (b + t) % 2 == 0:
                bara[b, t] = edges[(b + 3 * t) % 5]
    bara[:, 0] = 1024                            # first step on the patterns themselves: -2 ACC
    default = T.version()
    try:
        T.select_kernel(4)
        d_acc = torch.from_numpy(acc0.copy()).cuda()
        xctx.blind_rotate_dev(d_acc, torch.from_numpy(bara).cuda(), iters)
        xctx.sync()
        got = d_acc.cpu().numpy()
    finally:
        tag = default.split("br-v")[1].split(" ")[0]
        T.select_kernel(int(tag) if tag.isdigit() else 0)
    for b in range(B):
        want = acc0[b].copy()
        for t in range(iters):
            want = F["school"].mux_rotate(want, t, int(bara[b, t]))
        assert np.array_equal(got[b], want), names[b]


@pytest.mark.gpu
def test_guarded_path_on_structured_key(xctx):
    """The product's default path (fp64 kernel + guard + key switch) on the structured key and KSK:
    woKS and full bootstraps word for word the oracle's."""
    r = np.random.default_rng(1007)
    B = 16
    x_a = r.integers(MIN, MAX + 1, (B, n), dtype=np.int64).astype(np.int32)
    x_b = r.integers(MIN, MAX + 1, B, dtype=np.int64).astype(np.int32)
    okey = O.OracleKey(xctx.bk, xctx.ksk, use_ntt=True)
    xctx.guard_stats(reset=True)
    u = xctx.woks_host(T.MU, x_a, x_b)
    g = xctx.bootstrap_host(T.MU, x_a, x_b)
    print("guard_stats (distance, recomputed) over 2 x 16 bootstraps:", xctx.guard_stats(reset=True))
    want_u = okey.woks_batch(T.MU, x_a, x_b, nthreads=8)
    want_g = okey.keyswitch_batch(*want_u, nthreads=8)
    assert np.array_equal(u[0], want_u[0]) and np.array_equal(u[1], want_u[1])
    assert np.array_equal(g[0], want_g[0]) and np.array_equal(g[1], want_g[1])


GUARD_MAGNITUDES = [2**27, 2**29, 2**30, 3 * 2**29, 2**31 - 1]


@pytest.mark.gpu
def test_guard_across_the_threshold():
    """Keys of one constant magnitude and a random sign per polynomial, the magnitude swept from
    where the fp64 error is far below the guard's 1/8 (2^27: 0.031 in the CPU port) to where an
    existing test sees every ciphertext recomputed (2^31 - 1): guarded results are exact for every
    key, the guard recomputes at least the ciphertexts the raw fp64 steps get wrong, and over the
    sweep some but not all launches' ciphertexts are flagged."""
    from test_guard import _raw_fp64_woks
    r = np.random.default_rng(1008)
    B = 16
    x_a = r.integers(MIN, MAX + 1, (B, n), dtype=np.int64).astype(np.int32)
    x_b = r.integers(MIN, MAX + 1, B, dtype=np.int64).astype(np.int32)
    ksk = structured_ksk()
    sign = r.choice([-1, 1], size=(n, 4, 2, 1))
    report = []
    for m in GUARD_MAGNITUDES:
        bk = np.broadcast_to(sign * m, (n, 4, 2, N)).astype(np.int32)
        c = T.Context(bk, ksk, device=0)
        try:
            g = c.woks_host(T.MU, x_a, x_b)
            d, redo = c.guard_stats()
            u = _raw_fp64_woks(c, x_a, x_b)
        finally:
            c.close()
        want = O.OracleKey(bk, None, use_ntt=True).woks_batch(T.MU, x_a, x_b, nthreads=8)
        wrong = lambda v: int(np.sum(np.any(v[0] != want[0], axis=1) | (v[1] != want[1])))
        report.append({"magnitude": m, "guard_distance": d, "recomputed": redo, "wrong_unguarded": wrong(u),
                       "wrong_guarded": wrong(g)})
    print("| key magnitude | guard_distance | recomputed / 16 | wrong_unguarded | wrong_guarded |")
    print("|---|---|---|---|---|")
    for row in report:
        print(f"| {row['magnitude']} | {row['guard_distance']:.4f} | {row['recomputed']} | {row['wrong_unguarded']} | "
              f"{row['wrong_guarded']} |")
    for row in report:
        assert row["wrong_guarded"] == 0, row
        assert row["recomputed"] >= row["wrong_unguarded"], row
    total = sum(row["recomputed"] for row in report)
    assert 0 < total < len(GUARD_MAGNITUDES) * B, report


@pytest.mark.gpu
def test_keyswitch_on_structured_ksk(xctx):
    """keyswitch_host on the KSK of carry-chain words at B = 5 (per-key-index kernel), 40 and 300
    (ks-v5, split 8 and 4), inputs of every digit 0 / 1 / 2 / 3 then random, against the oracle; a
    second context whose KSK differs only in the h = 0 rows gives identical words."""
    okey = O.OracleKey(None, xctx.ksk)
    got = {}
    for B in (5, 40, 300):
        u_a, u_b = ks_inputs(B, 1009 + B)
        got[B] = xctx.keyswitch_host(u_a, u_b)
        o_a, o_b = okey.keyswitch_batch(u_a, u_b, nthreads=8)
        assert np.array_equal(got[B][0], o_a) and np.array_equal(got[B][1], o_b), B
    other_ksk = structured_ksk(h0_seed=1010)
    assert np.array_equal(other_ksk[:, :, 1:], xctx.ksk[:, :, 1:])
    assert not np.array_equal(other_ksk[:, :, 0], xctx.ksk[:, :, 0])
    other = T.Context(xctx.bk, other_ksk, device=0)
    try:
        for B in (5, 40):
            k_a, k_b = other.keyswitch_host(*ks_inputs(B, 1009 + B))
            assert np.array_equal(k_a, got[B][0]) and np.array_equal(k_b, got[B][1]), B
    finally:
        other.close()
