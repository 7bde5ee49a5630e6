"""Partly flagged batches for the exactness guard (TEST INFRASTRUCTURE: the inputs of
tests/test_guard_partial.py and tests/test_guard_partial_gpu.py; plain numpy, no GPU).

The key: the real bootstrapping key with the polynomials of the key indices 0 .. HEAD - 1 replaced
by the constant 2^31 - 1 (test_guard.py's MAXK); the indices HEAD .. 499 and the key-switching key
stay real.  Two kinds of LWE sample x then enter a blind rotation:
  * clean: x.a[0 : HEAD] = 0, so bara = 0 on every adversarial step (the one-ciphertext kernels
    skip those steps, the paired kernel runs them as identity CMuxes) and the remaining 250 steps
    are real ones: rounding distance <= 0.062 in the fp64 CPU port, nothing flagged;
  * dirty: x.a random everywhere: rounding distance 1/2, flagged, and the unguarded fp64 result is
    wrong for most of them (56 of 64 in the CPU port at mu = 2^29).
A filler is a clean sample with x.a = 0 altogether (no step at all: it costs the oracle nothing).

Every word of a dirty sample is even (the low bit is far below the modulus switch, which reads the
top 11 bits): so the XOR prologue 2 (a + b) + (0, 2^30) can be inverted for any of them as well.

The inverse-prologue builders return gate inputs whose prologue combination is a wanted x exactly,
in wrapping int32 arithmetic; the placement tables say which slots of which launch form are dirty.
"""
import numpy as np

import oracle_ctypes as O

MAXK = 2**31 - 1
HEAD = 250
MU = 1 << 29
N, n_lwe = O.N, O.n_lwe
HOST_SLICE = 1024   # host_batch.cpp host_slice(): host gate batches above it run slice by slice


def head_key(bk):
    """the real key with the polynomials of the key indices 0 .. HEAD - 1 set to the constant MAXK"""
    out = np.array(bk, dtype=np.int32, copy=True)
    out[:HEAD] = MAXK
    return out


def wrap(x):
    return ((np.asarray(x, dtype=np.int64) + 2**31) % 2**32 - 2**31).astype(np.int32)


def _words(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def dirty(rng, n):
    """n dirty samples (a [n][500], b [n]): random even words everywhere"""
    return _words(rng, (n, n_lwe)) & np.int32(-2), _words(rng, n) & np.int32(-2)


def clean(rng, n):
    """n clean samples that still run their 250 real steps"""
    a = _words(rng, (n, n_lwe))
    a[:, :HEAD] = 0
    return a, _words(rng, n)


def filler(rng, n):
    """n clean samples with x.a = 0: no CMux step at all"""
    return np.zeros((n, n_lwe), np.int32), _words(rng, n)


def batch(rng, B, dirty_at, real_at, pool):
    """B samples: fillers, but clean real-step samples at the slots real_at and the dirty samples
    pool = (a, b) (in order, wrapping around) at the slots dirty_at"""
    a, b = filler(rng, B)
    ra, rb = clean(rng, len(real_at))
    for j, s in enumerate(real_at):
        a[s], b[s] = ra[j], rb[j]
    for j, s in enumerate(dirty_at):
        a[s], b[s] = pool[0][j % len(pool[1])], pool[1][j % len(pool[1])]
    assert not set(dirty_at) & set(real_at) and len(set(dirty_at)) == len(dirty_at)
    return a, b


# ------------------------------------------------------------------ inverse prologues

def zero(n):
    return np.zeros((n, n_lwe), np.int32), np.zeros(n, np.int32)


def gate_inputs(gate, x_a, x_b):
    """(ca_a, ca_b, cb_a, cb_b) with (0, c) + sa ca + sb cb = x for the binary gate's prologue
    constants (oracle_ctypes.GATE_SPEC): cb is the zero sample and sa ca = x - (0, c).  |sa| = 2
    (XOR, XNOR) needs even words in x.a and in x.b - c."""
    c, sa, _ = O.GATE_SPEC[gate]
    q_a, q_b = wrap(x_a), wrap(np.asarray(x_b, dtype=np.int64) - c)
    m = abs(sa)
    if np.any(q_a % m) or np.any(q_b % m):
        raise ValueError(f"{gate}: x - (0, c) is not a multiple of {m}")
    s = 1 if sa > 0 else -1
    return (wrap(s * (q_a.astype(np.int64) // m)), wrap(s * (q_b.astype(np.int64) // m))) + zero(q_a.shape[0])


def mux_inputs(x0_a, x0_b, x1_a, x1_b):
    """(a, b, c) sample pairs with -mu + a + b = x0 and -mu - a + c = x1 (the two MUX half rows):
    a is the zero sample, b = x0 + (0, mu), c = x1 + (0, mu)"""
    n = np.asarray(x0_a).shape[0]
    return (zero(n) + (wrap(x0_a), wrap(np.asarray(x0_b, dtype=np.int64) + MU))
            + (wrap(x1_a), wrap(np.asarray(x1_b, dtype=np.int64) + MU)))


# ------------------------------------------------------------------ placement tables
# slots of a launch's ciphertexts; for MUX (ciphertext, half).  real: clean samples that run their
# 250 real steps (at least two per case); every other slot is a filler.

def placements(cus):
    """the cases of test_guard_partial_gpu.py for a device with `cus` compute units (the
    library's form thresholds are in these units: paired above CUs, reg-rotation above 2 CUs,
    chunks of 4 CUs)"""
    assert cus >= 176 and cus % 2 == 0, cus
    P = {}
    P["lds"] = dict(B=6, dirty=[1, 4], real=[0, 5])
    B = cus + 45   # odd: slot B - 1 shares its workgroup with the padding ciphertext
    P["paired"] = dict(B=B, dirty=[10, 21, 64, 65, B - 1], real=[11, 20, B - 2])
    P["paired_clean"] = dict(B=B, dirty=[], real=[10, B - 1])
    P["paired_even"] = dict(B=B - 1, dirty=[B - 2], real=[0, B - 3])
    B = 2 * cus + 8
    P["reg"] = dict(B=B, dirty=[0, B // 2, B - 1], real=[1, B - 2])
    B, base = 5 * cus + 3, 4 * cus
    P["chunked"] = dict(B=B, base=base, dirty=[base - 1, base, base + 1, B - 1], real=[base - 2, base + 2])
    P["mux_small"] = dict(B=5, dirty=[(1, 0), (3, 1), (4, 0), (4, 1)], real=[(0, 0), (1, 1), (3, 0)])
    B = cus // 2 + 21
    B += 1 - B % 2   # odd: rotations B - 1 (half 0) and B (half 1, ciphertext 0) share a workgroup
    assert cus < 2 * B <= 2 * cus
    P["mux_seam_a"] = dict(B=B, dirty=[(B - 1, 0)], real=[(0, 1), (B - 2, 0)])
    P["mux_seam_b"] = dict(B=B, dirty=[(0, 1)], real=[(B - 1, 0), (1, 1)])
    B, base = 2 * cus + 88, 4 * cus   # 2 B > 4 CUs: rotation `base` is ciphertext base - B of half 1
    assert B < base < 2 * B and B <= HOST_SLICE
    P["mux_chunked"] = dict(B=B, base=base, dirty=[(base - B - 1, 1), (base - B, 1)],
                            real=[(base - B - 1, 0), (base - B, 0), (base - B + 1, 1)])
    B = 4 * cus + 40
    assert HOST_SLICE + 20 < B <= 2 * HOST_SLICE
    P["sliced"] = dict(B=B, dirty=[3, HOST_SLICE + 20], real=[HOST_SLICE + 3, 20])
    # circuit level: (row, instance) -> slot row * B + instance of the circuit state's flags
    # (every instance of row 2 runs real steps: its key-switched outputs all have a random mask,
    # which a filler's has not — u.a = 0 switches to a = 0 — so a gate behind it is dirty throughout)
    P["circuit"] = dict(B=7, gates=["NAND", "OR", "ANDNY"], dirty=[(0, 2), (1, 6), (2, 0)],
                        real=[(0, 0), (1, 1)] + [(2, k) for k in range(1, 7)])
    # mixed host batch: rows NAND | MUX half 0 | MUX half 1 | XOR | MUX half 0 | MUX half 1
    P["mixed"] = dict(gates=["NAND", "MUX", "XOR", "MUX"], dirty=[(1, 1), (2, 0)], real=[(0, 0), (3, 0)])
    # (there the dirty rows are 2 and 3, neighbours that a slot off by one bit would merely swap;
    # in this order they are rows 1 and 3, each beside a clean row: MUX, MUX | NAND | XOR | MUX, MUX)
    P["mixed_b"] = dict(gates=["MUX", "NAND", "XOR", "MUX"], dirty=[(0, 1), (2, 0)], real=[(0, 0), (1, 0)])
    P["lut"] = dict(B=5, dirty=[2], real=[0, 4])
    return P


def mux_batch(rng, B, dirty_at, real_at, pool):
    """the two half batches x0, x1 of a MUX batch with (ciphertext, half) placements"""
    flat = lambda at: [h * B + k for k, h in at]
    a, b = batch(rng, 2 * B, flat(dirty_at), flat(real_at), pool)
    return (a[:B], b[:B]), (a[B:], b[B:])
