"""Bootstrap from encrypted accumulators composed from the CPU oracle's own functions
and numpy (TEST INFRASTRUCTURE: the expected values of tests/test_acc.py and tests/test_acc_gpu.py).

  woks_one    lut_oracle.woks_one with the accumulator X^{2N - barb} (acc_a, acc_b) in place of the
              trivial (0, X^{2N - barb} tv): orc_mul_by_xai on both polynomials, orc_blind_rotate on the
              explicit accumulator, extraction at index 0;
  box_fill    out[j] = sum_{k < w} +-in[(j - k) mod N] as plain int64 sums, wrapped;
  select      pack_oracle (candidate m at coefficient m N / p) -> box_fill -> woks -> keyswitch_batch."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import lut_oracle as LO
import oracle_ctypes as O
import pack_oracle as PO

N, n_lwe = O.N, O.n_lwe
THREADS = LO.THREADS
wrap = LO.wrap


def woks_one(okey, acc, x_a, x_b):
    """one sample from the TLWE accumulator acc [2][N] -> (u_a [N], u_b)"""
    L = O.lib()
    bara = np.ascontiguousarray(LO.modswitch_2n(x_a))
    barb = int(LO.modswitch_2n(np.int64(x_b)))
    e = (2 * N - barb) % (2 * N)
    a = np.zeros((2, N), np.int32)
    a[0] = O.mul_by_xai(e, np.ascontiguousarray(acc[0]))
    a[1] = O.mul_by_xai(e, np.ascontiguousarray(acc[1]))
    L.orc_blind_rotate(O._p(a.reshape(2 * N)), ctypes.c_void_p(okey.h), O._p(bara), n_lwe)
    u_a = np.empty(N, np.int32)
    u_a[0] = a[0, 0]
    u_a[1:] = wrap(-a[0, :0:-1].astype(np.int64))
    return u_a, int(a[1, 0])


def acc_of(n_acc, B, acc_index):
    """the accumulator of each ciphertext under the entry points' rule for a null index"""
    if acc_index is not None:
        return np.asarray(acc_index, dtype=np.int64)
    assert n_acc in (1, B)
    return np.zeros(B, np.int64) if n_acc == 1 else np.arange(B)


def woks_batch(okey, accs, x_a, x_b, acc_index=None):
    """B samples from their accumulators: accs [n_acc][2][N] (or one [2][N])"""
    accs = O.i32(accs).reshape(-1, 2, N)
    x_a, x_b = O.i32(x_a), O.i32(x_b)
    B = x_a.shape[0]
    idx = acc_of(accs.shape[0], B, acc_index)
    with ThreadPoolExecutor(THREADS) as pool:
        out = list(pool.map(lambda i: woks_one(okey, accs[idx[i]], x_a[i], x_b[i]), range(B)))
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def bootstrap_batch(okey, accs, x_a, x_b, acc_index=None):
    u_a, u_b = woks_batch(okey, accs, x_a, x_b, acc_index)
    return okey.keyswitch_batch(u_a, u_b, nthreads=THREADS)


def box_fill(tlwe, log_w):
    """tlwe [..., N] int32 -> tlwe (1 + X + ... + X^(2^log_w - 1)), negacyclic, wrapped"""
    x = np.asarray(tlwe).astype(np.int64)
    ext = np.concatenate([-x, x], axis=-1)              # ext[N + j] = x[j], ext[N + j - k] = -x[N + j - k] below 0
    out = np.zeros_like(x)
    for k in range(1 << log_w):
        out += ext[..., N - k:2 * N - k]
    return wrap(out)


def packed_boxes(pack_key, cand_a, cand_b):
    """function-major candidates cand_a [p][B][500], cand_b [p][B] -> the B box-filled accumulators
    [B][2][N] of select"""
    cand_a, cand_b = O.i32(cand_a), O.i32(cand_b)
    p = cand_a.shape[0]
    log_w = (N // p).bit_length() - 1
    in_a = np.ascontiguousarray(cand_a.transpose(1, 0, 2))
    in_b = np.ascontiguousarray(cand_b.T)
    packed = PO.pack_inputs(pack_key, in_a, in_b, np.arange(p) * (N // p))
    return box_fill(packed, log_w)


def select(okey, pack_key, cand_a, cand_b, c, sa, y_a, y_b):
    """the composed p-way selector -> (r_a [B][500], r_b [B])"""
    B = np.asarray(y_b).shape[0]
    x_a, x_b = LO.lin(c, [(sa, (y_a, y_b))], B)
    return bootstrap_batch(okey, packed_boxes(pack_key, cand_a, cand_b), x_a, x_b)


_chain = {}


def chain_pack_key(keyset):
    """the generated packing key of the decode chain and the noise test (fixed generator seed)"""
    import tfhe_amd as T
    if "key" not in _chain:
        T.lib.tfhe_random_generator_setSeed((ctypes.c_uint32 * 2)(2025, 38), 2)
        _chain["key"] = keyset.pack_key()
    return _chain["key"]


def decode_chain(keyset, okey, B=32, p=4):
    """The decode chain of tests/test_acc.py, all on the oracle, once per process (fixed seed): two
    fresh p-digit batches x, y; candidates r = LUT bootstrap of x through f(., r), function-major; the
    selector a bootstrapped copy of y (identity table); res = select.  -> dict"""
    import tfhe_amd as T
    if "case" not in _chain:
        rng = np.random.default_rng(3808)
        x, y = rng.integers(0, p, B), rng.integers(0, p, B)
        f = rng.integers(0, p, (p, p))                       # f[m][r] = f(m, r)
        x_a, x_b = keyset.encrypt_digits(x, p, rng)
        y_a, y_b = keyset.encrypt_digits(y, p, rng)
        tvs = np.stack([T.lut_table(p, T.lut_encode(f[:, r], p)) for r in range(p)])
        cand = [LO.bootstrap_batch(okey, tvs[r], x_a, x_b) for r in range(p)]
        cand_a, cand_b = np.stack([c[0] for c in cand]), np.stack([c[1] for c in cand])
        sel_a, sel_b = LO.bootstrap_batch(okey, T.lut_table(p, T.lut_encode(np.arange(p), p)), y_a, y_b)
        key = chain_pack_key(keyset)
        res = select(okey, key, cand_a, cand_b, 0, 1, sel_a, sel_b)
        _chain["case"] = dict(p=p, B=B, x=x, y=y, f=f, cand_a=cand_a, cand_b=cand_b, sel_a=sel_a, sel_b=sel_b,
                              key=key, res=res)
    return _chain["case"]
