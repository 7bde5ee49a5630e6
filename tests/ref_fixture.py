"""tests/golden/ref_hotpath_vectors.npz: the reference's OWN hot-path functions on fixed inputs
(TEST INFRASTRUCTURE: read by tests/test_ref_hotpath.py and tests/test_ref_fixtures_gpu.py, written
by tests/golden/make_golden.py).

The file holds data only.  Every output family `name` of C cases is stored as
    name_sha   [C]       sha256 of the case's little-endian int32 words
    name_head  [C][16]   its first 16 words      name_tail [C][16]   its last 16 words
    name       [F][...]  the first F <= C cases word for word (the edge cases come first)
and `same(G, name, i, got)` compares a result with all that the file has of case i.

Ref is the ctypes binding of oracle/_ref/libtfheref.so (the reference's functions, compiled from
its own text by oracle/build_ref.sh); it exists where the reference does, never on a GPU machine."""
import ctypes
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PATH = os.path.join(HERE, "golden", "ref_hotpath_vectors.npz")
REF_SO = os.path.join(REPO, "oracle", "_ref", "libtfheref.so")
REF_AVX2_SO = os.path.join(REPO, "oracle", "_ref", "libtfheref_avx2.so")

N, n_lwe = 1024, 500
MU = 1 << 29
OFFSET = 512 * ((1 << 22) + (1 << 12))      # tgsw.cu:7-29, pinned by test_oracle_golden.py
NAND, XOR, MUX = 0, 3, 10
GATE_NAME = {NAND: "NAND", XOR: "XOR", MUX: "MUX"}

_I32P = ctypes.POINTER(ctypes.c_int32)
_VP = ctypes.c_void_p


def load():
    return np.load(PATH)


def _has_hot_path(path):
    """the library at `path` exports the ref_hp_* entry points (read from the file: a library
    this process has already loaded is not loaded again after a rebuild)"""
    with open(path, "rb") as f:
        return b"ref_hp_key_create" in f.read()


def ref_library():
    """True when oracle/_ref/ holds the reference library WITH its hot-path entry points.  A library
    left by an earlier recipe (leaf functions only) is rebuilt by oracle/build_ref.sh, which does
    nothing where the reference is absent; without the entry points it counts as absent."""
    if not os.path.exists(REF_SO):
        return False
    if not (_has_hot_path(REF_SO) and os.path.exists(REF_AVX2_SO)) and os.access(os.path.dirname(REF_SO), os.W_OK):
        import subprocess
        subprocess.check_call([os.path.join(REPO, "oracle", "build_ref.sh")], stdout=subprocess.DEVNULL)
    return _has_hot_path(REF_SO) and os.path.exists(REF_AVX2_SO)


def i32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64).astype(np.int32))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def pack(out, name, cases, n_full):
    """store the outputs `cases` (equal shapes) of one family, the first n_full in full"""
    cases = [np.ascontiguousarray(c, dtype=np.int32) for c in cases]
    flat = [c.reshape(-1) for c in cases]
    out[name + "_sha"] = np.array([sha(c) for c in cases])
    out[name + "_head"] = np.stack([f[:16] for f in flat])
    out[name + "_tail"] = np.stack([f[-16:] for f in flat])
    out[name] = np.stack(cases[:n_full])


def same(G, name, i, got):
    """got == case i of family `name`, by everything the fixture holds of it"""
    got = np.ascontiguousarray(got, dtype=np.int32)
    flat = got.reshape(-1)
    ok = sha(got) == str(G[name + "_sha"][i])
    ok = ok and np.array_equal(flat[:16], G[name + "_head"][i]) and np.array_equal(flat[-16:], G[name + "_tail"][i])
    if i < G[name].shape[0]:
        ok = ok and got.shape == G[name][i].shape and np.array_equal(got, G[name][i])
    return bool(ok)


def full(G, name):
    """how many cases of the family are stored word for word"""
    return G[name].shape[0]


def _p(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_I32P)


class Ref:
    """The reference's functions over flat arrays (oracle/ref_driver.cpp's ref_hp_* entry points).
    bk [n_bk][4][2][1024] and ksk [1024][8][4][501] may each be None."""

    def __init__(self, bk=None, ksk=None, lib=REF_SO):
        self.L = ctypes.CDLL(lib)
        self.L.ref_hp_key_create.restype = _VP
        self.L.ref_hp_key_create.argtypes = [_I32P, ctypes.c_int, _I32P]
        self.L.ref_hp_key_free.argtypes = [_VP]
        self.bk = None if bk is None else i32(bk)
        self.ksk = None if ksk is None else i32(ksk)
        self.h = self.L.ref_hp_key_create(None if bk is None else _p(self.bk), 0 if bk is None else self.bk.shape[0],
                                          None if ksk is None else _p(self.ksk))

    def close(self):
        if self.h:
            self.L.ref_hp_key_free(self.h)
            self.h = None

    def modswitch(self, x, M):
        x = i32(x).reshape(-1)
        out = np.zeros_like(x)
        self.L.ref_modswitch_from(_p(out), _p(x), len(x), int(M))
        return out

    def mul_by_xai(self, a, x, minus_one=False):
        out = np.zeros(N, np.int32)
        f = self.L.ref_hp_mul_by_xai_minus_one if minus_one else self.L.ref_hp_mul_by_xai
        f(_p(out), int(a), _p(i32(x)), N)
        return out

    def decompose(self, x):
        return decompose(self.L, x)

    def extract(self, acc, index):
        out = np.zeros(N, np.int32)
        b = ctypes.c_int32(0)
        self.L.ref_hp_extract(_VP(self.h), _p(out), ctypes.byref(b), _p(i32(acc).reshape(2 * N)), int(index))
        return out, b.value

    def keyswitch(self, u_a, u_b):
        out = np.zeros(n_lwe, np.int32)
        b = ctypes.c_int32(0)
        self.L.ref_hp_keyswitch(_VP(self.h), _p(out), ctypes.byref(b), _p(i32(u_a)), ctypes.c_int32(int(u_b)))
        return out, b.value

    def external_product(self, acc, i):
        acc = i32(acc).reshape(2 * N).copy()
        self.L.ref_hp_external_product(_VP(self.h), _p(acc), int(i))
        return acc.reshape(2, N)

    def mux_rotate(self, acc, i, a):
        acc = i32(acc).reshape(2 * N).copy()
        self.L.ref_hp_mux_rotate(_VP(self.h), _p(acc), int(i), int(a))
        return acc.reshape(2, N)

    def blind_rotate(self, acc, bara):
        acc = i32(acc).reshape(2 * N).copy()
        bara = i32(bara)
        self.L.ref_hp_blind_rotate(_VP(self.h), _p(acc), _p(bara), len(bara))
        return acc.reshape(2, N)

    def blind_rotate_extract(self, tv, barb, bara):
        out = np.zeros(N, np.int32)
        b = ctypes.c_int32(0)
        bara = i32(bara)
        self.L.ref_hp_blind_rotate_extract(_VP(self.h), _p(out), ctypes.byref(b), _p(i32(tv)), int(barb), _p(bara),
                                           len(bara))
        return out, b.value

    def _boot(self, f, width, mu, x_a, x_b):
        out = np.zeros(width, np.int32)
        b = ctypes.c_int32(0)
        f(_VP(self.h), _p(out), ctypes.byref(b), ctypes.c_int32(int(mu)), _p(i32(x_a)), ctypes.c_int32(int(x_b)))
        return out, b.value

    def bootstrap_woks(self, mu, x_a, x_b):
        return self._boot(self.L.ref_hp_bootstrap_woks, N, mu, x_a, x_b)

    def bootstrap(self, mu, x_a, x_b):
        return self._boot(self.L.ref_hp_bootstrap, n_lwe, mu, x_a, x_b)

    def gate(self, code, in_a, in_b):
        """in_a [3][500], in_b [3] (the third input only for MUX)"""
        out = np.zeros(n_lwe, np.int32)
        b = ctypes.c_int32(0)
        in_a = i32(in_a)
        rc = self.L.ref_hp_gate(_VP(self.h), int(code), _p(out), ctypes.byref(b),
                                *sum(([_p(in_a[k]), ctypes.c_int32(int(in_b[k]))] for k in range(3)), []))
        assert rc == 0, code
        return out, b.value


def decompose(L, x):
    """ref_hp_decompose of the library L (the scalar or the AVX2 build) -> [2][N]"""
    out = np.zeros((2, N), np.int32)
    L.ref_hp_decompose(_p(out), _p(i32(x)), N)
    return out
