"""Python binding (ctypes) of libtfhe_amd.so — the MI355X TFHE gate-bootstrapping engine.

Thin host-side mirror of the C ABI (include/tfhe/tfhe.h = the TFHE API cpuParallel links,
include/tfhe_amd.h = the batched device API).  It exists for the tests and bench.py; the
product is the C ABI itself.  Importing this module loads lib/libtfhe_amd.so and fails
loudly if it is missing (there is no CPU fallback).

Ciphertext batches are SoA numpy / torch arrays: a int32 [B][500], b int32 [B].
"""
import ctypes
import os

import numpy as np

try:
    # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's): load it FIRST so
    # that this process has one HIP runtime, shared by torch tensors and our kernels.
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - the C ABI itself does not need torch
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
# TFHE_AMD_LIB selects an alternative build of the same library (A/B kernel variants)
LIB_PATH = os.environ.get("TFHE_AMD_LIB") or os.path.join(HERE, "lib", "libtfhe_amd.so")

N, n_lwe, KPL, KS_T, KS_BASE = 1024, 500, 4, 8, 4
PACK_T = 6   # digits of the packing key switch (params.h kPackT)
GATES = {"NAND": 0, "OR": 1, "AND": 2, "XOR": 3, "XNOR": 4, "NOR": 5,
         "ANDNY": 6, "ANDYN": 7, "ORNY": 8, "ORYN": 9, "MUX": 10}
MU = 1 << 29   # modSwitchToTorus32(1, 8)

_I32P = ctypes.POINTER(ctypes.c_int32)
_VP = ctypes.c_void_p


class TfheAmdError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise TfheAmdError(
            f"{LIB_PATH} is missing: build it (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C cpu-gpu-tfhe_amd). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    L.tfhe_amd_version.restype = ctypes.c_char_p
    L.new_default_gate_bootstrapping_parameters.restype = _VP
    L.new_random_gate_bootstrapping_secret_keyset.restype = _VP
    L.new_random_gate_bootstrapping_secret_keyset.argtypes = [_VP]
    L.delete_gate_bootstrapping_secret_keyset.argtypes = [_VP]
    L.delete_gate_bootstrapping_parameters.argtypes = [_VP]
    L.tfhe_amd_export_bk.argtypes = [_VP, _I32P]
    L.tfhe_amd_export_ksk.argtypes = [_VP, _I32P]
    L.tfhe_amd_export_lwe_key.argtypes = [_VP, _I32P]
    L.tfhe_amd_export_tlwe_key.argtypes = [_VP, _I32P]
    L.tfhe_amd_context_create_raw.argtypes = [_I32P, _I32P, ctypes.c_int, ctypes.POINTER(_VP)]
    L.tfhe_amd_context_create.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(_VP)]
    L.tfhe_amd_context_destroy.argtypes = [_VP]
    L.tfhe_amd_context_stream.restype = _VP
    L.tfhe_amd_context_stream.argtypes = [_VP]
    L.tfhe_amd_sync.argtypes = [_VP]
    L.tfhe_amd_reserve.argtypes = [_VP, ctypes.c_int]
    for f in ("tfhe_amd_gate_batch_dev",):
        getattr(L, f).argtypes = [_VP, ctypes.c_int, ctypes.c_int] + [_VP] * 8 + [_VP]
    L.tfhe_amd_gate_batch_host.argtypes = [_VP, ctypes.c_int, ctypes.c_int] + [_I32P] * 8
    L.tfhe_amd_host_alloc.restype = _VP
    L.tfhe_amd_host_alloc.argtypes = [ctypes.c_size_t]
    L.tfhe_amd_host_free.argtypes = [_VP]
    L.tfhe_amd_host_is_pinned.argtypes = [_VP, ctypes.c_size_t]
    L.tfhe_amd_gate_batch_mixed_host.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_int)] + [_I32P] * 8
    L.tfhe_amd_bootstrap_woks_batch_dev.argtypes = [_VP, ctypes.c_int, ctypes.c_int32] + [_VP] * 4 + [_VP]
    L.tfhe_amd_bootstrap_batch_dev.argtypes = [_VP, ctypes.c_int, ctypes.c_int32] + [_VP] * 4 + [_VP]
    L.tfhe_amd_keyswitch_batch_dev.argtypes = [_VP, ctypes.c_int] + [_VP] * 4 + [_VP]
    L.tfhe_amd_bootstrap_woks_batch_host.argtypes = [_VP, ctypes.c_int, ctypes.c_int32] + [_I32P] * 4
    L.tfhe_amd_bootstrap_batch_host.argtypes = [_VP, ctypes.c_int, ctypes.c_int32] + [_I32P] * 4
    L.tfhe_amd_keyswitch_batch_host.argtypes = [_VP, ctypes.c_int] + [_I32P] * 4
    L.tfhe_amd_lut_fill.argtypes = [_I32P, ctypes.c_int, _I32P]
    for f in ("tfhe_amd_bootstrap_lut_woks_batch_dev", "tfhe_amd_bootstrap_lut_batch_dev"):
        getattr(L, f).argtypes = ([_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int32, ctypes.c_int32, _VP, _VP,
                                   ctypes.c_int32] + [_VP] * 4 + [_VP])
    for f in ("tfhe_amd_bootstrap_lut_woks_batch_host", "tfhe_amd_bootstrap_lut_batch_host"):
        getattr(L, f).argtypes = ([_VP, ctypes.c_int, ctypes.c_int, _I32P, _I32P, ctypes.c_int32, ctypes.c_int32, _I32P,
                                   _I32P, ctypes.c_int32] + [_I32P] * 4)
    L.tfhe_amd_lut_fill_many.argtypes = [_I32P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _I32P]
    for f in ("tfhe_amd_bootstrap_lut_many_woks_batch_dev", "tfhe_amd_bootstrap_lut_many_batch_dev"):
        getattr(L, f).argtypes = ([_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int32, ctypes.c_int32, _VP, _VP, ctypes.c_int32] + [_VP] * 4 + [_VP])
    for f in ("tfhe_amd_bootstrap_lut_many_woks_batch_host", "tfhe_amd_bootstrap_lut_many_batch_host"):
        getattr(L, f).argtypes = ([_VP, ctypes.c_int, ctypes.c_int, _I32P, _I32P, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int32, ctypes.c_int32, _I32P, _I32P, ctypes.c_int32] + [_I32P] * 4)
    L.tfhe_amd_full_add_table.argtypes = [_I32P, ctypes.c_int, ctypes.c_int]
    L.tfhe_amd_full_add_batch_dev.argtypes = [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_VP] * 8 + [_VP]
    L.tfhe_amd_full_add_batch_host.argtypes = [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_I32P] * 8
    L.tfhe_amd_blind_rotate_dev.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]
    L.tfhe_amd_external_product_dev.argtypes = [_VP, ctypes.c_int, _VP, _VP, _VP]
    L.tfhe_amd_context_create_replica.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(_VP)]
    L.tfhe_amd_context_key_digest.argtypes = [_VP, ctypes.POINTER(ctypes.c_ulonglong)]
    L.tfhe_amd_profile_enable.argtypes = [_VP, ctypes.c_int]
    L.tfhe_amd_profile_read.argtypes = [_VP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    L.tfhe_amd_guard_stats.argtypes = [_VP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong),
                                       ctypes.c_int]
    L.tfhe_amd_set_guard_threshold.argtypes = [ctypes.c_double]
    L.tfhe_amd_fp64_ceiling.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, _VP, _VP]
    L.tfhe_amd_tier1_lane_count.argtypes = [_VP]
    L.tfhe_amd_last_kernels.argtypes = [_VP, ctypes.c_char_p, ctypes.c_int]
    L.tfhe_amd_context_key_bytes.restype = ctypes.c_longlong
    L.tfhe_amd_context_key_bytes.argtypes = [_VP]
    L.tfhe_amd_multi_create_raw.argtypes = [_I32P, _I32P, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                            ctypes.POINTER(_VP)]
    L.tfhe_amd_multi_create.argtypes = [_VP, ctypes.c_int, ctypes.POINTER(_VP)]
    L.tfhe_amd_multi_destroy.argtypes = [_VP]
    L.tfhe_amd_multi_devices.argtypes = [_VP, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.tfhe_amd_multi_context.restype = _VP
    L.tfhe_amd_multi_context.argtypes = [_VP, ctypes.c_int]
    L.tfhe_amd_multi_gate_batch_host.argtypes = [_VP, ctypes.c_int, ctypes.c_int] + [_I32P] * 8
    L.tfhe_amd_shard_range.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    L.tfhe_gpu_init.argtypes = [_VP, ctypes.c_int]
    L.tfhe_gpu_boots_batch.argtypes = [ctypes.c_int] + [_I32P] * 8 + [ctypes.c_int, _VP]
    L.tfhe_random_generator_setSeed.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]
    L.modSwitchToTorus32.restype = ctypes.c_int32
    L.modSwitchFromTorus32.restype = ctypes.c_int
    L.lwePhase.restype = ctypes.c_int32
    # tfhe_io.h (FILE* entry points)
    for f in ("export_tfheGateBootstrappingSecretKeySet_toFile", "export_tfheGateBootstrappingCloudKeySet_toFile",
              "export_tfheGateBootstrappingParameterSet_toFile"):
        getattr(L, f).argtypes = [_VP, _VP]
    for f in ("new_tfheGateBootstrappingSecretKeySet_fromFile", "new_tfheGateBootstrappingCloudKeySet_fromFile",
              "new_tfheGateBootstrappingParameterSet_fromFile"):
        getattr(L, f).argtypes = [_VP]
        getattr(L, f).restype = _VP
    L.export_gate_bootstrapping_ciphertext_toFile.argtypes = [_VP, _VP, _VP]
    L.import_gate_bootstrapping_ciphertext_fromFile.argtypes = [_VP, _VP, _VP]
    L.new_gate_bootstrapping_ciphertext_array.argtypes = [ctypes.c_int, _VP]
    L.new_gate_bootstrapping_ciphertext_array.restype = _VP
    L.delete_gate_bootstrapping_ciphertext_array.argtypes = [ctypes.c_int, _VP]
    L.delete_gate_bootstrapping_cloud_keyset.argtypes = [_VP]
    # leveled mode (tfhe_amd_tgsw_*)
    L.tfhe_amd_tgsw_encrypt_bits.argtypes = [_VP, ctypes.c_int, _I32P, _I32P]
    L.tfhe_amd_tlwe_encrypt_polys.argtypes = [_VP, ctypes.c_int, _I32P, _I32P]
    L.tfhe_amd_tgsw_import.argtypes = [_VP, ctypes.c_int, _I32P, ctypes.POINTER(_VP)]
    L.tfhe_amd_tgsw_count.argtypes = [_VP]
    L.tfhe_amd_tgsw_destroy.argtypes = [_VP]
    L.tfhe_amd_tgsw_cmux_dev.argtypes = [_VP, _VP, ctypes.c_int] + [_VP] * 4 + [_VP]
    for f in ("tfhe_amd_tgsw_lookup_woks_dev", "tfhe_amd_tgsw_lookup_dev"):
        getattr(L, f).argtypes = ([_VP, _VP, ctypes.c_int, ctypes.c_int, _VP] + [ctypes.c_int] * 3 + [_VP, _VP]
                                  + [ctypes.c_int] * 2 + [_VP, _VP, _VP])
    for f in ("tfhe_amd_tgsw_lookup_woks_host", "tfhe_amd_tgsw_lookup_host"):
        getattr(L, f).argtypes = ([_VP, _VP, ctypes.c_int, ctypes.c_int, _I32P] + [ctypes.c_int] * 3 + [_I32P, _I32P]
                                  + [ctypes.c_int] * 2 + [_I32P, _I32P])
    # leveled automata (tfhe_amd_dfa_*)
    L.tfhe_amd_dfa_create.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _I32P, ctypes.c_int, ctypes.POINTER(_VP)]
    L.tfhe_amd_dfa_destroy.argtypes = [_VP]
    L.tfhe_amd_dfa_info.argtypes = [_VP] + [ctypes.POINTER(ctypes.c_int)] * 4
    L.tfhe_amd_dfa_live.argtypes = [_VP, ctypes.c_int, _I32P]
    for f in ("tfhe_amd_dfa_run_woks_dev", "tfhe_amd_dfa_run_dev"):
        getattr(L, f).argtypes = ([_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP,
                                   ctypes.c_int, _VP, _VP, _VP])
    for f in ("tfhe_amd_dfa_run_woks_host", "tfhe_amd_dfa_run_host"):
        getattr(L, f).argtypes = ([_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _I32P, ctypes.c_int, ctypes.c_int, _I32P,
                                   _I32P, ctypes.c_int, _I32P, _I32P])
    L.tfhe_amd_dfa_build_compare.argtypes = [_I32P, ctypes.POINTER(ctypes.c_int), _I32P]
    L.tfhe_amd_dfa_build_contains.argtypes = [ctypes.c_int, _I32P, _I32P, ctypes.POINTER(ctypes.c_int)]
    L.tfhe_amd_dfa_build_at_least.argtypes = [ctypes.c_int, _I32P, ctypes.POINTER(ctypes.c_int)]
    L.tfhe_amd_dfa_fin_fill.argtypes = [ctypes.c_int, ctypes.c_int, _I32P, _I32P]
    L.tfhe_amd_dfa_simulate.argtypes = [ctypes.c_int, ctypes.c_int, _I32P, ctypes.c_int, _I32P]
    # weighted runs of a leveled automaton (tfhe_amd_wfa_*)
    for f in ("tfhe_amd_wfa_run_woks_dev", "tfhe_amd_wfa_run_dev"):
        getattr(L, f).argtypes = ([_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, ctypes.c_int, ctypes.c_int,
                                   _VP, _VP, ctypes.c_int, _VP, _VP, _VP])
    for f in ("tfhe_amd_wfa_run_woks_host", "tfhe_amd_wfa_run_host"):
        getattr(L, f).argtypes = ([_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _I32P, _I32P, _I32P, ctypes.c_int,
                                   ctypes.c_int, _I32P, _I32P, ctypes.c_int, _I32P, _I32P])
    L.tfhe_amd_wfa_build_max.argtypes = [ctypes.c_int, ctypes.c_int, _I32P, ctypes.POINTER(ctypes.c_int), _I32P, _I32P]
    L.tfhe_amd_wfa_build_popcount.argtypes = [ctypes.c_int, ctypes.c_int, _I32P, ctypes.POINTER(ctypes.c_int), _I32P, _I32P]
    L.tfhe_amd_wfa_build_first_one.argtypes = [ctypes.c_int, _I32P, ctypes.POINTER(ctypes.c_int), _I32P, _I32P]
    L.tfhe_amd_wfa_fin_fill.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int32, _I32P]
    L.tfhe_amd_wfa_simulate.argtypes = [ctypes.c_int, ctypes.c_int, _I32P, _I32P, _I32P, ctypes.c_int, _I32P, _I32P]
    # packing key switch (tfhe_amd_pack_*)
    L.tfhe_amd_pack_key_generate.argtypes = [_VP, _I32P]
    L.tfhe_amd_tlwe_phase_polys.argtypes = [_VP, ctypes.c_int, _I32P, _I32P]
    L.tfhe_amd_pack_key_import.argtypes = [_VP, _I32P, ctypes.POINTER(_VP)]
    L.tfhe_amd_pack_key_destroy.argtypes = [_VP]
    L.tfhe_amd_pack_dev.argtypes = [_VP, _VP, ctypes.c_int, ctypes.c_int] + [_VP] * 4 + [_VP]
    L.tfhe_amd_pack_host.argtypes = [_VP, _VP, ctypes.c_int, ctypes.c_int] + [_I32P] * 4
    # bootstrap from encrypted accumulators (tfhe_amd_tlwe_box_fill_*, tfhe_amd_bootstrap_acc_*, tfhe_amd_select_*)
    L.tfhe_amd_tlwe_box_fill_dev.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]
    L.tfhe_amd_tlwe_box_fill_host.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _I32P, _I32P]
    for f in ("tfhe_amd_bootstrap_acc_woks_batch_dev", "tfhe_amd_bootstrap_acc_batch_dev"):
        getattr(L, f).argtypes = ([_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int32, ctypes.c_int32, _VP, _VP,
                                   ctypes.c_int32] + [_VP] * 4 + [_VP])
    for f in ("tfhe_amd_bootstrap_acc_woks_batch_host", "tfhe_amd_bootstrap_acc_batch_host"):
        getattr(L, f).argtypes = ([_VP, ctypes.c_int, ctypes.c_int, _I32P, _I32P, ctypes.c_int32, ctypes.c_int32, _I32P,
                                   _I32P, ctypes.c_int32] + [_I32P] * 4)
    L.tfhe_amd_select_batch_dev.argtypes = ([_VP, _VP, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int32,
                                             ctypes.c_int32] + [_VP] * 4 + [_VP])
    L.tfhe_amd_select_batch_host.argtypes = ([_VP, _VP, ctypes.c_int, ctypes.c_int, _I32P, _I32P, ctypes.c_int32,
                                              ctypes.c_int32] + [_I32P] * 4)
    return L


lib = _load()


def version():
    return lib.tfhe_amd_version().decode()


def select_kernel(generation):
    """tfhe_amd_select_kernel: blind-rotation kernel generation (0 = default v6, 4 = exact NTT;
    EXPERIMENTAL=1 builds also 1, 2, 3, 5, 7) for A/B runs and cross-checks."""
    _check(lib.tfhe_amd_select_kernel(int(generation)), "select_kernel")


def available_kernels():
    """The blind-rotation generations this build of the library carries (selection restored)."""
    cur = version().split("br-v")[1].split(" ")[0]
    out = [v for v in range(1, 8) if lib.tfhe_amd_select_kernel(v) == 0]
    lib.tfhe_amd_select_kernel(int(cur) if cur.isdigit() else 0)
    return out


def fp64_ceiling(device=0, waves_per_simd=2, seconds=2.0):
    """tfhe_amd_fp64_ceiling: (TFLOP/s, MHz) of register-operand fp64 FMA chains on every SIMD
    for ~seconds: the fp64 rate the device sustains under its power limit (bench roofline)."""
    tf, mhz = ctypes.c_double(), ctypes.c_double()
    _check(lib.tfhe_amd_fp64_ceiling(int(device), int(waves_per_simd), float(seconds), ctypes.byref(tf),
                                     ctypes.byref(mhz)), "fp64_ceiling")
    return tf.value, mhz.value


def set_guard_threshold(distance):
    """tfhe_amd_set_guard_threshold: rounding distance at which the fp64 kernel's results are
    recomputed by the exact NTT kernel (default 1/8, the loosest allowed; 0 recomputes everything)."""
    _check(lib.tfhe_amd_set_guard_threshold(float(distance)), "set_guard_threshold")


def _p(a):
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(_I32P)


def _check(rc, what):
    if rc != 0:
        raise TfheAmdError(f"{what} failed with code {rc}")


def i32(x):
    """int32, C-contiguous view of x: the array itself when it already is one (the host batch paths
    then read the caller's memory directly instead of a fresh copy per call — 2 copies of every
    input, ~0.3 ms per 1 024-gate call), else a copy with the values reduced mod 2^32."""
    a = np.asarray(x)
    if a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]:
        return a
    return np.ascontiguousarray(a.astype(np.int64).astype(np.int32))


# ---- programmable bootstrapping: the encoding convention of include/tfhe_amd.h (tfhe_amd_lut_fill)

def _lut_p(p):
    p = int(p)
    if p < 1 or p > N or p & (p - 1):
        raise TfheAmdError(f"p must be a power of two in [1, {N}], got {p}")
    return p


def lut_encode(m, p):
    """Torus32 of message m in [0, p): (2m + 1) / (4p), the centre of box m of the half torus."""
    p = _lut_p(p)
    m = np.asarray(m, dtype=np.int64)
    if np.any((m < 0) | (m >= p)):
        raise TfheAmdError(f"message outside [0, {p})")
    return ((2 * m + 1) * ((1 << 30) // p)).astype(np.int32)


def lut_decode(phase, p):
    """The box of the half torus a phase (Torus32) lies in: floor(2p phase), the message when it is
    in [0, p); values in [p, 2p) mean the phase left the half torus [0, 1/2)."""
    p = _lut_p(p)
    ph = np.asarray(phase).astype(np.int64) & 0xFFFFFFFF
    return (ph * p) >> 31


def lut_table(p, values):
    """tfhe_amd_lut_fill: the test vector int32 [1024] with tv[j] = values[floor(j p / N)], so an
    input encoding m (lut_encode(m, p)) bootstraps to values[m] (Torus32 words, e.g.
    lut_encode(f(m), p2))."""
    v = np.ascontiguousarray(np.asarray(values).astype(np.int64).astype(np.int32))
    if v.ndim != 1 or v.shape[0] != int(p):
        raise TfheAmdError(f"values: need {p} Torus32 words, got shape {v.shape}")
    tv = np.zeros(N, np.int32)
    _check(lib.tfhe_amd_lut_fill(_p(tv), int(p), _p(v)), "lut_fill")
    return tv


def lut_table_many(p, values, log_nu):
    """tfhe_amd_lut_fill_many: the test vector int32 [1024] that interleaves the n_fn <= 2^log_nu
    functions values [n_fn][p] (Torus32 words), tv[j] = values[j mod nu][floor(j p / N)] (0 where
    j mod nu >= n_fn), so output f of a many-LUT bootstrap at log_nu reads values[f][m]."""
    v = np.ascontiguousarray(np.asarray(values).astype(np.int64).astype(np.int32))
    if v.ndim != 2 or v.shape[0] < 1 or v.shape[1] != int(p):
        raise TfheAmdError(f"values: need [n_fn][{p}] Torus32 words, got shape {v.shape}")
    tv = np.zeros(N, np.int32)
    _check(lib.tfhe_amd_lut_fill_many(_p(tv), int(p), int(log_nu), v.shape[0], _p(v)), "lut_fill_many")
    return tv


# ---- one-rotation adder cells (include/tfhe_amd.h): the two encodings of a bit
ENC_GATE, ENC_HALF = 0, 1
H0, H1 = 1 << 28, 3 << 28   # half-torus bit 0 / 1: 1/16, 3/16 = lut_encode(m, 4)


def _enc(enc):
    return {"G": ENC_GATE, "H": ENC_HALF}.get(enc, enc) if isinstance(enc, str) else int(enc)


def half_encode(bits):
    """Torus32 of bits in the half-torus encoding: 1/16 for 0, 3/16 for 1"""
    return np.where(np.asarray(bits) != 0, H1, H0).astype(np.int32)


def half_decode(phase):
    """the bit of a half-torus phase: box 0 or 1 of lut_decode(phase, 4); anything else means the
    phase left the two boxes"""
    return lut_decode(phase, 4)


def full_add_table(enc_sum, enc_carry):
    """tfhe_amd_full_add_table: the adder cell's test vector int32 [1024] for outputs in
    (enc_sum, enc_carry)"""
    tv = np.zeros(N, np.int32)
    _check(lib.tfhe_amd_full_add_table(_p(tv), _enc(enc_sum), _enc(enc_carry)), "full_add_table")
    return tv


class _PinnedBlock:
    """one tfhe_amd_host_alloc buffer, freed when the last array viewing it goes"""

    def __init__(self, nbytes):
        self.ptr = lib.tfhe_amd_host_alloc(max(1, nbytes))
        if not self.ptr:
            raise TfheAmdError(f"tfhe_amd_host_alloc({nbytes}) failed")

    def __del__(self):
        if getattr(self, "ptr", None) and lib is not None:
            lib.tfhe_amd_host_free(self.ptr)
            self.ptr = None


def host_empty(shape, dtype=np.int32):
    """A numpy array in caller-owned pinned host memory (tfhe_amd_host_alloc).  Host batch calls
    whose arrays are all such arrays DMA straight from and into them, with no staging copy."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    blk = _PinnedBlock(n)
    buf = (ctypes.c_char * max(1, n)).from_address(blk.ptr)
    buf._owner = blk
    return np.frombuffer(buf, dtype=dt, count=n // dt.itemsize).reshape(shape)


def host_copy(x, dtype=np.int32):
    """x copied into a new pinned array (host_empty)"""
    a = np.asarray(x)
    out = host_empty(a.shape, dtype)
    out[...] = a
    return out


def is_pinned(a):
    """whether the array's bytes lie inside one tfhe_amd_host_alloc buffer"""
    a = np.asarray(a)
    return bool(lib.tfhe_amd_host_is_pinned(a.ctypes.data, a.nbytes))


# --------------------------------------------------------------------- files (tfhe_io.h)

_libc = ctypes.CDLL(None)
_libc.fopen.restype = _VP
_libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_libc.fclose.argtypes = [_VP]


class _File:
    """FILE* for the tfhe_io.h entry points (they take C stdio streams, like the reference)."""

    def __init__(self, path, mode):
        self.f = _libc.fopen(os.fsencode(path), mode.encode())
        if not self.f:
            raise OSError(f"cannot open {path} ({mode})")

    def __enter__(self):
        return self.f

    def __exit__(self, *exc):
        _libc.fclose(self.f)


class LweSampleC(ctypes.Structure):
    """struct LweSample (lwesamples.h:18-29)."""
    _fields_ = [("a", _I32P), ("b", ctypes.c_int32), ("current_variance", ctypes.c_double)]


def write_ciphertexts(path, params, a, b, variance=0.0, mode="wb"):
    """export_gate_bootstrapping_ciphertext_toFile for each row of the SoA batch (a [B][n], b [B])."""
    a = i32(a); b = i32(b); B = a.shape[0]
    arr = lib.new_gate_bootstrapping_ciphertext_array(B, params)
    try:
        s = (LweSampleC * B).from_address(arr)
        with _File(path, mode) as f:
            for i in range(B):
                ctypes.memmove(s[i].a, a[i].ctypes.data, 4 * n_lwe)
                s[i].b = int(b[i]); s[i].current_variance = float(variance)
                lib.export_gate_bootstrapping_ciphertext_toFile(f, ctypes.byref(s[i]), params)
    finally:
        lib.delete_gate_bootstrapping_ciphertext_array(B, arr)


def read_ciphertexts(path, params, B):
    """import_gate_bootstrapping_ciphertext_fromFile B times -> (a [B][n], b [B], variance [B])."""
    arr = lib.new_gate_bootstrapping_ciphertext_array(B, params)
    a = np.zeros((B, n_lwe), np.int32); b = np.zeros(B, np.int32); v = np.zeros(B)
    try:
        s = (LweSampleC * B).from_address(arr)
        with _File(path, "rb") as f:
            for i in range(B):
                lib.import_gate_bootstrapping_ciphertext_fromFile(f, ctypes.byref(s[i]), params)
                ctypes.memmove(a[i].ctypes.data, s[i].a, 4 * n_lwe)
                b[i] = s[i].b; v[i] = s[i].current_variance
    finally:
        lib.delete_gate_bootstrapping_ciphertext_array(B, arr)
    return a, b, v


# --------------------------------------------------------------------- keys (host)

class SecretKeyset:
    """new_random_gate_bootstrapping_secret_keyset (tfhe_gate_bootstrapping.cu:57-68) seeded
    through tfhe_random_generator_setSeed; exposes the key material as numpy arrays."""

    def __init__(self, seed=(314, 1592, 657), path=None):
        """seeded keygen, or (path=...) new_tfheGateBootstrappingSecretKeySet_fromFile."""
        if path is None:
            s = (ctypes.c_uint32 * len(seed))(*seed)
            lib.tfhe_random_generator_setSeed(s, len(seed))
            self.own_params = lib.new_default_gate_bootstrapping_parameters(110)
            self.h = lib.new_random_gate_bootstrapping_secret_keyset(self.own_params)
        else:
            self.own_params = None            # belongs to the keyset read from the file
            with _File(path, "rb") as f:
                self.h = lib.new_tfheGateBootstrappingSecretKeySet_fromFile(f)
        if not self.h:
            raise TfheAmdError("keygen failed")
        self.params = ctypes.c_void_p.from_address(self.h).value     # key->params
        self.bk = np.zeros((n_lwe, KPL, 2, N), np.int32)
        self.ksk = np.zeros((N, KS_T, KS_BASE, n_lwe + 1), np.int32)
        self.lwe_key = np.zeros(n_lwe, np.int32)
        _check(lib.tfhe_amd_export_bk(ctypes.c_void_p(self._cloud()), _p(self.bk)), "export_bk")
        _check(lib.tfhe_amd_export_ksk(ctypes.c_void_p(self._cloud()), _p(self.ksk)), "export_ksk")
        _check(lib.tfhe_amd_export_lwe_key(ctypes.c_void_p(self.h), _p(self.lwe_key)), "export_lwe_key")
        self.tlwe_key = np.zeros(N, np.int32)
        _check(lib.tfhe_amd_export_tlwe_key(ctypes.c_void_p(self.h), _p(self.tlwe_key)), "export_tlwe_key")

    def save(self, path):
        """export_tfheGateBootstrappingSecretKeySet_toFile"""
        with _File(path, "wb") as f:
            lib.export_tfheGateBootstrappingSecretKeySet_toFile(f, self.h)

    def save_cloud(self, path):
        """export_tfheGateBootstrappingCloudKeySet_toFile(F, &key->cloud)"""
        with _File(path, "wb") as f:
            lib.export_tfheGateBootstrappingCloudKeySet_toFile(f, self._cloud())

    def _cloud(self):
        # &key->cloud: TFheGateBootstrappingSecretKeySet = {params*, lwe_key*, tgsw_key*, cloud}
        return self.h + 3 * ctypes.sizeof(ctypes.c_void_p)

    @property
    def cloud(self):
        return self._cloud()

    def close(self):
        if self.h:
            lib.delete_gate_bootstrapping_secret_keyset(self.h)
            self.h = None
        if self.own_params:
            lib.delete_gate_bootstrapping_parameters(self.own_params)
            self.own_params = None

    # numpy-side encryption with the same secret (fast path for big batches; the product's
    # bootsSymEncrypt is covered by its own test)
    def encrypt(self, bits, rng, stdev=2.4349504419032758e-05):
        bits = np.asarray(bits).astype(np.int64)
        B = bits.shape[0]
        a = rng.integers(-2**31, 2**31, (B, n_lwe), dtype=np.int64)
        mu = np.where(bits != 0, MU, -MU)
        noise = np.rint(rng.normal(0.0, stdev, B) * 2**32).astype(np.int64)
        b = (a @ self.lwe_key.astype(np.int64) + mu + noise)
        return i32(a), i32(b)

    def encrypt_digits(self, m, p, rng, stdev=2.4349504419032758e-05):
        """fresh encryptions of messages m in [0, p) at the programmable bootstrap's encoding
        (lut_encode: (2m + 1) / (4p))."""
        mu = lut_encode(m, p).astype(np.int64)
        B = mu.shape[0]
        a = rng.integers(-2**31, 2**31, (B, n_lwe), dtype=np.int64)
        noise = np.rint(rng.normal(0.0, stdev, B) * 2**32).astype(np.int64)
        b = (a @ self.lwe_key.astype(np.int64) + mu + noise)
        return i32(a), i32(b)

    def phase(self, a, b):
        a = np.asarray(a).astype(np.int64)
        ph = (np.asarray(b).astype(np.int64) - a @ self.lwe_key.astype(np.int64)) & 0xFFFFFFFF
        return ph.astype(np.uint32).view(np.int32)

    def decrypt(self, a, b):
        return (self.phase(a, b) > 0).astype(np.int32)

    def phase_extracted(self, u_a, u_b):
        """phase of a woKS output (dimension N) under the extracted key (tLweExtractKey)."""
        u_a = np.asarray(u_a).astype(np.int64)
        ph = (np.asarray(u_b).astype(np.int64) - u_a @ self.tlwe_key.astype(np.int64)) & 0xFFFFFFFF
        return ph.astype(np.uint32).view(np.int32)

    # ---- client side of the leveled mode (tfhe_amd_tgsw_*; the library's generator, so
    # tfhe_random_generator_setSeed / a fresh SecretKeyset(seed) makes them reproducible)
    def tgsw_encrypt(self, bits):
        """tfhe_amd_tgsw_encrypt_bits: TGSW encryptions of bits in {0, 1} -> [n][4][2][1024], the
        layout of one entry of bk (Context.tgsw_import takes it)"""
        bits = i32(np.asarray(bits).reshape(-1))
        out = np.zeros((bits.shape[0], KPL, 2, N), np.int32)
        _check(lib.tfhe_amd_tgsw_encrypt_bits(self.h, bits.shape[0], _p(bits), _p(out)), "tgsw_encrypt_bits")
        return out

    def tlwe_encrypt(self, polys):
        """tfhe_amd_tlwe_encrypt_polys: TLWE encryptions of message polynomials [n][1024] (or one
        [1024]) -> [n][2][1024] (a, then b)"""
        mu = i32(polys).reshape(-1, N)
        out = np.zeros((mu.shape[0], 2, N), np.int32)
        _check(lib.tfhe_amd_tlwe_encrypt_polys(self.h, mu.shape[0], _p(mu), _p(out)), "tlwe_encrypt_polys")
        return out

    # ---- client side of the packing key switch (tfhe_amd_pack_*)
    def pack_key(self):
        """tfhe_amd_pack_key_generate: the LWE -> TLWE packing key [500][6][2][1024]
        (Context.pack_key_import takes it)"""
        out = np.zeros((n_lwe, PACK_T, 2, N), np.int32)
        _check(lib.tfhe_amd_pack_key_generate(self.h, _p(out)), "pack_key_generate")
        return out

    def tlwe_phase(self, polys):
        """tfhe_amd_tlwe_phase_polys: TLWE samples [n][2][1024] (or one [2][1024]) -> phases
        b - a s [n][1024] under the keyset's TLWE key"""
        x = i32(polys).reshape(-1, 2, N)
        out = np.zeros((x.shape[0], N), np.int32)
        _check(lib.tfhe_amd_tlwe_phase_polys(self.h, x.shape[0], _p(x), _p(out)), "tlwe_phase_polys")
        return out


class CloudKeyset:
    """new_tfheGateBootstrappingCloudKeySet_fromFile (tfhe_io.cu:1117): what cloud.cpp loads."""

    def __init__(self, path):
        with _File(path, "rb") as f:
            self.h = lib.new_tfheGateBootstrappingCloudKeySet_fromFile(f)
        if not self.h:
            raise TfheAmdError(f"cannot read cloud key {path}")
        self.params = ctypes.c_void_p.from_address(self.h).value      # bk->params

    def save(self, path):
        with _File(path, "wb") as f:
            lib.export_tfheGateBootstrappingCloudKeySet_toFile(f, self.h)

    def export_bk(self):
        bk = np.zeros((n_lwe, KPL, 2, N), np.int32)
        _check(lib.tfhe_amd_export_bk(ctypes.c_void_p(self.h), _p(bk)), "export_bk")
        return bk

    def export_ksk(self):
        ksk = np.zeros((N, KS_T, KS_BASE, n_lwe + 1), np.int32)
        _check(lib.tfhe_amd_export_ksk(ctypes.c_void_p(self.h), _p(ksk)), "export_ksk")
        return ksk

    def close(self):
        if self.h:
            lib.delete_gate_bootstrapping_cloud_keyset(self.h)
            self.h = None


# --------------------------------------------------------------------- device context

class TgswSet:
    """TfheAmdTgsw: caller-supplied TGSW samples imported to a context's device
    (Context.tgsw_import); close() frees them.  It does not depend on the context's lifetime."""

    def __init__(self, h, device):
        self.h, self.device = h, device

    def __len__(self):
        return int(lib.tfhe_amd_tgsw_count(self.h)) if self.h else 0

    def close(self):
        if getattr(self, "h", None):
            lib.tfhe_amd_tgsw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dfa:
    """TfheAmdDfa: a deterministic automaton over TGSW-encrypted bits on a context's device
    (Context.dfa_create), or a host-only one (Dfa.host: device -1, inspection only); close() frees
    it.  It does not depend on the context's lifetime."""

    def __init__(self, h):
        self.h = h
        v = [ctypes.c_int() for _ in range(4)]
        _check(lib.tfhe_amd_dfa_info(h, *[ctypes.byref(x) for x in v]), "dfa_info")
        self.n_states, self.start, self.max_len, self.device = (x.value for x in v)

    @classmethod
    def _create(cls, ctx_h, next, start, max_len):
        next = i32(next)
        if next.ndim != 2 or next.shape[1] != 2:
            raise TfheAmdError(f"next: need int32 [n_states][2], got {next.shape}")
        h = _VP()
        _check(lib.tfhe_amd_dfa_create(ctx_h, next.shape[0], int(start), _p(next), int(max_len), ctypes.byref(h)),
               "dfa_create")
        return cls(h.value)

    @classmethod
    def host(cls, next, start, max_len):
        """tfhe_amd_dfa_create without a context: the live sets can be read, no run accepts it"""
        return cls._create(None, next, start, max_len)

    def live(self, step):
        """tfhe_amd_dfa_live: the states reachable from the start state after `step` bits, ascending"""
        out = np.zeros(self.n_states, np.int32)
        n = lib.tfhe_amd_dfa_live(self.h, int(step), _p(out))
        if n < 0:
            raise TfheAmdError(f"dfa_live failed with code {n}")
        return out[:n]

    def close(self):
        if getattr(self, "h", None):
            lib.tfhe_amd_dfa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DFA_LT, DFA_EQ, DFA_GT, DFA_MID = 0, 1, 2, 3


def _dfa_built(n, what):
    if n < 0:
        raise TfheAmdError(f"{what} failed with code {n}")
    return n


def dfa_compare():
    """tfhe_amd_dfa_build_compare: x against y over the word x_{d-1}, y_{d-1}, ..., x_0, y_0 ->
    (next [5][2], start, cls [5] of DFA_LT / DFA_EQ / DFA_GT / DFA_MID)"""
    next, cls, start = np.zeros((5, 2), np.int32), np.zeros(5, np.int32), ctypes.c_int()
    _dfa_built(lib.tfhe_amd_dfa_build_compare(_p(next), ctypes.byref(start), _p(cls)), "dfa_build_compare")
    return next, start.value, cls


def dfa_contains(pattern):
    """tfhe_amd_dfa_build_contains: the KMP automaton of a bit pattern (first bit first) ->
    (next [m + 1][2], start); state m: the word contains the pattern"""
    pattern = i32(np.asarray(pattern).reshape(-1))
    next, start = np.zeros((pattern.shape[0] + 1, 2), np.int32), ctypes.c_int()
    _dfa_built(lib.tfhe_amd_dfa_build_contains(pattern.shape[0], _p(pattern), _p(next), ctypes.byref(start)),
               "dfa_build_contains")
    return next, start.value


def dfa_at_least(t):
    """tfhe_amd_dfa_build_at_least: a saturating count of ones -> (next [t + 1][2], start); state t:
    at least t bits are set"""
    t = int(t)
    next, start = np.zeros((max(t, 0) + 1, 2), np.int32), ctypes.c_int()
    _dfa_built(lib.tfhe_amd_dfa_build_at_least(t, _p(next), ctypes.byref(start)), "dfa_build_at_least")
    return next, start.value


def dfa_fin(values):
    """tfhe_amd_dfa_fin_fill: values [n_states][n_out] Torus32 -> the plaintext final weights
    [1][n_states][1][1024] (one table, fin_rows = 1)"""
    values = i32(values)
    if values.ndim == 1:
        values = np.ascontiguousarray(values[:, None])
    fin = np.zeros((1, values.shape[0], 1, N), np.int32)
    _check(lib.tfhe_amd_dfa_fin_fill(values.shape[0], values.shape[1], _p(values), _p(fin)), "dfa_fin_fill")
    return fin


def dfa_simulate(next, start, bits):
    """tfhe_amd_dfa_simulate: the state after the plain word bits (bit 0 first)"""
    next, bits = i32(next), i32(np.asarray(bits).reshape(-1))
    return _dfa_built(lib.tfhe_amd_dfa_simulate(next.shape[0], int(start), _p(next), bits.shape[0], _p(bits)),
                      "dfa_simulate")


def _wfa_fin(n_states, n_out, value):
    fin = np.zeros((1, n_states, 1, N), np.int32)
    _check(lib.tfhe_amd_wfa_fin_fill(n_states, n_out, int(value), _p(fin)), "wfa_fin_fill")
    return fin


def wfa_max(d, want_max=True):
    """tfhe_amd_wfa_build_max: max (or min) of two d-bit integers over the word x_{d-1}, y_{d-1}, ...,
    x_0, y_0 -> (next [7][2], start, (w_val [7][2], w_pos [2 d]), fin [1][7][1][1024]); with n_out = d
    output f is bit f of the result as +-1/8"""
    d = int(d)
    next, w_val, w_pos, start = (np.zeros((7, 2), np.int32), np.zeros((7, 2), np.int32),
                                 np.zeros(2 * max(d, 1), np.int32), ctypes.c_int())
    _dfa_built(lib.tfhe_amd_wfa_build_max(d, int(bool(want_max)), _p(next), ctypes.byref(start), _p(w_val), _p(w_pos)),
               "wfa_build_max")
    return next, start.value, (w_val, w_pos), _wfa_fin(7, d, -(1 << 29))


def wfa_popcount(length, p):
    """tfhe_amd_wfa_build_popcount: the number of set bits of a word of `length` <= p - 1 bits as a LUT
    digit modulo p -> (next [1][2], start, (w_val [1][2], w_pos [length]), fin [1][1][1][1024]); the
    single output is the digit (2 c + 1) / (4 p) of the count c"""
    length, p = int(length), int(p)
    next, w_val, w_pos, start = (np.zeros((1, 2), np.int32), np.zeros((1, 2), np.int32),
                                 np.zeros(max(length, 1), np.int32), ctypes.c_int())
    _dfa_built(lib.tfhe_amd_wfa_build_popcount(length, p, _p(next), ctypes.byref(start), _p(w_val), _p(w_pos)),
               "wfa_build_popcount")
    return next, start.value, (w_val, w_pos), _wfa_fin(1, 1, (1 << 32) // (4 * p))


def wfa_first_one(length):
    """tfhe_amd_wfa_build_first_one: the one-hot position of the first set bit of a word of `length`
    <= 64 bits -> (next [2][2], start, (w_val [2][2], w_pos [length]), fin [1][2][1][1024]); with
    n_out = length output f is 1 (as +-1/8) exactly when bit f is the first set bit"""
    length = int(length)
    next, w_val, w_pos, start = (np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32),
                                 np.zeros(max(length, 1), np.int32), ctypes.c_int())
    _dfa_built(lib.tfhe_amd_wfa_build_first_one(length, _p(next), ctypes.byref(start), _p(w_val), _p(w_pos)),
               "wfa_build_first_one")
    return next, start.value, (w_val, w_pos), _wfa_fin(2, length, -(1 << 29))


def wfa_simulate(next, start, weights, bits):
    """tfhe_amd_wfa_simulate: (the state after the plain word bits, poly [1024] = the sum of the
    weights w_val[s_i][bit_i] X^{w_pos[i]} along its path); weights = (w_val, w_pos)"""
    next, bits = i32(next), i32(np.asarray(bits).reshape(-1))
    w_val, w_pos = i32(weights[0]), i32(np.asarray(weights[1]).reshape(-1))
    if w_val.shape != next.shape or w_pos.shape[0] < bits.shape[0]:
        raise TfheAmdError(f"need w_val {next.shape} and w_pos of at least {bits.shape[0]} entries, got {w_val.shape}, "
                           f"{w_pos.shape}")
    poly = np.zeros(N, np.int32)
    s = _dfa_built(lib.tfhe_amd_wfa_simulate(next.shape[0], int(start), _p(next), _p(w_val), _p(w_pos), bits.shape[0],
                                             _p(bits), _p(poly)), "wfa_simulate")
    return s, poly


class PackKey:
    """TfheAmdPackKey: the packing key imported to a context's device (Context.pack_key_import);
    close() frees it.  It does not depend on the context's lifetime."""

    def __init__(self, h, device):
        self.h, self.device = h, device

    def close(self):
        if getattr(self, "h", None):
            lib.tfhe_amd_pack_key_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _log2(n_poly):
    n_poly = int(n_poly)
    if n_poly not in (1, 2, 4, 8, 16):
        raise TfheAmdError(f"n_poly: need 1, 2, 4, 8 or 16, got {n_poly}")
    return n_poly.bit_length() - 1


class Context:
    """TfheAmdContext: key material of one cloud key on one GPU (tfhe_amd_context_create_raw)."""

    def __init__(self, bk, ksk, device=0):
        self.bk = i32(bk)
        self.ksk = i32(ksk)
        h = _VP()
        _check(lib.tfhe_amd_context_create_raw(_p(self.bk), _p(self.ksk), int(device), ctypes.byref(h)),
               "tfhe_amd_context_create_raw")
        self.h = h.value
        self.device = device

    @classmethod
    def replica_of(cls, src, device):
        """tfhe_amd_context_create_replica: src's converted device key copied device to device"""
        h = _VP()
        _check(lib.tfhe_amd_context_create_replica(src.h, int(device), ctypes.byref(h)), "context_create_replica")
        c = cls.__new__(cls)
        c.bk, c.ksk, c.h, c.device = src.bk, src.ksk, h.value, device
        return c

    def key_digest(self):
        """FNV-1a 64 of the context's device key bytes (tfhe_amd_context_key_digest)"""
        d = ctypes.c_ulonglong()
        _check(lib.tfhe_amd_context_key_digest(self.h, ctypes.byref(d)), "context_key_digest")
        return d.value

    def close(self):
        if getattr(self, "h", None):
            lib.tfhe_amd_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib.tfhe_amd_context_stream(self.h)

    def key_bytes(self):
        """device bytes of this context's key material (tfhe_amd_context_key_bytes)"""
        return int(lib.tfhe_amd_context_key_bytes(self.h))

    def sync(self):
        _check(lib.tfhe_amd_sync(self.h), "sync")

    def reserve(self, B):
        _check(lib.tfhe_amd_reserve(self.h, int(B)), "reserve")

    # ---- host (numpy) batches
    def gate_host(self, gate, ca_a, ca_b, cb_a, cb_b, cc_a=None, cc_b=None, out=None):
        """tfhe_amd_gate_batch_host; out = (r_a [B][500], r_b [B]) int32 arrays to reuse (else new ones).
        With every array pinned (host_empty / host_copy) the kernels read the inputs in place and the
        results are copied straight into `out`.  `out` must be C-contiguous: the library writes B x 500
        consecutive words (a strided view would be overwritten past its rows)."""
        g = GATES[gate] if isinstance(gate, str) else int(gate)
        ca_a = i32(ca_a); B = ca_a.shape[0]
        if out is not None:
            r_a, r_b = out
            if r_a.shape != (B, n_lwe) or r_b.shape != (B,) or r_a.dtype != np.int32 or r_b.dtype != np.int32:
                raise TfheAmdError("out: need int32 arrays [B][500] and [B]")
            if not (r_a.flags["C_CONTIGUOUS"] and r_b.flags["C_CONTIGUOUS"]):
                raise TfheAmdError("out: need C-contiguous arrays")
        else:
            r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_gate_batch_host(self.h, g, B, _p(r_a), _p(r_b), _p(ca_a), _p(i32(ca_b)),
                                            _p(i32(cb_a)), _p(i32(cb_b)),
                                            _p(None if cc_a is None else i32(cc_a)),
                                            _p(None if cc_b is None else i32(cc_b))), "gate_batch_host")
        return r_a, r_b

    def gate_mixed_host(self, gates, ca_a, ca_b, cb_a, cb_b, cc_a=None, cc_b=None):
        """tfhe_amd_gate_batch_mixed_host: gate i of kind gates[i] (names or codes) on row i, all in
        one blind-rotation and one key-switch launch."""
        g = np.array([GATES[x] if isinstance(x, str) else int(x) for x in gates], dtype=np.int32)
        ca_a = i32(ca_a); B = ca_a.shape[0]
        if g.shape != (B,):
            raise TfheAmdError(f"gates: need one gate kind per row ({B}), got {g.shape[0]}")
        r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_gate_batch_mixed_host(self.h, B, g.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _p(r_a),
                                                  _p(r_b), _p(ca_a), _p(i32(ca_b)), _p(i32(cb_a)), _p(i32(cb_b)),
                                                  _p(None if cc_a is None else i32(cc_a)),
                                                  _p(None if cc_b is None else i32(cc_b))), "gate_batch_mixed_host")
        return r_a, r_b

    def woks_host(self, mu, x_a, x_b):
        x_a = i32(x_a); B = x_a.shape[0]
        u_a = np.zeros((B, N), np.int32); u_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_bootstrap_woks_batch_host(self.h, B, int(mu), _p(x_a), _p(i32(x_b)), _p(u_a), _p(u_b)),
               "woks_host")
        return u_a, u_b

    def bootstrap_host(self, mu, x_a, x_b):
        x_a = i32(x_a); B = x_a.shape[0]
        r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_bootstrap_batch_host(self.h, B, int(mu), _p(x_a), _p(i32(x_b)), _p(r_a), _p(r_b)),
               "bootstrap_host")
        return r_a, r_b

    def keyswitch_host(self, u_a, u_b):
        u_a = i32(u_a); B = u_a.shape[0]
        r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_keyswitch_batch_host(self.h, B, _p(u_a), _p(i32(u_b)), _p(r_a), _p(r_b)),
               "keyswitch_host")
        return r_a, r_b

    # ---- device (torch) batches: tensors must be int32 CUDA/HIP tensors, contiguous
    def _dev_check(self, t, shape, name):
        """The kernels index by shape and run on this context's GPU: refuse anything that would
        make them read or write out of bounds, or touch another device's memory, before it
        reaches the GPU."""
        if t is None:
            raise TfheAmdError(f"{name}: missing tensor")
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise TfheAmdError(f"{name}: need a contiguous int32 GPU tensor of shape {shape}, got "
                               f"{tuple(t.shape)} {t.dtype} cuda={t.is_cuda} contiguous={t.is_contiguous()}")
        if t.device.index is not None and t.device.index != self.device:
            raise TfheAmdError(f"{name}: tensor is on cuda:{t.device.index}, the context on cuda:{self.device}")

    def gate_dev(self, gate, res_a, res_b, ca_a, ca_b, cb_a, cb_b, cc_a=None, cc_b=None, stream=None):
        g = GATES[gate] if isinstance(gate, str) else int(gate)
        B = ca_a.shape[0]
        named = [("res_a", res_a, (B, n_lwe)), ("res_b", res_b, (B,)), ("ca_a", ca_a, (B, n_lwe)),
                 ("ca_b", ca_b, (B,)), ("cb_a", cb_a, (B, n_lwe)), ("cb_b", cb_b, (B,))]
        if g == GATES["MUX"]:
            named += [("cc_a", cc_a, (B, n_lwe)), ("cc_b", cc_b, (B,))]
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        ptr = (lambda t: None if t is None else t.data_ptr())
        _check(lib.tfhe_amd_gate_batch_dev(self.h, g, B, ptr(res_a), ptr(res_b), ptr(ca_a), ptr(ca_b),
                                           ptr(cb_a), ptr(cb_b), ptr(cc_a), ptr(cc_b), stream),
               "gate_batch_dev")

    def woks_dev(self, mu, x_a, x_b, u_a, u_b, stream=None):
        """tfhe_amd_bootstrap_woks_batch_dev on torch tensors: x (n = 500) -> the extracted samples
        u_a [B][1024], u_b [B]"""
        B = x_a.shape[0]
        for name, t, shape in (("x_a", x_a, (B, n_lwe)), ("x_b", x_b, (B,)), ("u_a", u_a, (B, N)), ("u_b", u_b, (B,))):
            self._dev_check(t, shape, name)
        _check(lib.tfhe_amd_bootstrap_woks_batch_dev(self.h, B, int(mu), x_a.data_ptr(), x_b.data_ptr(), u_a.data_ptr(),
                                                     u_b.data_ptr(), stream), "bootstrap_woks_batch_dev")

    def bootstrap_dev(self, mu, x_a, x_b, res_a, res_b, stream=None):
        """tfhe_amd_bootstrap_batch_dev on torch tensors: woKS + key switch, res_a [B][500], res_b [B]"""
        B = x_a.shape[0]
        for name, t, shape in (("x_a", x_a, (B, n_lwe)), ("x_b", x_b, (B,)), ("res_a", res_a, (B, n_lwe)),
                               ("res_b", res_b, (B,))):
            self._dev_check(t, shape, name)
        _check(lib.tfhe_amd_bootstrap_batch_dev(self.h, B, int(mu), x_a.data_ptr(), x_b.data_ptr(), res_a.data_ptr(),
                                                res_b.data_ptr(), stream), "bootstrap_batch_dev")

    def keyswitch_dev(self, u_a, u_b, res_a, res_b, stream=None):
        """tfhe_amd_keyswitch_batch_dev on torch tensors: u_a [B][1024], u_b [B] -> res_a [B][500], res_b [B]"""
        B = u_a.shape[0]
        for name, t, shape in (("u_a", u_a, (B, N)), ("u_b", u_b, (B,)), ("res_a", res_a, (B, n_lwe)),
                               ("res_b", res_b, (B,))):
            self._dev_check(t, shape, name)
        _check(lib.tfhe_amd_keyswitch_batch_dev(self.h, B, u_a.data_ptr(), u_b.data_ptr(), res_a.data_ptr(),
                                                res_b.data_ptr(), stream), "keyswitch_batch_dev")

    # ---- programmable bootstrapping (tfhe_amd_bootstrap_lut_*): tv = test vectors [n_lut][1024] (or
    # one [1024]), lut_index [B] picks each ciphertext's table (None: table 0); the blind-rotation
    # input is (0, c) + sa X + sb Y
    # log_nu / n_out given: the many-LUT entry points, outputs function-major ([n_out][B][...])
    def _lut_host(self, ks, tv, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, log_nu=None, n_out=None):
        tv = i32(tv).reshape(-1, N)
        x_a = i32(x_a); B = x_a.shape[0]
        idx = None if lut_index is None else i32(lut_index)
        if idx is not None and idx.shape != (B,):
            raise TfheAmdError(f"lut_index: need one table index per ciphertext ({B}), got {idx.shape}")
        if int(sb) != 0 and (y_a is None or y_b is None):
            raise TfheAmdError("sb != 0 needs y_a, y_b")
        many = n_out is not None
        lead = (max(int(n_out), 1),) if many else ()
        r_a = np.zeros(lead + (B, n_lwe if ks else N), np.int32); r_b = np.zeros(lead + (B,), np.int32)
        name = "bootstrap_lut" + ("_many" if many else "") + ("" if ks else "_woks") + "_batch_host"
        _check(getattr(lib, "tfhe_amd_" + name)(
            self.h, B, tv.shape[0], _p(tv), _p(idx), *((int(log_nu), int(n_out)) if many else ()), int(c), int(sa),
            _p(x_a), _p(i32(x_b)), int(sb), _p(None if y_a is None else i32(y_a)),
            _p(None if y_b is None else i32(y_b)), _p(r_a), _p(r_b)), name)
        return r_a, r_b

    def lut_woks_host(self, tv, x_a, x_b, lut_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None):
        """tfhe_amd_bootstrap_lut_woks_batch_host -> the extracted samples (u_a [B][1024], u_b [B])"""
        return self._lut_host(False, tv, x_a, x_b, lut_index, c, sa, sb, y_a, y_b)

    def lut_bootstrap_host(self, tv, x_a, x_b, lut_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None):
        """tfhe_amd_bootstrap_lut_batch_host -> the key-switched results (r_a [B][500], r_b [B])"""
        return self._lut_host(True, tv, x_a, x_b, lut_index, c, sa, sb, y_a, y_b)

    def _lut_dev(self, ks, tv, out_a, out_b, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, stream, log_nu=None,
                 n_out=None):
        B = x_a.shape[0]
        if tv is None or tv.dim() != 2 or tv.shape[0] < 1:
            raise TfheAmdError("tv: need a GPU tensor [n_lut][1024]")
        n_lut = tv.shape[0]
        many = n_out is not None
        lead = (max(int(n_out), 1),) if many else ()
        named = [("tv", tv, (n_lut, N)), ("out_a", out_a, lead + (B, n_lwe if ks else N)), ("out_b", out_b, lead + (B,)),
                 ("x_a", x_a, (B, n_lwe)), ("x_b", x_b, (B,))]
        if lut_index is not None:
            named.append(("lut_index", lut_index, (B,)))
        if int(sb) != 0:
            named += [("y_a", y_a, (B, n_lwe)), ("y_b", y_b, (B,))]
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        ptr = (lambda t: None if t is None else t.data_ptr())
        name = "bootstrap_lut" + ("_many" if many else "") + ("" if ks else "_woks") + "_batch_dev"
        _check(getattr(lib, "tfhe_amd_" + name)(
            self.h, B, n_lut, ptr(tv), ptr(lut_index), *((int(log_nu), int(n_out)) if many else ()), int(c), int(sa),
            ptr(x_a), ptr(x_b), int(sb), ptr(y_a) if int(sb) else None, ptr(y_b) if int(sb) else None, ptr(out_a),
            ptr(out_b), stream), name)

    def lut_woks_dev(self, tv, u_a, u_b, x_a, x_b, lut_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None, stream=None):
        """tfhe_amd_bootstrap_lut_woks_batch_dev on torch tensors (as gate_dev); a lut_index entry
        outside [0, n_lut) is clamped by the kernel"""
        self._lut_dev(False, tv, u_a, u_b, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, stream)

    def lut_bootstrap_dev(self, tv, res_a, res_b, x_a, x_b, lut_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None,
                          stream=None):
        """tfhe_amd_bootstrap_lut_batch_dev on torch tensors; res may alias x"""
        self._lut_dev(True, tv, res_a, res_b, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, stream)

    # ---- many-LUT bootstrapping (tfhe_amd_bootstrap_lut_many_*): as the lut_* methods, with the
    # modulus switch to a multiple of 2^log_nu and n_out <= 2^log_nu outputs per ciphertext,
    # function-major ([n_out][B][...])
    def lut_many_woks_host(self, tv, log_nu, n_out, x_a, x_b, lut_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None):
        """tfhe_amd_bootstrap_lut_many_woks_batch_host -> (u_a [n_out][B][1024], u_b [n_out][B])"""
        return self._lut_host(False, tv, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, log_nu, n_out)

    def lut_many_bootstrap_host(self, tv, log_nu, n_out, x_a, x_b, lut_index=None, c=0, sa=1, sb=0, y_a=None,
                                y_b=None):
        """tfhe_amd_bootstrap_lut_many_batch_host -> (r_a [n_out][B][500], r_b [n_out][B])"""
        return self._lut_host(True, tv, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, log_nu, n_out)

    def lut_many_woks_dev(self, tv, log_nu, n_out, u_a, u_b, x_a, x_b, lut_index=None, c=0, sa=1, sb=0, y_a=None,
                          y_b=None, stream=None):
        """tfhe_amd_bootstrap_lut_many_woks_batch_dev on torch tensors: u_a [n_out][B][1024], u_b [n_out][B]"""
        self._lut_dev(False, tv, u_a, u_b, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, stream, log_nu, n_out)

    def lut_many_bootstrap_dev(self, tv, log_nu, n_out, res_a, res_b, x_a, x_b, lut_index=None, c=0, sa=1, sb=0,
                               y_a=None, y_b=None, stream=None):
        """tfhe_amd_bootstrap_lut_many_batch_dev on torch tensors: res_a [n_out][B][500], res_b [n_out][B];
        res may overlap x"""
        self._lut_dev(True, tv, res_a, res_b, x_a, x_b, lut_index, c, sa, sb, y_a, y_b, stream, log_nu, n_out)

    # ---- one-rotation full adders (tfhe_amd_full_add_batch_*): a, b, c = (a [B][500], b [B]) of
    # half-torus bits, c = None: half adders; results [2][B][...]: the sum bits, then the carries
    def full_add_host(self, enc_sum, enc_carry, a, b, c=None):
        """tfhe_amd_full_add_batch_host -> (r_a [2][B][500], r_b [2][B])"""
        a_a = i32(a[0]); B = a_a.shape[0]
        r_a = np.zeros((2, B, n_lwe), np.int32); r_b = np.zeros((2, B), np.int32)
        _check(lib.tfhe_amd_full_add_batch_host(self.h, B, _enc(enc_sum), _enc(enc_carry), _p(a_a), _p(i32(a[1])),
                                                _p(i32(b[0])), _p(i32(b[1])), _p(None if c is None else i32(c[0])),
                                                _p(None if c is None else i32(c[1])), _p(r_a), _p(r_b)),
               "full_add_batch_host")
        return r_a, r_b

    def full_add_dev(self, enc_sum, enc_carry, res_a, res_b, a, b, c=None, stream=None):
        """tfhe_amd_full_add_batch_dev on torch tensors: res_a [2][B][500], res_b [2][B]; a, b, c are
        pairs (a [B][500], b [B]); res may overlap an input"""
        B = a[0].shape[0]
        named = [("res_a", res_a, (2, B, n_lwe)), ("res_b", res_b, (2, B))]
        for nm, v in (("a", a), ("b", b)) + ((("c", c),) if c is not None else ()):
            named += [(nm + "_a", v[0], (B, n_lwe)), (nm + "_b", v[1], (B,))]
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        cp = (None, None) if c is None else (c[0].data_ptr(), c[1].data_ptr())
        _check(lib.tfhe_amd_full_add_batch_dev(self.h, B, _enc(enc_sum), _enc(enc_carry), a[0].data_ptr(),
                                               a[1].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), cp[0], cp[1],
                                               res_a.data_ptr(), res_b.data_ptr(), stream), "full_add_batch_dev")

    # ---- leveled mode (tfhe_amd_tgsw_*): CMux chains on caller-supplied TGSW samples
    def tgsw_import(self, coef):
        """tfhe_amd_tgsw_import: coef [n][4][2][1024] (SecretKeyset.tgsw_encrypt) -> TgswSet on
        this context's device"""
        coef = i32(coef)
        if coef.ndim != 4 or coef.shape[1:] != (KPL, 2, N) or coef.shape[0] < 1:
            raise TfheAmdError(f"coef: need int32 [n][4][2][1024], got {coef.shape}")
        h = _VP()
        _check(lib.tfhe_amd_tgsw_import(self.h, coef.shape[0], _p(coef), ctypes.byref(h)), "tgsw_import")
        return TgswSet(h.value, self.device)

    def tgsw_cmux_dev(self, tset, sel, d1, d0, out, stream=None):
        """tfhe_amd_tgsw_cmux_dev on torch tensors: out[w] = d0[w] + C_sel[w] (x) (d1[w] - d0[w]);
        d0 = None: the external product; out may be d0 or d1"""
        B = sel.shape[0]
        named = [("sel", sel, (B,)), ("d1", d1, (B, 2, N)), ("out", out, (B, 2, N))]
        if d0 is not None:
            named.append(("d0", d0, (B, 2, N)))
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        _check(lib.tfhe_amd_tgsw_cmux_dev(self.h, tset.h, B, sel.data_ptr(), d1.data_ptr(),
                                          None if d0 is None else d0.data_ptr(), out.data_ptr(), stream),
               "tgsw_cmux_dev")

    def tgsw_lookup_host(self, tset, sel, tab, tab_index=None, log_stride=0, n_out=1, woks=False):
        """tfhe_amd_tgsw_lookup[_woks]_host: sel [B][d] selector indices (bit 0 first), tab
        [n_tab][n_poly][tab_rows][1024] -> (r_a [n_out][B][500], r_b [n_out][B]), or with woks the
        extracted samples (u_a [n_out][B][1024], u_b [n_out][B])"""
        sel = i32(sel); tab = i32(tab)
        if sel.ndim != 2 or tab.ndim != 4 or tab.shape[3] != N:
            raise TfheAmdError(f"need sel [B][d] and tab [n_tab][n_poly][tab_rows][1024], got {sel.shape}, {tab.shape}")
        B, d = sel.shape
        n_tab, n_poly, rows, _ = tab.shape
        _log2(n_poly)
        idx = None if tab_index is None else i32(tab_index)
        if idx is not None and idx.shape != (B,):
            raise TfheAmdError(f"tab_index: need one table index per query ({B}), got {idx.shape}")
        n_out = int(n_out)
        r_a = np.zeros((max(n_out, 1), B, N if woks else n_lwe), np.int32)
        r_b = np.zeros((max(n_out, 1), B), np.int32)
        name = "tgsw_lookup" + ("_woks" if woks else "") + "_host"
        _check(getattr(lib, "tfhe_amd_" + name)(self.h, tset.h, B, d, _p(sel), n_tab, n_poly, rows, _p(tab), _p(idx),
                                                int(log_stride), n_out, _p(r_a), _p(r_b)), name)
        return r_a, r_b

    def tgsw_lookup_dev(self, tset, sel, tab, out_a, out_b, tab_index=None, log_stride=0, n_out=1, woks=False,
                        stream=None):
        """tfhe_amd_tgsw_lookup[_woks]_dev on torch tensors (shapes as tgsw_lookup_host); asynchronous"""
        if sel is None or sel.dim() != 2 or tab is None or tab.dim() != 4:
            raise TfheAmdError("need GPU tensors sel [B][d] and tab [n_tab][n_poly][tab_rows][1024]")
        B, d = sel.shape
        n_tab, n_poly, rows, _ = tab.shape
        _log2(n_poly)
        n_out = int(n_out)
        named = [("sel", sel, (B, d)), ("tab", tab, (n_tab, n_poly, rows, N)),
                 ("out_a", out_a, (max(n_out, 1), B, N if woks else n_lwe)), ("out_b", out_b, (max(n_out, 1), B))]
        if tab_index is not None:
            named.append(("tab_index", tab_index, (B,)))
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        name = "tgsw_lookup" + ("_woks" if woks else "") + "_dev"
        _check(getattr(lib, "tfhe_amd_" + name)(self.h, tset.h, B, d, sel.data_ptr(), n_tab, n_poly, rows,
                                                tab.data_ptr(), None if tab_index is None else tab_index.data_ptr(),
                                                int(log_stride), n_out, out_a.data_ptr(), out_b.data_ptr(), stream),
               name)

    # ---- leveled automata (tfhe_amd_dfa_*): a DFA over TGSW-encrypted bits, one CMux per step
    def dfa_create(self, next, start, max_len):
        """tfhe_amd_dfa_create: next [n_states][2] (dfa_compare, dfa_contains, dfa_at_least or the
        caller's own) -> Dfa on this context's device, for words of up to max_len bits"""
        return Dfa._create(self.h, next, start, max_len)

    def dfa_run_host(self, tset, dfa, sel, fin, fin_index=None, n_out=1, woks=False, weights=None):
        """tfhe_amd_dfa_run[_woks]_host: sel [B][len] selector indices (bit 0 first), fin
        [n_fin][n_states][fin_rows][1024] final weights -> (r_a [n_out][B][500], r_b [n_out][B]), or
        with woks the extracted samples (u_a [n_out][B][1024], u_b [n_out][B]).
        weights = (w_val [n_states][2], w_pos [len]): the weighted run tfhe_amd_wfa_run[_woks]_host
        (wfa_max, wfa_popcount, wfa_first_one or the caller's own), n_out up to 64"""
        sel = i32(sel); fin = i32(fin)
        if sel.ndim != 2 or fin.ndim != 4 or fin.shape[1] != dfa.n_states or fin.shape[3] != N:
            raise TfheAmdError(f"need sel [B][len] and fin [n_fin][{dfa.n_states}][fin_rows][1024], got {sel.shape}, "
                               f"{fin.shape}")
        B, length = sel.shape
        n_fin, _, rows, _ = fin.shape
        idx = None if fin_index is None else i32(fin_index)
        if idx is not None and idx.shape != (B,):
            raise TfheAmdError(f"fin_index: need one table index per query ({B}), got {idx.shape}")
        n_out = int(n_out)
        r_a = np.zeros((max(n_out, 1), B, N if woks else n_lwe), np.int32)
        r_b = np.zeros((max(n_out, 1), B), np.int32)
        if weights is not None:
            w_val, w_pos = i32(weights[0]), i32(weights[1])
            if w_val.shape != (dfa.n_states, 2) or w_pos.shape != (length,):
                raise TfheAmdError(f"weights: need w_val [{dfa.n_states}][2] and w_pos [{length}], got {w_val.shape}, "
                                   f"{w_pos.shape}")
            name = "wfa_run" + ("_woks" if woks else "") + "_host"
            _check(getattr(lib, "tfhe_amd_" + name)(self.h, tset.h, dfa.h, B, length, _p(sel), _p(w_val), _p(w_pos),
                                                    n_fin, rows, _p(fin), _p(idx), n_out, _p(r_a), _p(r_b)), name)
            return r_a, r_b
        name = "dfa_run" + ("_woks" if woks else "") + "_host"
        _check(getattr(lib, "tfhe_amd_" + name)(self.h, tset.h, dfa.h, B, length, _p(sel), n_fin, rows, _p(fin),
                                                _p(idx), n_out, _p(r_a), _p(r_b)), name)
        return r_a, r_b

    def dfa_run_dev(self, tset, dfa, sel, fin, out_a, out_b, fin_index=None, n_out=1, woks=False, stream=None,
                    weights=None):
        """tfhe_amd_dfa_run[_woks]_dev on torch tensors (shapes as dfa_run_host); asynchronous.
        weights = (w_val, w_pos) GPU tensors: tfhe_amd_wfa_run[_woks]_dev"""
        if sel is None or sel.dim() != 2 or fin is None or fin.dim() != 4:
            raise TfheAmdError("need GPU tensors sel [B][len] and fin [n_fin][n_states][fin_rows][1024]")
        B, length = sel.shape
        n_fin, _, rows, _ = fin.shape
        n_out = int(n_out)
        named = [("sel", sel, (B, length)), ("fin", fin, (n_fin, dfa.n_states, rows, N)),
                 ("out_a", out_a, (max(n_out, 1), B, N if woks else n_lwe)), ("out_b", out_b, (max(n_out, 1), B))]
        if fin_index is not None:
            named.append(("fin_index", fin_index, (B,)))
        if weights is not None:
            named += [("w_val", weights[0], (dfa.n_states, 2)), ("w_pos", weights[1], (length,))]
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        if weights is not None:
            name = "wfa_run" + ("_woks" if woks else "") + "_dev"
            _check(getattr(lib, "tfhe_amd_" + name)(self.h, tset.h, dfa.h, B, length, sel.data_ptr(),
                                                    weights[0].data_ptr(), weights[1].data_ptr(), n_fin, rows,
                                                    fin.data_ptr(), None if fin_index is None else fin_index.data_ptr(),
                                                    n_out, out_a.data_ptr(), out_b.data_ptr(), stream), name)
            return
        name = "dfa_run" + ("_woks" if woks else "") + "_dev"
        _check(getattr(lib, "tfhe_amd_" + name)(self.h, tset.h, dfa.h, B, length, sel.data_ptr(), n_fin, rows,
                                                fin.data_ptr(), None if fin_index is None else fin_index.data_ptr(),
                                                n_out, out_a.data_ptr(), out_b.data_ptr(), stream), name)

    # ---- packing key switch (tfhe_amd_pack_*): computed LWE samples -> TLWE ciphertexts
    def pack_key_import(self, coef):
        """tfhe_amd_pack_key_import: coef [500][6][2][1024] (SecretKeyset.pack_key) -> PackKey on this
        context's device"""
        coef = i32(coef)
        if coef.shape != (n_lwe, PACK_T, 2, N):
            raise TfheAmdError(f"coef: need int32 [500][6][2][1024], got {coef.shape}")
        h = _VP()
        _check(lib.tfhe_amd_pack_key_import(self.h, _p(coef), ctypes.byref(h)), "pack_key_import")
        return PackKey(h.value, self.device)

    def pack_host(self, pkey, in_a, in_b, pos=None):
        """tfhe_amd_pack_host: in_a [T][P][500], in_b [T][P] (or one output's [P][500], [P]), pos [P]
        distinct positions (None: 0 .. P - 1) -> TLWE ciphertexts [T][2][1024]"""
        in_a = i32(in_a); in_b = i32(in_b)
        if in_a.ndim == 2:
            in_a, in_b = in_a[None], in_b[None]
        if in_a.ndim != 3 or in_a.shape[2] != n_lwe or in_b.shape != in_a.shape[:2]:
            raise TfheAmdError(f"need in_a [T][P][500] and in_b [T][P], got {in_a.shape}, {in_b.shape}")
        T_, P = in_b.shape
        pos = None if pos is None else i32(pos)
        if pos is not None and pos.shape != (P,):
            raise TfheAmdError(f"pos: need one position per input ({P}), got {pos.shape}")
        out = np.zeros((T_, 2, N), np.int32)
        _check(lib.tfhe_amd_pack_host(self.h, pkey.h, T_, P, _p(in_a), _p(in_b), _p(pos), _p(out)), "pack_host")
        return out

    def pack_dev(self, pkey, in_a, in_b, out, pos=None, stream=None):
        """tfhe_amd_pack_dev on torch tensors (shapes as pack_host, out [T][2][1024]); asynchronous"""
        if in_b is None or in_b.dim() != 2:
            raise TfheAmdError("need GPU tensors in_a [T][P][500] and in_b [T][P]")
        T_, P = in_b.shape
        named = [("in_a", in_a, (T_, P, n_lwe)), ("in_b", in_b, (T_, P)), ("out", out, (T_, 2, N))]
        if pos is not None:
            named.append(("pos", pos, (P,)))
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        _check(lib.tfhe_amd_pack_dev(self.h, pkey.h, T_, P, in_a.data_ptr(), in_b.data_ptr(),
                                     None if pos is None else pos.data_ptr(), out.data_ptr(), stream), "pack_dev")

    # ---- bootstrap from encrypted accumulators: acc = TLWE samples [n_acc][2][1024]
    # (or one [2][1024]); acc_index [B] picks each ciphertext's accumulator (None: accumulator 0 when
    # n_acc == 1, accumulator i when n_acc == B); the selector is (0, c) + sa X + sb Y
    def box_fill_host(self, tlwe, log_w):
        """tfhe_amd_tlwe_box_fill_host: tlwe [T][2][1024] (or one [2][1024]) -> tlwe (1 + X + ... +
        X^(2^log_w - 1)), same shape"""
        tlwe = i32(tlwe)
        if tlwe.ndim < 2 or tlwe.shape[-2:] != (2, N):
            raise TfheAmdError(f"need TLWE samples [T][2][1024], got {tlwe.shape}")
        out = np.zeros(tlwe.shape, np.int32)
        _check(lib.tfhe_amd_tlwe_box_fill_host(self.h, tlwe.size // (2 * N), int(log_w), _p(tlwe), _p(out)),
               "tlwe_box_fill_host")
        return out

    def box_fill_dev(self, tlwe, out, log_w, stream=None):
        """tfhe_amd_tlwe_box_fill_dev on torch tensors [T][2][1024]; out may be tlwe; asynchronous"""
        if tlwe is None or tlwe.dim() != 3:
            raise TfheAmdError("need a GPU tensor [T][2][1024]")
        T_ = tlwe.shape[0]
        for name, t in (("tlwe", tlwe), ("out", out)):
            self._dev_check(t, (T_, 2, N), name)
        _check(lib.tfhe_amd_tlwe_box_fill_dev(self.h, T_, int(log_w), tlwe.data_ptr(), out.data_ptr(), stream),
               "tlwe_box_fill_dev")

    def _acc_host(self, ks, acc, x_a, x_b, acc_index, c, sa, sb, y_a, y_b):
        acc = i32(acc).reshape(-1, 2, N)
        x_a = i32(x_a); B = x_a.shape[0]
        idx = None if acc_index is None else i32(acc_index)
        if idx is not None and idx.shape != (B,):
            raise TfheAmdError(f"acc_index: need one accumulator index per ciphertext ({B}), got {idx.shape}")
        if int(sb) != 0 and (y_a is None or y_b is None):
            raise TfheAmdError("sb != 0 needs y_a, y_b")
        r_a = np.zeros((B, n_lwe if ks else N), np.int32); r_b = np.zeros(B, np.int32)
        name = "bootstrap_acc" + ("" if ks else "_woks") + "_batch_host"
        _check(getattr(lib, "tfhe_amd_" + name)(
            self.h, B, acc.shape[0], _p(acc), _p(idx), int(c), int(sa), _p(x_a), _p(i32(x_b)), int(sb),
            _p(None if y_a is None else i32(y_a)), _p(None if y_b is None else i32(y_b)), _p(r_a), _p(r_b)), name)
        return r_a, r_b

    def acc_woks_host(self, acc, x_a, x_b, acc_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None):
        """tfhe_amd_bootstrap_acc_woks_batch_host -> the extracted samples (u_a [B][1024], u_b [B])"""
        return self._acc_host(False, acc, x_a, x_b, acc_index, c, sa, sb, y_a, y_b)

    def acc_bootstrap_host(self, acc, x_a, x_b, acc_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None):
        """tfhe_amd_bootstrap_acc_batch_host -> the key-switched results (r_a [B][500], r_b [B])"""
        return self._acc_host(True, acc, x_a, x_b, acc_index, c, sa, sb, y_a, y_b)

    def _acc_dev(self, ks, acc, out_a, out_b, x_a, x_b, acc_index, c, sa, sb, y_a, y_b, stream):
        B = x_a.shape[0]
        if acc is None or acc.dim() != 3 or acc.shape[0] < 1:
            raise TfheAmdError("acc: need a GPU tensor [n_acc][2][1024]")
        n_acc = acc.shape[0]
        named = [("acc", acc, (n_acc, 2, N)), ("out_a", out_a, (B, n_lwe if ks else N)), ("out_b", out_b, (B,)),
                 ("x_a", x_a, (B, n_lwe)), ("x_b", x_b, (B,))]
        if acc_index is not None:
            named.append(("acc_index", acc_index, (B,)))
        if int(sb) != 0:
            named += [("y_a", y_a, (B, n_lwe)), ("y_b", y_b, (B,))]
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        ptr = (lambda t: None if t is None else t.data_ptr())
        name = "bootstrap_acc" + ("" if ks else "_woks") + "_batch_dev"
        _check(getattr(lib, "tfhe_amd_" + name)(
            self.h, B, n_acc, ptr(acc), ptr(acc_index), int(c), int(sa), ptr(x_a), ptr(x_b), int(sb),
            ptr(y_a) if int(sb) else None, ptr(y_b) if int(sb) else None, ptr(out_a), ptr(out_b), stream), name)

    def acc_woks_dev(self, acc, u_a, u_b, x_a, x_b, acc_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None, stream=None):
        """tfhe_amd_bootstrap_acc_woks_batch_dev on torch tensors; an acc_index entry outside [0, n_acc)
        is clamped by the kernel; u must not overlap acc"""
        self._acc_dev(False, acc, u_a, u_b, x_a, x_b, acc_index, c, sa, sb, y_a, y_b, stream)

    def acc_bootstrap_dev(self, acc, res_a, res_b, x_a, x_b, acc_index=None, c=0, sa=1, sb=0, y_a=None, y_b=None,
                          stream=None):
        """tfhe_amd_bootstrap_acc_batch_dev on torch tensors; res may alias x"""
        self._acc_dev(True, acc, res_a, res_b, x_a, x_b, acc_index, c, sa, sb, y_a, y_b, stream)

    def select_host(self, pkey, cand_a, cand_b, y_a, y_b, c=0, sa=1):
        """tfhe_amd_select_batch_host: candidates cand_a [p][B][500], cand_b [p][B] (function-major),
        selectors (0, c) + sa Y -> (r_a [B][500], r_b [B]), query q the candidate in the box of its
        selector's phase"""
        cand_a = i32(cand_a); cand_b = i32(cand_b)
        if cand_a.ndim != 3 or cand_a.shape[2] != n_lwe or cand_b.shape != cand_a.shape[:2]:
            raise TfheAmdError(f"need cand_a [p][B][500] and cand_b [p][B], got {cand_a.shape}, {cand_b.shape}")
        p, B = cand_b.shape
        y_a = i32(y_a); y_b = i32(y_b)
        if y_a.shape != (B, n_lwe) or y_b.shape != (B,):
            raise TfheAmdError(f"need y_a [{B}][500] and y_b [{B}], got {y_a.shape}, {y_b.shape}")
        r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_select_batch_host(self.h, pkey.h, B, p, _p(cand_a), _p(cand_b), int(c), int(sa), _p(y_a),
                                              _p(y_b), _p(r_a), _p(r_b)), "select_batch_host")
        return r_a, r_b

    def select_dev(self, pkey, cand_a, cand_b, y_a, y_b, res_a, res_b, c=0, sa=1, stream=None):
        """tfhe_amd_select_batch_dev on torch tensors (shapes as select_host); asynchronous"""
        if cand_b is None or cand_b.dim() != 2:
            raise TfheAmdError("need GPU tensors cand_a [p][B][500] and cand_b [p][B]")
        p, B = cand_b.shape
        for name, t, shape in (("cand_a", cand_a, (p, B, n_lwe)), ("cand_b", cand_b, (p, B)), ("y_a", y_a, (B, n_lwe)),
                               ("y_b", y_b, (B,)), ("res_a", res_a, (B, n_lwe)), ("res_b", res_b, (B,))):
            self._dev_check(t, shape, name)
        _check(lib.tfhe_amd_select_batch_dev(self.h, pkey.h, B, p, cand_a.data_ptr(), cand_b.data_ptr(), int(c),
                                             int(sa), y_a.data_ptr(), y_b.data_ptr(), res_a.data_ptr(),
                                             res_b.data_ptr(), stream), "select_batch_dev")

    def blind_rotate_dev(self, acc, bara, iters, stream=None):
        B = acc.shape[0]
        self._dev_check(acc, (B, 2, 1024), "acc")
        if int(iters) > 0:
            self._dev_check(bara, (B, int(iters)), "bara")
        _check(lib.tfhe_amd_blind_rotate_dev(self.h, B, int(iters), acc.data_ptr(),
                                             None if bara is None else bara.data_ptr(), stream),
               "blind_rotate_dev")

    def guard_stats(self, reset=False):
        """(largest rounding distance measured, ciphertexts recomputed exactly) since the last
        reset (tfhe_amd_guard_stats; synchronizes the device)."""
        d = ctypes.c_double(); r = ctypes.c_longlong()
        _check(lib.tfhe_amd_guard_stats(self.h, ctypes.byref(d), ctypes.byref(r), int(bool(reset))), "guard_stats")
        return d.value, r.value

    def last_kernels(self):
        """tfhe_amd_last_kernels: the kernels (and variants) the last batch call enqueued."""
        buf = ctypes.create_string_buffer(1024)
        n = lib.tfhe_amd_last_kernels(self.h, buf, 1024)
        if n < 0:
            raise TfheAmdError(f"last_kernels failed (rc={n})")
        return [k for k in buf.value.decode().split(",") if k]

    def profile_enable(self, on=True):
        _check(lib.tfhe_amd_profile_enable(self.h, int(on)), "profile_enable")

    def profile_read(self):
        br = ctypes.c_double(); ks = ctypes.c_double(); nb = ctypes.c_int(); nk = ctypes.c_int()
        _check(lib.tfhe_amd_profile_read(self.h, ctypes.byref(br), ctypes.byref(nb), ctypes.byref(ks),
                                         ctypes.byref(nk)), "profile_read")
        return {"br_ms": br.value, "br_launches": nb.value, "ks_ms": ks.value, "ks_launches": nk.value}


# --------------------------------------------------------------------- several GPUs (§8(e))

def shard_range(total, rank, world):
    """tfhe_amd_shard_range: the library's contiguous shard [lo, hi) (= shard.shard_range)."""
    lo, hi = ctypes.c_longlong(), ctypes.c_longlong()
    _check(lib.tfhe_amd_shard_range(int(total), int(rank), int(world), ctypes.byref(lo), ctypes.byref(hi)),
           "shard_range")
    return lo.value, hi.value


class MultiContext:
    """TfheAmdMulti: one key replica and worker thread per device; a batch of independent gates
    is split into contiguous shards, one per device (tfhe_amd_multi_gate_batch_host)."""

    def __init__(self, bk, ksk, devices):
        self.bk = i32(bk)
        self.ksk = i32(ksk)
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        h = _VP()
        _check(lib.tfhe_amd_multi_create_raw(_p(self.bk), _p(self.ksk), arr, len(self.devices), ctypes.byref(h)),
               "tfhe_amd_multi_create_raw")
        self.h = h.value

    def close(self):
        if getattr(self, "h", None):
            lib.tfhe_amd_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gate_host(self, gate, ca_a, ca_b, cb_a, cb_b, cc_a=None, cc_b=None):
        g = GATES[gate] if isinstance(gate, str) else int(gate)
        ca_a = i32(ca_a); B = ca_a.shape[0]
        r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_multi_gate_batch_host(self.h, g, B, _p(r_a), _p(r_b), _p(ca_a), _p(i32(ca_b)),
                                                  _p(i32(cb_a)), _p(i32(cb_b)),
                                                  _p(None if cc_a is None else i32(cc_a)),
                                                  _p(None if cc_b is None else i32(cc_b))), "multi_gate_batch_host")
        return r_a, r_b

    def gate_dev(self, gate, shards, streams=None):
        """tfhe_amd_multi_gate_batch_dev: shards[i] = (res_a, res_b, ca_a, ca_b, cb_a, cb_b[, cc_a, cc_b])
        int32 tensors on slot i's device (the shard of that slot; may be empty).  Enqueued on
        every slot; call sync()."""
        g = GATES[gate] if isinstance(gate, str) else int(gate)
        k = len(self.devices)
        if len(shards) != k:
            raise TfheAmdError(f"need {k} shards, got {len(shards)}")
        counts = (ctypes.c_int * k)()
        arrs = [(_VP * k)() for _ in range(8)]
        for i, sh in enumerate(shards):
            B = sh[2].shape[0]
            counts[i] = B
            shapes = [(B, n_lwe), (B,)] * (4 if g == GATES["MUX"] else 3)
            for j, t in enumerate(sh[:len(shapes)]):
                if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != shapes[j]:
                    raise TfheAmdError(f"shard {i} tensor {j}: need a contiguous int32 GPU tensor {shapes[j]}")
                if t.device.index is not None and t.device.index != self.devices[i]:
                    raise TfheAmdError(f"shard {i} tensor {j} is on cuda:{t.device.index}, slot device {self.devices[i]}")
                arrs[j][i] = t.data_ptr()
        st = None
        if streams is not None:
            st = (_VP * k)(*[s for s in streams])
        cc = (arrs[6], arrs[7]) if g == GATES["MUX"] else (None, None)
        _check(lib.tfhe_amd_multi_gate_batch_dev(self.h, g, counts, arrs[0], arrs[1], arrs[2], arrs[3], arrs[4],
                                                 arrs[5], cc[0], cc[1], st), "multi_gate_batch_dev")

    def sync(self):
        _check(lib.tfhe_amd_multi_sync(self.h), "multi_sync")

    def circuit_host(self, circ, B, in_wires, in_a, in_b, out_wires):
        """tfhe_amd_multi_circuit_run_host: the B instances sharded over the devices; in_a [n_in][B][500],
        in_b [n_in][B] for the wires in_wires -> (out_a [n_out][B][500], out_b [n_out][B])."""
        in_a = i32(in_a); in_b = i32(in_b)
        n_in, n_out = len(in_wires), len(out_wires)
        if in_a.shape != (n_in, B, n_lwe) or in_b.shape != (n_in, B):
            raise TfheAmdError(f"inputs: need [{n_in}][{B}][500] / [{n_in}][{B}], got {in_a.shape} / {in_b.shape}")
        out_a = np.zeros((n_out, B, n_lwe), np.int32); out_b = np.zeros((n_out, B), np.int32)
        _check(lib.tfhe_amd_multi_circuit_run_host(self.h, circ.h, int(B), n_in, _ids(in_wires), _p(in_a), _p(in_b),
                                                   n_out, _ids(out_wires), _p(out_a), _p(out_b)),
               "multi_circuit_run_host")
        return out_a, out_b

    def circuit_dev(self, circ, shards, streams=None):
        """tfhe_amd_multi_circuit_run_dev: shards[i] = (wires_a [n_wires][B_i][500], wires_b [n_wires][B_i])
        on slot i's device.  Enqueued on every slot; call sync()."""
        k = len(self.devices)
        if len(shards) != k:
            raise TfheAmdError(f"need {k} shards, got {len(shards)}")
        for i, sh in enumerate(shards):
            wa, wb = sh[0], sh[1]
            if wa.dim() != 3 or wa.shape[2] != n_lwe or tuple(wb.shape) != tuple(wa.shape[:2]):
                raise TfheAmdError(f"shard {i}: need wires_a [n_wires][B][500] and wires_b [n_wires][B], "
                                   f"got {tuple(wa.shape)} / {tuple(wb.shape)}")
            for j, t in enumerate((wa, wb)):
                if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
                    raise TfheAmdError(f"shard {i} tensor {j}: need a contiguous int32 GPU tensor")
                if t.device.index is not None and t.device.index != self.devices[i]:
                    raise TfheAmdError(f"shard {i} tensor {j} is on cuda:{t.device.index}, slot device {self.devices[i]}")
        counts = (ctypes.c_int * k)(*[int(sh[0].shape[1]) for sh in shards])
        wa = (_VP * k)(*[sh[0].data_ptr() for sh in shards])
        wb = (_VP * k)(*[sh[1].data_ptr() for sh in shards])
        st = None if streams is None else (_VP * k)(*streams)
        _check(lib.tfhe_amd_multi_circuit_run_dev(self.h, circ.h, counts, wa, wb, st), "multi_circuit_run_dev")

    def key_digest(self, i):
        """FNV-1a 64 of slot i's device key bytes (slots > 0 are peer-copied replicas of slot 0)"""
        d = ctypes.c_ulonglong()
        _check(lib.tfhe_amd_context_key_digest(lib.tfhe_amd_multi_context(self.h, int(i)), ctypes.byref(d)),
               "context_key_digest")
        return d.value

    def guard_stats(self, reset=False):
        """per device slot: (largest rounding distance, ciphertexts recomputed exactly)"""
        out = []
        for i in range(len(self.devices)):
            c = lib.tfhe_amd_multi_context(self.h, i)
            d = ctypes.c_double(); r = ctypes.c_longlong()
            _check(lib.tfhe_amd_guard_stats(c, ctypes.byref(d), ctypes.byref(r), int(bool(reset))), "guard_stats")
            out.append((d.value, r.value))
        return out


def gpu_init(cloud, device_mask):
    """tfhe_gpu_init(cloud key, device_mask): register a multi-device context for the key."""
    _check(lib.tfhe_gpu_init(ctypes.c_void_p(cloud), int(device_mask)), "tfhe_gpu_init")


def gpu_boots_batch(cloud, gate, ca_a, ca_b, cb_a, cb_b, cc_a=None, cc_b=None):
    """tfhe_gpu_boots_batch over the key's registered devices (SURVEY.md §8(b) Tier-2)."""
    g = GATES[gate] if isinstance(gate, str) else int(gate)
    ca_a = i32(ca_a); B = ca_a.shape[0]
    r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
    _check(lib.tfhe_gpu_boots_batch(g, _p(r_a), _p(r_b), _p(ca_a), _p(i32(ca_b)), _p(i32(cb_a)), _p(i32(cb_b)),
                                    _p(None if cc_a is None else i32(cc_a)), _p(None if cc_b is None else i32(cc_b)),
                                    B, ctypes.c_void_p(cloud)), "tfhe_gpu_boots_batch")
    return r_a, r_b


# --------------------------------------------------------------------- circuits (§8(f) row 1)

GATES.update({"MAJ": 11, "XOR3": 12, "NOT": 13, "COPY": 14, "CONST": 15})
_IP = ctypes.POINTER(ctypes.c_int)
lib.tfhe_amd_circuit_create.argtypes = [ctypes.POINTER(_VP)]
lib.tfhe_amd_circuit_destroy.argtypes = [_VP]
lib.tfhe_amd_circuit_state_count.argtypes = [_VP]
lib.tfhe_amd_circuit_inputs.argtypes = [_VP, ctypes.c_int]
lib.tfhe_amd_circuit_gate.argtypes = [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
lib.tfhe_amd_circuit_lincomb.argtypes = [_VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_int32,
                                         ctypes.c_int, ctypes.c_int32, ctypes.c_int]
LUT_GATE = -2   # gate code tfhe_amd_circuit_node reports for a programmable-bootstrap node
LUT_MANY_GATE = -3   # ... for every wire of a many-LUT node
AFFINE_GATE = -4   # ... for an affine node (kind 2): (0, c0) + s[0] * W[in[0]]
lib.tfhe_amd_circuit_affine.argtypes = [_VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int]
lib.tfhe_amd_circuit_to_gate.argtypes = [_VP, ctypes.c_int]
lib.tfhe_amd_circuit_to_half.argtypes = [_VP, ctypes.c_int]
lib.tfhe_amd_circuit_and_half.argtypes = [_VP, ctypes.c_int, ctypes.c_int]
lib.tfhe_amd_circuit_full_add.argtypes = [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          _IP, _IP]
lib.tfhe_amd_circuit_mul_fa.argtypes = [_VP, ctypes.c_int, _IP, _IP, _IP]
lib.tfhe_amd_circuit_dot_fa.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _IP, _IP, ctypes.c_int, _IP]
lib.tfhe_amd_circuit_add_half.argtypes = [_VP, ctypes.c_int, _IP, _IP, ctypes.c_int, ctypes.c_int, _IP]
lib.tfhe_amd_circuit_lut_many.argtypes = [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_int, ctypes.c_int32, ctypes.c_int, ctypes.c_int32, ctypes.c_int]
lib.tfhe_amd_circuit_lut_many_node.argtypes = [_VP, ctypes.c_int, _IP, ctypes.POINTER(ctypes.c_int32), _IP, _IP, _IP]
lib.tfhe_amd_circuit_lut_table.argtypes = [_VP, _I32P]
lib.tfhe_amd_circuit_lut_table_get.argtypes = [_VP, ctypes.c_int, _I32P]
lib.tfhe_amd_circuit_lut.argtypes = [_VP, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_int32,
                                     ctypes.c_int, ctypes.c_int32, ctypes.c_int]
lib.tfhe_amd_circuit_lut_node.argtypes = [_VP, ctypes.c_int, _IP, ctypes.POINTER(ctypes.c_int32)]
lib.tfhe_amd_circuit_info.argtypes = [_VP, _IP, _IP, _IP, _IP]
lib.tfhe_amd_circuit_level_sizes.argtypes = [_VP, _IP, ctypes.c_int]
lib.tfhe_amd_circuit_node.argtypes = [_VP, ctypes.c_int, _IP, _IP, ctypes.POINTER(ctypes.c_int32),
                                      ctypes.POINTER(ctypes.c_int32), _IP]
lib.tfhe_amd_circuit_run_dev.argtypes = [_VP, _VP, ctypes.c_int, _VP, _VP, _VP]
SELECT_GATE = -5   # ... for a select node: the selector is (0, c0) + s[0] * W[in[0]]
lib.tfhe_amd_circuit_select.argtypes = [_VP, ctypes.c_int, _IP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int]
lib.tfhe_amd_circuit_select_node.argtypes = [_VP, ctypes.c_int, _IP, _IP, ctypes.POINTER(ctypes.c_int32)]
lib.tfhe_amd_circuit_select_count.argtypes = [_VP]
lib.tfhe_amd_circuit_lut2.argtypes = [_VP, _I32P, ctypes.c_int, ctypes.c_int]
lib.tfhe_amd_circuit_run_pk_dev.argtypes = [_VP, _VP, _VP, ctypes.c_int, _VP, _VP, _VP]
lib.tfhe_amd_circuit_dot.argtypes = [_VP, ctypes.c_int, ctypes.c_int, _IP, _IP, ctypes.c_int, _IP]
lib.tfhe_amd_circuit_compare.argtypes = [_VP, ctypes.c_int, _IP, _IP, ctypes.c_int, ctypes.c_int]
lib.tfhe_amd_circuit_minmax.argtypes = [_VP, ctypes.c_int, _IP, _IP, ctypes.c_int, ctypes.c_int, _IP]
lib.tfhe_amd_circuit_neg.argtypes = [_VP, ctypes.c_int, _IP, _IP]
lib.tfhe_amd_circuit_abs.argtypes = [_VP, ctypes.c_int, _IP, _IP]
lib.tfhe_amd_circuit_divu.argtypes = [_VP, ctypes.c_int, _IP, _IP, _IP, _IP]
lib.tfhe_amd_circuit_div.argtypes = [_VP, ctypes.c_int, _IP, _IP, _IP]
_VPP = ctypes.POINTER(_VP)
lib.tfhe_amd_multi_gate_batch_dev.argtypes = [_VP, ctypes.c_int, _IP] + [_VPP] * 9
lib.tfhe_amd_multi_sync.argtypes = [_VP]
lib.tfhe_amd_multi_circuit_run_dev.argtypes = [_VP, _VP, _IP, _VPP, _VPP, _VPP]
lib.tfhe_amd_multi_circuit_run_host.argtypes = [_VP, _VP, ctypes.c_int, ctypes.c_int, _IP, _I32P, _I32P, ctypes.c_int,
                                                _IP, _I32P, _I32P]
CMP = {"GT": 0, "GE": 1, "LT": 2, "LE": 3, "EQ": 4, "NE": 5}
for _f in ("add", "sub", "add_prefix", "mul"):
    getattr(lib, "tfhe_amd_circuit_" + _f).argtypes = (
        [_VP, ctypes.c_int, _IP, _IP] + ([ctypes.c_int] if _f == "add" else []) + [_IP])


def _ids(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


class Circuit:
    """TfheAmdCircuit: gates over SSA wires, evaluated level by level on the GPU for B
    independent instances (include/tfhe_amd.h, csrc/circuit.cpp)."""

    def __init__(self):
        h = _VP()
        _check(lib.tfhe_amd_circuit_create(ctypes.byref(h)), "circuit_create")
        self.h = h.value

    def close(self):
        if getattr(self, "h", None):
            lib.tfhe_amd_circuit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def state_count(self):
        """contexts this circuit holds device state for (dropped when a context is destroyed)"""
        return self._w(lib.tfhe_amd_circuit_state_count(self.h), "state_count")

    def _w(self, rc, what):
        if rc < 0:
            raise TfheAmdError(f"{what} failed with code {rc}")
        return rc

    def inputs(self, n):
        first = self._w(lib.tfhe_amd_circuit_inputs(self.h, int(n)), "inputs")
        return list(range(first, first + n))

    def gate(self, name, a, b=-1, c=-1):
        g = GATES[name] if isinstance(name, str) else int(name)
        return self._w(lib.tfhe_amd_circuit_gate(self.h, g, int(a), int(b), int(c)), f"gate {name}")

    def lincomb(self, c0, sa, a, sb=0, b=-1, sc=0, c=-1):
        return self._w(lib.tfhe_amd_circuit_lincomb(self.h, int(c0), int(sa), int(a), int(sb), int(b), int(sc),
                                                    int(c)), "lincomb")

    def lut_table(self, tv):
        """tfhe_amd_circuit_lut_table: register a test vector int32 [1024] (lut_table(p, values));
        returns its table id"""
        tv = i32(tv)
        if tv.shape != (N,):
            raise TfheAmdError(f"tv: need {N} Torus32 words, got shape {tv.shape}")
        return self._w(lib.tfhe_amd_circuit_lut_table(self.h, _p(tv)), "lut_table")

    def lut_table_get(self, table):
        out = np.zeros(N, np.int32)
        _check(lib.tfhe_amd_circuit_lut_table_get(self.h, int(table), _p(out)), "lut_table_get")
        return out

    def lut(self, table, c0, sa, a, sb=0, b=-1, sc=0, c=-1):
        """tfhe_amd_circuit_lut: one programmable bootstrap of (0, c0) + sa*a + sb*b + sc*c through
        `table`; returns the new wire"""
        return self._w(lib.tfhe_amd_circuit_lut(self.h, int(table), int(c0), int(sa), int(a), int(sb), int(b),
                                                int(sc), int(c)), "lut")

    def lut_node(self, w):
        """(table id, c0) of the LUT node w (node(w) reports gate -2 and the table id as c0)"""
        t, c0 = ctypes.c_int(), ctypes.c_int32()
        _check(lib.tfhe_amd_circuit_lut_node(self.h, int(w), ctypes.byref(t), ctypes.byref(c0)), "circuit_lut_node")
        return t.value, c0.value

    def lut_many(self, table, log_nu, n_out, c0, sa, a, sb=0, b=-1, sc=0, c=-1):
        """tfhe_amd_circuit_lut_many: ONE bootstrap of (0, c0) + sa*a + sb*b + sc*c through `table`
        with the modulus switch to a multiple of 2^log_nu; defines n_out consecutive wires (wire
        first + f = the extraction at index f) and returns the first"""
        return self._w(lib.tfhe_amd_circuit_lut_many(self.h, int(table), int(log_nu), int(n_out), int(c0), int(sa),
                                                     int(a), int(sb), int(b), int(sc), int(c)), "lut_many")

    def lut_many_node(self, w):
        """(table id, c0, log_nu, n_out, index) of wire w of a many-LUT node (node(w) reports gate -3
        and the table id as c0)"""
        t, c0 = ctypes.c_int(), ctypes.c_int32()
        th, n, ix = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib.tfhe_amd_circuit_lut_many_node(self.h, int(w), ctypes.byref(t), ctypes.byref(c0), ctypes.byref(th),
                                                  ctypes.byref(n), ctypes.byref(ix)), "circuit_lut_many_node")
        return t.value, c0.value, th.value, n.value, ix.value

    def select(self, cand, sel, c0=0, s=1):
        """tfhe_amd_circuit_select: the box of (0, c0) + s * sel among the p = len(cand) boxes of
        [0, 1/2) picks one of the candidate wires (p in 2, 4, 8, 16); returns the new wire.  A circuit
        with a select node runs with a pack key (run_dev(..., pack_key=))"""
        cand = [int(x) for x in cand]
        return self._w(lib.tfhe_amd_circuit_select(self.h, len(cand), _ids(cand) if cand else None, int(c0), int(s),
                                                   int(sel)), "select")

    def select_node(self, w):
        """(p, candidate wires [p], c0) of the select node w (node(w) reports gate -5, the selector's
        coefficient in s[0] and its wire in in[0])"""
        p, c0 = ctypes.c_int(), ctypes.c_int32()
        cand = (ctypes.c_int * 16)()
        _check(lib.tfhe_amd_circuit_select_node(self.h, int(w), ctypes.byref(p), cand, ctypes.byref(c0)),
               "circuit_select_node")
        return p.value, list(cand[:p.value]), c0.value

    def select_count(self):
        return self._w(lib.tfhe_amd_circuit_select_count(self.h), "select_count")

    def lut2(self, values, x, y):
        """tfhe_amd_circuit_lut2: values [16] Torus32 (lut_encode(m, 4)); the wire of values[4 y + x] for
        two p = 4 digit wires x, y: one many-LUT row on x, one select node driven by y"""
        values = i32(values).reshape(-1)
        if values.shape != (16,):
            raise TfheAmdError(f"values: need 16 Torus32 words, got shape {values.shape}")
        return self._w(lib.tfhe_amd_circuit_lut2(self.h, _p(values), int(x), int(y)), "lut2")

    # ---- one-rotation adder cells (include/tfhe_amd.h): G = gate bits (+-1/8),
    # H = half-torus bits (1/16, 3/16).  The library cannot check which one a wire carries.
    def affine(self, c0, s, a):
        """tfhe_amd_circuit_affine: the bootstrap-free wire (0, c0) + s * a"""
        return self._w(lib.tfhe_amd_circuit_affine(self.h, int(c0), int(s), int(a)), "affine")

    def to_gate(self, a):
        """H -> G, no bootstrap"""
        return self._w(lib.tfhe_amd_circuit_to_gate(self.h, int(a)), "to_gate")

    def to_half(self, a):
        """G -> H, one bootstrap"""
        return self._w(lib.tfhe_amd_circuit_to_half(self.h, int(a)), "to_half")

    def and_half(self, a, b):
        """the AND of two G bits as an H bit, one bootstrap"""
        return self._w(lib.tfhe_amd_circuit_and_half(self.h, int(a), int(b)), "and_half")

    def full_add(self, a, b, cin=-1, enc_sum=ENC_HALF, enc_carry=ENC_HALF, carry=True):
        """tfhe_amd_circuit_full_add on H wires (cin = -1: half adder): ONE bootstrap ->
        (sum wire, carry wire); carry=False: an n_out = 1 row -> (sum wire, None)"""
        s, co = ctypes.c_int(-1), ctypes.c_int(-1)
        self._w(lib.tfhe_amd_circuit_full_add(self.h, int(a), int(b), int(cin), _enc(enc_sum), _enc(enc_carry),
                                              ctypes.byref(s), ctypes.byref(co) if carry else None), "full_add")
        return s.value, (co.value if carry else None)

    def mul_fa(self, a, b):
        """tfhe_amd_circuit_mul_fa: mul with one-rotation adder cells (G in, G out)"""
        return self._vec("mul_fa", a, b, 2 * len(a))[0]

    def dot_fa(self, a_terms, b_terms, out_bits):
        """tfhe_amd_circuit_dot_fa: dot with one-rotation adder cells (G in, G out)"""
        nt, nb = len(a_terms), len(a_terms[0])
        fa = [w for v in a_terms for w in v]
        fb = [w for v in b_terms for w in v]
        out = (ctypes.c_int * out_bits)()
        self._w(lib.tfhe_amd_circuit_dot_fa(self.h, nt, nb, _ids(fa), _ids(fb), int(out_bits), out), "dot_fa")
        return list(out)

    def add_half(self, a, b, carry_in=-1, enc_out=ENC_HALF):
        """tfhe_amd_circuit_add_half: ripple add of H vectors, one row per bit -> (sum wires in
        enc_out, carry-out wire in enc_out)"""
        return self._vec("add_half", a, b, len(a), int(carry_in), _enc(enc_out))

    def _vec(self, fn, a, b, n_out, *extra):
        out = (ctypes.c_int * n_out)()
        rc = getattr(lib, "tfhe_amd_circuit_" + fn)(self.h, len(a), _ids(a), _ids(b), *extra, out)
        self._w(rc, fn)
        return list(out), rc

    def add(self, a, b, carry_in=-1):
        return self._vec("add", a, b, len(a), int(carry_in))

    def sub(self, a, b):
        return self._vec("sub", a, b, len(a))

    def add_prefix(self, a, b):
        return self._vec("add_prefix", a, b, len(a))

    def mul(self, a, b):
        return self._vec("mul", a, b, 2 * len(a))[0]

    def dot(self, a_terms, b_terms, out_bits):
        """sum_t a_t * b_t: a_terms / b_terms are lists of bit-vectors (little-endian wires)"""
        nt, nb = len(a_terms), len(a_terms[0])
        fa = [w for v in a_terms for w in v]
        fb = [w for v in b_terms for w in v]
        out = (ctypes.c_int * out_bits)()
        self._w(lib.tfhe_amd_circuit_dot(self.h, nt, nb, _ids(fa), _ids(fb), int(out_bits), out), "dot")
        return list(out)

    def compare(self, a, b, op, signed=False):
        """one wire: a OP b, OP in GT GE LT LE EQ NE (tfhe_amd_circuit_compare)"""
        return self._w(lib.tfhe_amd_circuit_compare(self.h, len(a), _ids(a), _ids(b), CMP[op], int(signed)),
                       "compare")

    def minmax(self, a, b, want_max=False, signed=False):
        out = (ctypes.c_int * len(a))()
        self._w(lib.tfhe_amd_circuit_minmax(self.h, len(a), _ids(a), _ids(b), int(want_max), int(signed), out),
                "minmax")
        return list(out)

    def neg(self, a):
        out = (ctypes.c_int * len(a))()
        self._w(lib.tfhe_amd_circuit_neg(self.h, len(a), _ids(a), out), "neg")
        return list(out)

    def abs(self, a):
        out = (ctypes.c_int * len(a))()
        self._w(lib.tfhe_amd_circuit_abs(self.h, len(a), _ids(a), out), "abs")
        return list(out)

    def divu(self, a, b):
        q, r = (ctypes.c_int * len(a))(), (ctypes.c_int * len(a))()
        self._w(lib.tfhe_amd_circuit_divu(self.h, len(a), _ids(a), _ids(b), q, r), "divu")
        return list(q), list(r)

    def div(self, a, b):
        q = (ctypes.c_int * len(a))()
        self._w(lib.tfhe_amd_circuit_div(self.h, len(a), _ids(a), _ids(b), q), "div")
        return list(q)

    def info(self):
        v = [ctypes.c_int() for _ in range(4)]
        _check(lib.tfhe_amd_circuit_info(self.h, *[ctypes.byref(x) for x in v]), "circuit_info")
        return dict(zip(("wires", "gates", "bootstraps", "depth"), (x.value for x in v)))

    def level_sizes(self):
        buf = (ctypes.c_int * 4096)()
        n = self._w(lib.tfhe_amd_circuit_level_sizes(self.h, buf, 4096), "level_sizes")
        return list(buf[:n])

    def node(self, w):
        kind, gate = ctypes.c_int(), ctypes.c_int()
        c0 = ctypes.c_int32()
        s = (ctypes.c_int32 * 3)()
        ins = (ctypes.c_int * 3)()
        _check(lib.tfhe_amd_circuit_node(self.h, int(w), ctypes.byref(kind), ctypes.byref(gate), ctypes.byref(c0),
                                         s, ins), "circuit_node")
        return kind.value, gate.value, c0.value, list(s), list(ins)

    def eval_plain(self, bits):
        """Plaintext evaluation of the circuit as built (host; test oracle for the builders):
        wire encodings are +-2^29 and every bootstrapped row is the sign of its torus sum,
        so the threshold gates are checked in the same arithmetic the GPU rows use.
        bits: {input wire: 0/1 array}; returns {wire: 0/1 array} for all wires."""
        e8 = 1 << 29
        n_w = self.info()["wires"]
        val = {}

        def enc(w):
            return val[w]
        spec = {0: (e8, -1, -1), 1: (e8, 1, 1), 2: (-e8, 1, 1), 3: (1 << 30, 2, 2), 4: (-(1 << 30), -2, -2),
                5: (-e8, -1, -1), 6: (-e8, -1, 1), 7: (-e8, 1, -1), 8: (e8, -1, 1), 9: (e8, 1, -1)}

        def sign(x):   # torus phase > 0 (int32)
            x = (np.asarray(x, dtype=np.int64) + 2**31) % 2**32 - 2**31
            return np.where(x > 0, e8, -e8).astype(np.int64)
        for w in range(n_w):
            kind, gate, c0, s, ins = self.node(w)
            if gate == LUT_GATE:
                raise TfheAmdError(f"eval_plain evaluates bits; wire {w} is a LUT node (multi-valued): evaluate it "
                                   "from its table (lut_node, lut_table_get)")
            if gate == LUT_MANY_GATE:
                raise TfheAmdError(f"eval_plain evaluates bits; wire {w} belongs to a many-LUT node (multi-valued): "
                                   "evaluate it from its table (lut_many_node, lut_table_get)")
            if gate == SELECT_GATE:
                raise TfheAmdError(f"eval_plain evaluates bits; wire {w} is a select node (multi-valued): evaluate "
                                   "it from its candidates (select_node)")
            if kind == 0:
                val[w] = np.where(np.asarray(bits[w]) != 0, e8, -e8).astype(np.int64)
            elif kind == 2:
                if gate == GATES["CONST"]:
                    val[w] = np.int64(c0)
                elif gate == AFFINE_GATE:
                    val[w] = np.int64(c0) + np.int64(s[0]) * enc(ins[0])
                else:
                    val[w] = (-1 if gate == GATES["NOT"] else 1) * enc(ins[0])
            elif gate == GATES["MUX"]:
                u1 = sign(-e8 + enc(ins[0]) + enc(ins[1]))
                u2 = sign(-e8 - enc(ins[0]) + enc(ins[2]))
                val[w] = sign(e8 + u1 + u2)
            else:
                if gate in spec:
                    c, sa, sb = spec[gate]
                    x = c + sa * enc(ins[0]) + sb * enc(ins[1])
                else:
                    x = c0 + sum(s[t] * enc(ins[t]) for t in range(3) if ins[t] >= 0)
                val[w] = sign(x)
        return {w: (np.asarray(v) > 0).astype(np.int64) for w, v in val.items()}

    def run(self, ctx, B, inputs, outputs, keyset, rng, stream=None, pack_key=None):
        """Encrypt `inputs` ({wire: bit array [B]}), run on the GPU, decrypt `outputs`
        (list of wires) -> {wire: bit array}.  Convenience for tests and the bench."""
        import torch
        n_w = self.info()["wires"]
        # every wire the run does not write stays this word (0xA5A5A5A5), not a plausible 0
        wa = torch.full((n_w, B, n_lwe), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
        wb = torch.full((n_w, B), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
        for w, bits in inputs.items():
            a, b = keyset.encrypt(np.asarray(bits), rng)
            wa[w] = torch.from_numpy(a).cuda()
            wb[w] = torch.from_numpy(b).cuda()
        self.run_dev(ctx, B, wa, wb, stream, pack_key=pack_key)
        torch.cuda.synchronize()
        ha, hb = wa.cpu().numpy(), wb.cpu().numpy()
        return {w: keyset.decrypt(ha[w], hb[w]) for w in outputs}

    def run_dev(self, ctx, B, wa, wb, stream=None, pack_key=None):
        """pack_key (PackKey): tfhe_amd_circuit_run_pk_dev, the run form a circuit with select nodes needs"""
        if pack_key is not None:
            _check(lib.tfhe_amd_circuit_run_pk_dev(ctx.h, pack_key.h, self.h, int(B), wa.data_ptr(), wb.data_ptr(),
                                                   stream), "circuit_run_pk_dev")
            return
        _check(lib.tfhe_amd_circuit_run_dev(ctx.h, self.h, int(B), wa.data_ptr(), wb.data_ptr(), stream),
               "circuit_run_dev")


def bits_of(x, nbits):
    """little-endian bit planes of an integer array: [nbits][B]"""
    x = np.asarray(x, dtype=np.int64)
    return [((x >> i) & 1) for i in range(nbits)]


def int_of(planes):
    return sum(np.asarray(p, dtype=np.int64) << i for i, p in enumerate(planes))


# --------------------------------------------------------------------- mixed-key batches

lib.tfhe_amd_keyring_create.argtypes = [_VPP, ctypes.c_int, _VPP]
lib.tfhe_amd_keyring_destroy.argtypes = [_VP]
lib.tfhe_amd_keyring_count.argtypes = [_VP]
lib.tfhe_amd_keyring_device.argtypes = [_VP]
lib.tfhe_amd_keyring_plan.argtypes = [ctypes.c_int, ctypes.c_int, _IP, _IP, _IP, _IP, _IP]
lib.tfhe_amd_keyring_gate_batch_dev.argtypes = [_VP, ctypes.c_int, _IP, _IP] + [_VP] * 8 + [_VP]
lib.tfhe_amd_keyring_gate_batch_host.argtypes = [_VP, ctypes.c_int, _IP, _IP] + [_I32P] * 8
lib.tfhe_amd_keyring_bootstrap_lut_batch_dev.argtypes = [_VP, ctypes.c_int, _IP, ctypes.c_int] + [_VP] * 6 + [_VP]
lib.tfhe_amd_keyring_bootstrap_lut_batch_host.argtypes = [_VP, ctypes.c_int, _IP, ctypes.c_int] + [_I32P] * 6


def _ip(a):
    return a.ctypes.data_as(_IP)


class KeyRing:
    """TfheAmdKeyRing: 1 .. 256 contexts of one GPU as key slots; its batch calls take ciphertexts of
    any slot's key (key_of [B], host) in one blind-rotation launch chain.  The ring borrows the
    contexts' keys and runs in contexts[0]'s frame (stream, scratch, guard_stats, last_kernels):
    close it before them (it keeps them referenced until then)."""

    def __init__(self, contexts):
        self.contexts = list(contexts)
        arr = (_VP * max(len(self.contexts), 1))(*[c.h for c in self.contexts])
        h = _VP()
        _check(lib.tfhe_amd_keyring_create(arr, len(self.contexts), ctypes.byref(h)), "tfhe_amd_keyring_create")
        self.h = h.value
        self.device = lib.tfhe_amd_keyring_device(self.h)

    def close(self):
        if getattr(self, "h", None):
            lib.tfhe_amd_keyring_destroy(self.h)
            self.h = None
        self.contexts = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return lib.tfhe_amd_keyring_count(self.h)

    @staticmethod
    def _codes(gates):
        if isinstance(gates, np.ndarray) and gates.dtype.kind in "iu":   # codes already (large batches)
            return np.ascontiguousarray(gates, dtype=np.int32)
        return np.array([GATES[x] if isinstance(x, str) else int(x) for x in gates], dtype=np.int32)

    @staticmethod
    def plan_of(n_keys, key_of, gates=None):
        """tfhe_amd_keyring_plan -> (order [B], offsets [n_keys + 1], rows); needs no GPU"""
        k = np.ascontiguousarray(key_of, dtype=np.int32); B = k.shape[0]
        g = None if gates is None else KeyRing._codes(gates)
        if g is not None and g.shape != (B,):
            raise TfheAmdError(f"gates: need one gate kind per ciphertext ({B}), got {g.shape[0]}")
        order = np.zeros(B, np.int32); offsets = np.zeros(max(int(n_keys), 0) + 1, np.int32); rows = ctypes.c_int()
        _check(lib.tfhe_amd_keyring_plan(B, int(n_keys), _ip(k), None if g is None else _ip(g), _ip(order),
                                         _ip(offsets), ctypes.byref(rows)), "tfhe_amd_keyring_plan")
        return order, offsets, rows.value

    def plan(self, key_of, gates=None):
        return self.plan_of(len(self), key_of, gates)

    def _keys(self, key_of, B):
        k = np.ascontiguousarray(key_of, dtype=np.int32)
        if k.shape != (B,):
            raise TfheAmdError(f"key_of: need one key slot per ciphertext ({B}), got {k.shape}")
        return k

    def gate_host(self, gates, key_of, ca_a, ca_b, cb_a=None, cb_b=None, cc_a=None, cc_b=None):
        """tfhe_amd_keyring_gate_batch_host: gate i of kind gates[i] under key slot key_of[i]"""
        ca_a = i32(ca_a); B = ca_a.shape[0]
        g = self._codes(gates)
        if g.shape != (B,):
            raise TfheAmdError(f"gates: need one gate kind per row ({B}), got {g.shape[0]}")
        k = self._keys(key_of, B)
        r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        opt = lambda x: _p(None if x is None else i32(x))
        _check(lib.tfhe_amd_keyring_gate_batch_host(self.h, B, _ip(g), _ip(k), _p(r_a), _p(r_b), _p(ca_a), _p(i32(ca_b)),
                                                    opt(cb_a), opt(cb_b), opt(cc_a), opt(cc_b)),
               "keyring_gate_batch_host")
        return r_a, r_b

    def _dev_check(self, t, shape, name):
        if t is None:
            raise TfheAmdError(f"{name}: missing tensor")
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise TfheAmdError(f"{name}: need a contiguous int32 GPU tensor of shape {shape}, got "
                               f"{tuple(t.shape)} {t.dtype} cuda={t.is_cuda} contiguous={t.is_contiguous()}")
        if t.device.index is not None and t.device.index != self.device:
            raise TfheAmdError(f"{name}: tensor is on cuda:{t.device.index}, the ring on cuda:{self.device}")

    def gate_dev(self, gates, key_of, res_a, res_b, ca_a, ca_b, cb_a=None, cb_b=None, cc_a=None, cc_b=None,
                 stream=None):
        """tfhe_amd_keyring_gate_batch_dev on torch tensors (as Context.gate_dev); gates and key_of
        are host sequences"""
        B = ca_a.shape[0]
        g = self._codes(gates)
        if g.shape != (B,):
            raise TfheAmdError(f"gates: need one gate kind per row ({B}), got {g.shape[0]}")
        k = self._keys(key_of, B)
        named = [("res_a", res_a, (B, n_lwe)), ("res_b", res_b, (B,)), ("ca_a", ca_a, (B, n_lwe)), ("ca_b", ca_b, (B,))]
        if ((g != GATES["NOT"]) & (g != GATES["COPY"])).any():
            named += [("cb_a", cb_a, (B, n_lwe)), ("cb_b", cb_b, (B,))]
        if (g == GATES["MUX"]).any():
            named += [("cc_a", cc_a, (B, n_lwe)), ("cc_b", cc_b, (B,))]
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        ptr = (lambda t: None if t is None else t.data_ptr())
        _check(lib.tfhe_amd_keyring_gate_batch_dev(self.h, B, _ip(g), _ip(k), ptr(res_a), ptr(res_b), ptr(ca_a),
                                                   ptr(ca_b), ptr(cb_a), ptr(cb_b), ptr(cc_a), ptr(cc_b), stream),
               "keyring_gate_batch_dev")

    def lut_bootstrap_host(self, tv, key_of, x_a, x_b, lut_index=None):
        """tfhe_amd_keyring_bootstrap_lut_batch_host -> (r_a [B][500], r_b [B])"""
        tv = i32(tv).reshape(-1, N)
        x_a = i32(x_a); B = x_a.shape[0]
        idx = None if lut_index is None else i32(lut_index)
        if idx is not None and idx.shape != (B,):
            raise TfheAmdError(f"lut_index: need one table index per ciphertext ({B}), got {idx.shape}")
        k = self._keys(key_of, B)
        r_a = np.zeros((B, n_lwe), np.int32); r_b = np.zeros(B, np.int32)
        _check(lib.tfhe_amd_keyring_bootstrap_lut_batch_host(self.h, B, _ip(k), tv.shape[0], _p(tv), _p(idx), _p(r_a),
                                                             _p(r_b), _p(x_a), _p(i32(x_b))),
               "keyring_bootstrap_lut_batch_host")
        return r_a, r_b

    def lut_bootstrap_dev(self, tv, key_of, res_a, res_b, x_a, x_b, lut_index=None, stream=None):
        """tfhe_amd_keyring_bootstrap_lut_batch_dev on torch tensors; a lut_index entry outside
        [0, n_lut) is clamped by the kernel"""
        B = x_a.shape[0]
        if tv is None or tv.dim() != 2 or tv.shape[0] < 1:
            raise TfheAmdError("tv: need a GPU tensor [n_lut][1024]")
        k = self._keys(key_of, B)
        named = [("tv", tv, (tv.shape[0], N)), ("res_a", res_a, (B, n_lwe)), ("res_b", res_b, (B,)),
                 ("x_a", x_a, (B, n_lwe)), ("x_b", x_b, (B,))]
        if lut_index is not None:
            named.append(("lut_index", lut_index, (B,)))
        for name, t, shape in named:
            self._dev_check(t, shape, name)
        _check(lib.tfhe_amd_keyring_bootstrap_lut_batch_dev(
            self.h, B, _ip(k), tv.shape[0], tv.data_ptr(), None if lut_index is None else lut_index.data_ptr(),
            res_a.data_ptr(), res_b.data_ptr(), x_a.data_ptr(), x_b.data_ptr(), stream),
            "keyring_bootstrap_lut_batch_dev")

    # ---- mixed-key circuits

    @staticmethod
    def circuit_tile():
        """the tile size (lanes) of the engine's one-launch key switch over key groups"""
        return lib.tfhe_amd_keyring_circuit_tile()

    @staticmethod
    def circuit_plan_of(n_keys, key_of, nks, tile=None):
        """tfhe_amd_keyring_circuit_plan -> (order [B], offsets [n_keys + 1], tiles [n_tiles][3] = slot,
        first lane, live lanes) of a level with nks key-switched outputs; needs no GPU"""
        k = np.ascontiguousarray(key_of, dtype=np.int32); B = k.shape[0]
        tile = KeyRing.circuit_tile() if tile is None else int(tile)
        order = np.zeros(B, np.int32); offsets = np.zeros(max(int(n_keys), 0) + 1, np.int32); nt = ctypes.c_int()
        _check(lib.tfhe_amd_keyring_circuit_plan(B, int(n_keys), _ip(k), int(nks), tile, None, None, None, 0,
                                                 ctypes.byref(nt)), "tfhe_amd_keyring_circuit_plan")
        tiles = np.zeros((nt.value, 3), np.int32)
        _check(lib.tfhe_amd_keyring_circuit_plan(B, int(n_keys), _ip(k), int(nks), tile, _ip(order), _ip(offsets),
                                                 _ip(tiles), nt.value, None), "tfhe_amd_keyring_circuit_plan")
        return order, offsets, tiles

    def circuit_plan(self, key_of, nks, tile=None):
        return self.circuit_plan_of(len(self), key_of, nks, tile)

    def circuit_dev(self, circ, key_of, wa, wb, stream=None):
        """tfhe_amd_keyring_circuit_run_dev on torch tensors: wa [n_wires][B][500], wb [n_wires][B] with the
        input wires filled, instance k under key slot key_of[k] (host sequence).  Enqueued."""
        k = np.ascontiguousarray(key_of, dtype=np.int32)
        if k.ndim != 1:
            raise TfheAmdError(f"key_of: need one key slot per instance, got shape {k.shape}")
        B = k.shape[0]
        n_w = circ.info()["wires"]
        if B > 0:
            self._dev_check(wa, (n_w, B, n_lwe), "wa")
            self._dev_check(wb, (n_w, B), "wb")
        ptr = (lambda t: None if t is None or B == 0 else t.data_ptr())
        _check(lib.tfhe_amd_keyring_circuit_run_dev(self.h, circ.h, B, _ip(k), ptr(wa), ptr(wb), stream),
               "keyring_circuit_run_dev")

    def circuit_host(self, circ, key_of, in_wires, in_a, in_b, out_wires):
        """tfhe_amd_keyring_circuit_run_host: in_a [n_in][B][500], in_b [n_in][B] for the wires in_wires ->
        (out_a [n_out][B][500], out_b [n_out][B]); synchronous"""
        k = np.ascontiguousarray(key_of, dtype=np.int32)
        if k.ndim != 1:
            raise TfheAmdError(f"key_of: need one key slot per instance, got shape {k.shape}")
        B = k.shape[0]
        in_a = i32(in_a); in_b = i32(in_b)
        n_in, n_out = len(in_wires), len(out_wires)
        if in_a.shape != (n_in, B, n_lwe) or in_b.shape != (n_in, B):
            raise TfheAmdError(f"inputs: need [{n_in}][{B}][500] / [{n_in}][{B}], got {in_a.shape} / {in_b.shape}")
        out_a = np.zeros((n_out, B, n_lwe), np.int32); out_b = np.zeros((n_out, B), np.int32)
        _check(lib.tfhe_amd_keyring_circuit_run_host(self.h, circ.h, B, _ip(k), n_in, _ids(in_wires), _p(in_a), _p(in_b),
                                                     n_out, _ids(out_wires), _p(out_a), _p(out_b)),
               "keyring_circuit_run_host")
        return out_a, out_b


lib.tfhe_amd_keyring_circuit_plan.argtypes = [ctypes.c_int, ctypes.c_int, _IP, ctypes.c_int, ctypes.c_int, _IP, _IP, _IP,
                                              ctypes.c_int, _IP]
lib.tfhe_amd_keyring_circuit_tile.argtypes = []
lib.tfhe_amd_keyring_circuit_run_dev.argtypes = [_VP, _VP, ctypes.c_int, _IP, _VP, _VP, _VP]
lib.tfhe_amd_keyring_circuit_run_host.argtypes = [_VP, _VP, ctypes.c_int, _IP, ctypes.c_int, _IP, _I32P, _I32P,
                                                  ctypes.c_int, _IP, _I32P, _I32P]
