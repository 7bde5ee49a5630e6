"""Write discipline of every device entry point (and the host gate / key-switch forms): outputs that
start as poison, guard bands around every tensor (tests/dev_arena.py).

Every case asserts, in this order,
  (P1) independence: the call runs once per poison (constant 0xA5A5A5A5, position-dependent) on the
       same inputs, and all output words of the two runs are equal — a kernel that accumulates into, or
       leaves, what the output held before the call differs between the two;
  (P2) correctness: outputs equal the project's oracle word for word — every row of a case with at most
       16 bootstraps or at most 257 key switches, else the first and last row, the rows on both sides of
       every tile and launch seam of the form (c, 2c, 4c and its multiples for the blind rotation,
       multiples of 256 for ks-v5, the many-LUT function blocks) and 16 rows drawn from the case's seed;
  (P3) bands: no word next to a tensor of the call changed — a lane that must not store did not;
  (P4) inputs: tables, test vectors, accumulators, candidates, index arrays and samples are unchanged;
and last that tfhe_amd_last_kernels names the launch form the case is named for.  c is the device's
compute-unit count.  Seeds are explicit integers and every assertion message carries its seed.

The kernels that depend on an earlier launch for their output's initial value — k_keyswitch_small,
k_keyswitch_v5 with a key-index split (both add into rows k_keyswitch_small_init wrote), k_pack_v4
(subtracts from what k_pack_digits* wrote) — and k_circuit_linear's constant zeros are the reason:
on zero-filled outputs "added into garbage", "row not written" and "wrote zeros" look alike."""
import numpy as np
import pytest

import acc_oracle as AO
import dag_oracle as DGO
import dev_arena as DA
import dfa_oracle as DO
import fa_oracle as FO
import lut_oracle as LO
import many_lut_oracle as MO
import pack_oracle as PO
import select_dag_oracle as SO
import tfhe_amd as T
import tgsw_oracle as TO

pytestmark = pytest.mark.gpu

N, n_lwe = 1024, 500
COUNT = 24                       # TGSW samples of the leveled cases' pool
SMALL, SPLIT8, SPLIT4, SPLIT2, UNSPLIT = ("k_keyswitch_small", "k_keyswitch_v5(int8-mfma+split8)",
                                          "k_keyswitch_v5(int8-mfma+split4)", "k_keyswitch_v5(int8-mfma+split2)",
                                          "k_keyswitch_v5(int8-mfma)")


def _cus():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _ks_form(count):
    """launch_keyswitch / ks5_split: the key-switch form of `count` key switches"""
    return SMALL if count <= 12 else SPLIT8 if count <= 256 else SPLIT4 if count <= 768 else SPLIT2 if count <= 1792 \
        else UNSPLIT


def _rows(n, seams, seed, full):
    """the rows of P2 over n rows: all of them when `full`, else the first, the last, both sides of
    every seam (a seam s is the first row of a tile or launch: rows s - 1 and s; seams outside (0, n)
    are dropped) and 16 rows drawn from the seed"""
    if full:
        return np.arange(n)
    rng = np.random.default_rng([int(seed), 77])
    pick = {0, n - 1} | {int(r) for r in rng.choice(n, min(16, n), replace=False)}
    for s in seams:
        if 0 < s < n:
            pick |= {s - 1, s}
    return np.array(sorted(pick))


def _rot_seams(total):
    """blind-rotation indices where a launch form or a launch changes: c, 2c, and every multiple of 4c"""
    c = _cus()
    return [s for s in [c, 2 * c] + list(range(4 * c, total + 1, 4 * c)) if s < total]


def _gate_rows(B, halves, seed):
    """P2 rows of a B-gate batch whose blind rotation runs halves * B rotations (rotation k is gate
    k mod B) and whose key switch runs B rows"""
    seams = [s % B for s in _rot_seams(halves * B)] + list(range(256, B, 256))
    return _rows(B, seams, seed, halves * B <= 16)


def _both(ctx, outs, inps, call, results=None, prepare=None):
    """call(views) once per poison on fresh arenas holding outs [(name, shape)] and inps
    [(name, host array)] -> [(arena, {name: host copy of result}, kernels)] per poison; results: the
    views to read back (default: the outs); prepare(views): device-side filling before the call"""
    import torch
    runs = []
    for poison in DA.POISONS:
        arena, v = DA.Arena.of("cuda", poison, outs, inps)
        if prepare is not None:
            prepare(v)
            torch.cuda.synchronize()
        call(v)
        kern = ctx.last_kernels()
        ctx.sync()
        names = [name for name, _ in outs] if results is None else results
        runs.append((arena, {name: v[name].cpu().numpy() for name in names}, kern))
    return runs


def _verdict(runs, want, what, forms, aliased=(), exact_forms=()):
    """P1, P2 (want: {name: (index, expected)}: result[name][index] == expected), P3 + P4, then the
    launch names: every fragment of `forms` in some kernel name, every name of `exact_forms` listed"""
    (a0, got0, kern0), (a1, got1, kern1) = runs
    for name in got0:
        diff = np.flatnonzero(got0[name].reshape(-1) != got1[name].reshape(-1))
        assert diff.size == 0, (f"{what}: P1 {name} depends on what it held before the call: {diff.size} words differ "
                                f"between the two poisons, the first at word {int(diff[0]) if diff.size else -1}")
    for name, (index, expected) in want.items():
        for poison, got in zip(DA.POISONS, (got0, got1)):
            g = got[name][index]
            assert g.shape == np.asarray(expected).shape, (what, name, g.shape, np.asarray(expected).shape)
            bad = np.argwhere(g != expected)
            assert bad.shape[0] == 0, (f"{what}: P2 {name} != oracle ({poison} poison) at {bad.shape[0]} words, the first "
                                       f"at {bad[0].tolist() if bad.shape[0] else None} of the compared rows")
    for poison, arena in zip(DA.POISONS, (a0, a1)):
        try:
            arena.check(aliased=aliased)
        except AssertionError as e:
            raise AssertionError(f"{what}: P3 / P4 ({poison} poison): {e}") from None
    for kern in (kern0, kern1):
        for frag in forms:
            assert any(frag in k for k in kern), (what, frag, kern)
        for name in exact_forms:
            assert name in kern, (what, name, kern)


# ---------------------------------------------------------------- (a) key switch alone

KS_BATCHES = [1, 4, 5, 12, 13, 256, 257, 768, 769, 1792, 1793]


def _ks_case(B, seed):
    """uniformly random samples with the fixed rows: 0 all digits 0 (u_a = 0), 1 all digits 0 through
    the carry of the 2^15 offset, 2 all digits 3"""
    rng = np.random.default_rng(seed)
    u_a, u_b = _rand32(rng, (B, N)), _rand32(rng, B)
    for row, word in ((0, 0), (1, 0xFFFF8000), (2, 0xFFFE8000)):
        if row < B:                          # B < 4: as many as fit; from 4 on the last row stays random
            u_a[row] = np.uint32(word).astype(np.int32)
    return u_a, u_b


@pytest.mark.parametrize("B", KS_BATCHES)
def test_keyswitch_dev(ctx, okey, B):
    seed = 91000 + B
    what = f"keyswitch_dev B = {B}, seed {seed}"
    u_a, u_b = _ks_case(B, seed)
    runs = _both(ctx, [("res_a", (B, n_lwe)), ("res_b", (B,))], [("u_a", u_a), ("u_b", u_b)],
                 lambda v: ctx.keyswitch_dev(v["u_a"], v["u_b"], v["res_a"], v["res_b"]))
    rows = np.union1d(_rows(B, range(256, B, 256), seed, B <= 257), np.arange(min(B, 3)))   # the fixed rows too
    o_a, o_b = okey.keyswitch_batch(u_a[rows], u_b[rows])
    assert rows[0] == 0 and not o_a[0].any() and o_b[0] == u_b[0], what      # row 0: 500 zeros and b = u_b
    if B > 1:
        assert rows[1] == 1 and not o_a[1].any() and o_b[1] == u_b[1], what  # the carry row as well
    _verdict(runs, {"res_a": (rows, o_a), "res_b": (rows, o_b)}, what, (), exact_forms=(_ks_form(B),))
    assert (B == 1793) == (_ks_form(B) == UNSPLIT)


# ---------------------------------------------------------------- (b) gates

def _gate_case(keyset, gate, B, seed):
    rng = np.random.default_rng(seed)
    nin = 3 if gate == "MUX" else 2
    return [v for _ in range(nin) for v in keyset.encrypt(rng.integers(0, 2, B), rng)]


def _gate_run(ctx, okey, gate, B, seed, host, what, forms, exact_forms):
    names = ["ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b"][:len(host)]
    runs = _both(ctx, [("res_a", (B, n_lwe)), ("res_b", (B,))], list(zip(names, host)),
                 lambda v: ctx.gate_dev(gate, v["res_a"], v["res_b"], *[v[k] for k in names]))
    rows = _gate_rows(B, 2 if gate == "MUX" else 1, seed)
    o_a, o_b = okey.gate_batch(gate, *[h[rows] for h in host])
    _verdict(runs, {"res_a": (rows, o_a), "res_b": (rows, o_b)}, what, forms, exact_forms=exact_forms)


@pytest.mark.parametrize("form", ["lds-1", "lds-13", "paired-odd", "reg", "two-launches"])
def test_gate_dev_nand(ctx, okey, keyset, form):
    """LDS rotation, the paired kernel with an odd count (a padding ciphertext that must not store), the
    register rotation, and two launches with a 3-ciphertext tail"""
    c = _cus()
    B, forms = {"lds-1": (1, ("lds-rotation",)), "lds-13": (13, ("lds-rotation",)),
                "paired-odd": (c + 1, ("paired",)), "reg": (2 * c + 1, ("reg-rotation",)),
                "two-launches": (4 * c + 3, ("reg-rotation", "lds-rotation"))}[form]
    seed = 92000 + B
    what = f"gate_dev NAND B = {B} ({form}), seed {seed}"
    _gate_run(ctx, okey, "NAND", B, seed, _gate_case(keyset, "NAND", B, seed), what, forms + ("guard",),
              (_ks_form(B),))


@pytest.mark.parametrize("form", ["small-ks", "split8", "seam", "unsplit"])
def test_gate_dev_mux(ctx, okey, keyset, form):
    """the key switch of u1 + u2 + (0, 1/8) (ua2) in the small, split-8 and unsplit forms, and 4c + 4
    rotations across a launch seam"""
    c = _cus()
    B, forms = {"small-ks": (3, ("lds-rotation",)), "split8": (13, ("lds-rotation",)),
                "seam": (2 * c + 2, ("reg-rotation", "lds-rotation")), "unsplit": (1793, ("reg-rotation",))}[form]
    seed = 93000 + B
    what = f"gate_dev MUX B = {B} ({form}), seed {seed}"
    _gate_run(ctx, okey, "MUX", B, seed, _gate_case(keyset, "MUX", B, seed), what, forms + ("guard",), (_ks_form(B),))
    if form == "unsplit":
        assert _ks_form(B) == UNSPLIT


@pytest.mark.parametrize("gate,B", [("NAND", 13), ("MUX", 3)])
def test_gate_dev_guard_threshold_zero(ctx, okey, keyset, gate, B):
    """threshold 0: every flag is set and the exact kernel in guard mode writes every row"""
    seed = 94000 + B
    what = f"gate_dev {gate} B = {B} at guard threshold 0, seed {seed}"
    host = _gate_case(keyset, gate, B, seed)
    ctx.guard_stats(reset=True)
    try:
        T.set_guard_threshold(0.0)
        _gate_run(ctx, okey, gate, B, seed, host, what, ("k_blind_rotate_v4", "guard"), (_ks_form(B),))
        _, redo = ctx.guard_stats(reset=True)
    finally:
        T.set_guard_threshold(0.125)
    assert redo == 2 * B * (2 if gate == "MUX" else 1), (what, redo)           # both poisons' runs


# ---------------------------------------------------------------- (c) woKS and bootstrap

def _br_forms(B):
    c = _cus()
    return ("lds-rotation",) if B <= c else ("paired",) if B <= 2 * c else ("reg-rotation",)


@pytest.mark.parametrize("size", ["1", "c+1"])
def test_woks_and_bootstrap_dev(ctx, okey, size):
    B = 1 if size == "1" else _cus() + 1
    seed = 95000 + B
    what = f"woks_dev / bootstrap_dev B = {B}, seed {seed}"
    rng = np.random.default_rng(seed)
    x_a, x_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B)
    x_a[0, :40] = 0                                                            # a run of skipped CMux steps
    rows = _rows(B, _rot_seams(B) + list(range(256, B, 256)), seed, B <= 16)
    w_a, w_b = okey.woks_batch(T.MU, x_a[rows], x_b[rows])
    runs = _both(ctx, [("u_a", (B, N)), ("u_b", (B,))], [("x_a", x_a), ("x_b", x_b)],
                 lambda v: ctx.woks_dev(T.MU, v["x_a"], v["x_b"], v["u_a"], v["u_b"]))
    _verdict(runs, {"u_a": (rows, w_a), "u_b": (rows, w_b)}, what + " (woks)", _br_forms(B) + ("guard",))
    k_a, k_b = okey.keyswitch_batch(w_a, w_b)
    runs = _both(ctx, [("res_a", (B, n_lwe)), ("res_b", (B,))], [("x_a", x_a), ("x_b", x_b)],
                 lambda v: ctx.bootstrap_dev(T.MU, v["x_a"], v["x_b"], v["res_a"], v["res_b"]))
    _verdict(runs, {"res_a": (rows, k_a), "res_b": (rows, k_b)}, what + " (bootstrap)", _br_forms(B) + ("guard",),
             exact_forms=(_ks_form(B),))


# ---------------------------------------------------------------- (d) programmable forms

def _sizes():
    return [("3", 3), ("c+1", _cus() + 1)]


@pytest.mark.parametrize("size", ["3", "c+1"])
def test_lut_dev(ctx, okey, size):
    """lut_woks_dev and lut_bootstrap_dev with two tables and a lut_index"""
    B = dict(_sizes())[size]
    seed = 96000 + B
    what = f"lut_*_dev B = {B}, seed {seed}"
    rng = np.random.default_rng(seed)
    tvs, idx = _rand32(rng, (2, N)), rng.integers(0, 2, B).astype(np.int32)
    idx[:2] = (1, 0)
    x_a, x_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B)
    rows = _rows(B, _rot_seams(B) + list(range(256, B, 256)), seed, B <= 16)
    w = LO.woks_batch(okey, tvs, x_a[rows], x_b[rows], idx[rows])
    inps = [("tv", tvs), ("lut_index", idx), ("x_a", x_a), ("x_b", x_b)]
    runs = _both(ctx, [("u_a", (B, N)), ("u_b", (B,))], inps,
                 lambda v: ctx.lut_woks_dev(v["tv"], v["u_a"], v["u_b"], v["x_a"], v["x_b"], v["lut_index"]))
    _verdict(runs, {"u_a": (rows, w[0]), "u_b": (rows, w[1])}, what + " (woks)", _br_forms(B) + ("lut", "guard"))
    k = okey.keyswitch_batch(*w, nthreads=LO.THREADS)
    runs = _both(ctx, [("res_a", (B, n_lwe)), ("res_b", (B,))], inps,
                 lambda v: ctx.lut_bootstrap_dev(v["tv"], v["res_a"], v["res_b"], v["x_a"], v["x_b"], v["lut_index"]))
    _verdict(runs, {"res_a": (rows, k[0]), "res_b": (rows, k[1])}, what + " (bootstrap)",
             _br_forms(B) + ("lut", "guard"), exact_forms=(_ks_form(B),))


@pytest.mark.parametrize("size", ["3", "c+1"])
def test_lut_many_dev(ctx, okey, size):
    """(log_nu, n_out) = (2, 3): 9 key switches (small) and 3 (c + 1) (split 2 on 256 CUs), function-major"""
    B = dict(_sizes())[size]
    theta, n_out = 2, 3
    seed = 97000 + B
    what = f"lut_many_*_dev B = {B}, seed {seed}"
    rng = np.random.default_rng(seed)
    tvs, idx = _rand32(rng, (2, N)), rng.integers(0, 2, B).astype(np.int32)
    idx[:2] = (1, 0)
    x_a, x_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B)
    ks_seams = [s % B for s in range(256, n_out * B, 256)]                    # key switch f B + i: row i
    rows = _rows(B, _rot_seams(B) + ks_seams, seed, B <= 16)
    w = MO.woks_batch(okey, tvs, x_a[rows], x_b[rows], theta, n_out, idx[rows])
    inps = [("tv", tvs), ("lut_index", idx), ("x_a", x_a), ("x_b", x_b)]
    at = (slice(None), rows)
    runs = _both(ctx, [("u_a", (n_out, B, N)), ("u_b", (n_out, B))], inps,
                 lambda v: ctx.lut_many_woks_dev(v["tv"], theta, n_out, v["u_a"], v["u_b"], v["x_a"], v["x_b"],
                                                 v["lut_index"]))
    _verdict(runs, {"u_a": (at, w[0]), "u_b": (at, w[1])}, what + " (woks)", _br_forms(B) + ("lut-many", "guard"))
    k = MO.keyswitch(okey, w)
    runs = _both(ctx, [("res_a", (n_out, B, n_lwe)), ("res_b", (n_out, B))], inps,
                 lambda v: ctx.lut_many_bootstrap_dev(v["tv"], theta, n_out, v["res_a"], v["res_b"], v["x_a"], v["x_b"],
                                                      v["lut_index"]))
    _verdict(runs, {"res_a": (at, k[0]), "res_b": (at, k[1])}, what + " (bootstrap)",
             _br_forms(B) + ("lut-many", "guard"), exact_forms=(_ks_form(n_out * B),))


@pytest.mark.parametrize("third", ["c", "none"])
@pytest.mark.parametrize("size", ["3", "c+1"])
def test_full_add_dev(ctx, okey, size, third):
    B = dict(_sizes())[size]
    seed = 98000 + B + (1 if third == "c" else 0)
    what = f"full_add_dev B = {B}, c = {third}, seed {seed}"
    rng = np.random.default_rng(seed)
    a, b, c = ((_rand32(rng, (B, n_lwe)), _rand32(rng, B)) for _ in range(3))
    ks_seams = [s % B for s in range(256, 2 * B, 256)]
    rows = _rows(B, _rot_seams(B) + ks_seams, seed, B <= 16)
    sub = lambda x: (x[0][rows], x[1][rows])
    want = FO.cell(okey, FO.H, FO.G, sub(a), sub(b), sub(c) if third == "c" else None)
    inps = [("a_a", a[0]), ("a_b", a[1]), ("b_a", b[0]), ("b_b", b[1])] + ([("c_a", c[0]), ("c_b", c[1])]
                                                                           if third == "c" else [])
    runs = _both(ctx, [("res_a", (2, B, n_lwe)), ("res_b", (2, B))], inps,
                 lambda v: ctx.full_add_dev(FO.H, FO.G, v["res_a"], v["res_b"], (v["a_a"], v["a_b"]), (v["b_a"], v["b_b"]),
                                            (v["c_a"], v["c_b"]) if third == "c" else None))
    at = (slice(None), rows)
    _verdict(runs, {"res_a": (at, want[0]), "res_b": (at, want[1])}, what, _br_forms(B) + ("lut-many", "guard"),
             exact_forms=(_ks_form(2 * B),))


@pytest.mark.parametrize("size", ["3", "c+1"])
def test_acc_dev(ctx, okey, keyset, size):
    """acc_woks_dev and acc_bootstrap_dev with n_acc = 2 and an acc_index"""
    B = dict(_sizes())[size]
    seed = 99000 + B
    what = f"acc_*_dev B = {B}, seed {seed}"
    rng = np.random.default_rng(seed)
    acc, idx = _rand32(rng, (2, 2, N)), rng.integers(0, 2, B).astype(np.int32)
    idx[:2] = (1, 0)
    x_a, x_b = keyset.encrypt_digits(rng.integers(0, 4, B), 4, rng)
    rows = _rows(B, _rot_seams(B) + list(range(256, B, 256)), seed, B <= 16)
    w = AO.woks_batch(okey, acc, x_a[rows], x_b[rows], idx[rows])
    inps = [("acc", acc), ("acc_index", idx), ("x_a", x_a), ("x_b", x_b)]
    runs = _both(ctx, [("u_a", (B, N)), ("u_b", (B,))], inps,
                 lambda v: ctx.acc_woks_dev(v["acc"], v["u_a"], v["u_b"], v["x_a"], v["x_b"], v["acc_index"]))
    _verdict(runs, {"u_a": (rows, w[0]), "u_b": (rows, w[1])}, what + " (woks)", _br_forms(B) + ("tlwe", "guard"))
    k = okey.keyswitch_batch(*w, nthreads=AO.THREADS)
    runs = _both(ctx, [("res_a", (B, n_lwe)), ("res_b", (B,))], inps,
                 lambda v: ctx.acc_bootstrap_dev(v["acc"], v["res_a"], v["res_b"], v["x_a"], v["x_b"], v["acc_index"]))
    _verdict(runs, {"res_a": (rows, k[0]), "res_b": (rows, k[1])}, what + " (bootstrap)",
             _br_forms(B) + ("tlwe", "guard"), exact_forms=(_ks_form(B),))


_cache = {}


def _pack_key(ctx):
    """a packing key of uniformly random words, as tests/test_acc_gpu.py takes it: (words, imported key)"""
    if "pack" not in _cache:
        words = _rand32(np.random.default_rng(3803), (n_lwe, 6, 2, N))
        _cache["pack"] = (words, ctx.pack_key_import(words))
    return _cache["pack"]


@pytest.mark.parametrize("size", ["3", "c+1"])
def test_select_dev(ctx, okey, keyset, size):
    B, p = dict(_sizes())[size], 4
    seed = 100000 + B
    what = f"select_dev p = {p}, B = {B}, seed {seed}"
    words, pkey = _pack_key(ctx)
    rng = np.random.default_rng(seed)
    cand_a, cand_b = _rand32(rng, (p, B, n_lwe)), _rand32(rng, (p, B))
    y_a, y_b = keyset.encrypt_digits(rng.integers(0, p, B), p, rng)
    rows = _rows(B, _rot_seams(B) + list(range(256, B, 256)), seed, B <= 16)
    want = AO.select(okey, words, cand_a[:, rows], cand_b[:, rows], 0, 1, y_a[rows], y_b[rows])
    runs = _both(ctx, [("res_a", (B, n_lwe)), ("res_b", (B,))],
                 [("cand_a", cand_a), ("cand_b", cand_b), ("y_a", y_a), ("y_b", y_b)],
                 lambda v: ctx.select_dev(pkey, v["cand_a"], v["cand_b"], v["y_a"], v["y_b"], v["res_a"], v["res_b"]))
    pack = "k_pack_v4(split)" if B <= _cus() else "k_pack_v4"
    _verdict(runs, {"res_a": (rows, want[0]), "res_b": (rows, want[1])}, what,
             _br_forms(B) + ("tlwe", "guard"), exact_forms=("k_pack_digits(function-major)", pack, "k_tlwe_box_fill",
                                                            _ks_form(B)))


# ---------------------------------------------------------------- (e) leveled and packing forms

def _pool(ctx, keyset):
    """24 TGSW samples of uniformly random words: (imported set, oracle key), once per session"""
    if "pool" not in _cache:
        words = _rand32(np.random.default_rng(2420), (COUNT, 4, 2, N))
        _cache["pool"] = (ctx.tgsw_import(words), TO.key(words, keyset.ksk))
    return _cache["pool"]


@pytest.mark.parametrize("d,log_stride,n_out,size,woks", [(1, 0, 1, "1", False), (3, 1, 2, "5", True),
                                                          (1, 0, 1, "c+1", False)])
def test_tgsw_lookup_dev(ctx, keyset, d, log_stride, n_out, size, woks):
    B = _cus() + 1 if size == "c+1" else int(size)
    seed = 101000 + 10 * B + d
    what = f"tgsw_lookup_dev d = {d}, log_stride = {log_stride}, n_out = {n_out}, B = {B}, woks = {woks}, seed {seed}"
    tset, ok = _pool(ctx, keyset)
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, COUNT, (B, d)).astype(np.int32)
    tab, idx = _rand32(rng, (2, 1, 1, N)), rng.integers(0, 2, B).astype(np.int32)
    rows = _rows(B, _rot_seams(B) + list(range(256, B, 256)), seed, B <= 16)
    want = TO.lookup_woks(ok, sel[rows], tab, idx[rows], log_stride, n_out)
    if not woks:
        want = MO.keyswitch(ok, want)
    width = N if woks else n_lwe
    runs = _both(ctx, [("out_a", (n_out, B, width)), ("out_b", (n_out, B))],
                 [("sel", sel), ("tab", tab), ("tab_index", idx)],
                 lambda v: ctx.tgsw_lookup_dev(tset, v["sel"], v["tab"], v["out_a"], v["out_b"], v["tab_index"], log_stride,
                                               n_out, woks))
    at = (slice(None), rows)
    _verdict(runs, {"out_a": (at, want[0]), "out_b": (at, want[1])}, what, (),
             exact_forms=("k_tgsw_lookup_v4",) + (() if woks else (_ks_form(n_out * B),)))


@pytest.mark.parametrize("with_d0", [True, False])
def test_tgsw_cmux_dev(ctx, keyset, with_d0):
    B = 3
    seed = 102000 + int(with_d0)
    what = f"tgsw_cmux_dev B = {B}, d0 {'given' if with_d0 else 'None'}, out of place, seed {seed}"
    tset, ok = _pool(ctx, keyset)
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, COUNT, B).astype(np.int32)
    d0, d1 = _rand32(rng, (B, 2, N)), _rand32(rng, (B, 2, N))
    want = np.stack([TO.cmux(ok, int(sel[w]), d1[w], d0[w] if with_d0 else None) for w in range(B)])
    runs = _both(ctx, [("out", (B, 2, N))], [("sel", sel), ("d1", d1)] + ([("d0", d0)] if with_d0 else []),
                 lambda v: ctx.tgsw_cmux_dev(tset, v["sel"], v["d1"], v["d0"] if with_d0 else None, v["out"]))
    _verdict(runs, {"out": (slice(None), want)}, what, (), exact_forms=("k_tgsw_cmux_v4",))


def _automaton():
    """Q = 5: the start state branches, a copy state (next0 == next1), a self-loop, and a state nothing
    leads to -> (next [5][2], start)"""
    nxt = np.array([[1, 2], [3, 3], [2, 0], [0, 1], [3, 2]], np.int32)
    assert all(4 not in r for r in DO.reach(nxt, 0, 8))
    return nxt, 0


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("B", [1, 5])
def test_dfa_run_dev(ctx, keyset, B, n_out):
    Q, length = 5, 3
    seed = 103000 + 10 * B + n_out
    what = f"dfa_run_dev Q = {Q}, length = {length}, B = {B}, n_out = {n_out}, seed {seed}"
    tset, ok = _pool(ctx, keyset)
    rng = np.random.default_rng(seed)
    nxt, start = _automaton()
    sel = rng.integers(0, COUNT, (B, length)).astype(np.int32)
    fin, idx = _rand32(rng, (2, Q, 1, N)), rng.integers(0, 2, B).astype(np.int32)
    want = DO.run(ok, nxt, start, sel, fin, idx, n_out)
    dfa = ctx.dfa_create(nxt, start, 8)
    try:
        runs = _both(ctx, [("out_a", (n_out, B, n_lwe)), ("out_b", (n_out, B))],
                     [("sel", sel), ("fin", fin), ("fin_index", idx)],
                     lambda v: ctx.dfa_run_dev(tset, dfa, v["sel"], v["fin"], v["out_a"], v["out_b"], v["fin_index"], n_out))
    finally:
        dfa.close()
    _verdict(runs, {"out_a": (slice(None), want[0]), "out_b": (slice(None), want[1])}, what, ("k_tgsw_dfa_v4",),
             exact_forms=(_ks_form(n_out * B),))


@pytest.mark.parametrize("shape", ["1x1", "3x5", "(c+1)x1"])
def test_pack_dev(ctx, shape):
    """(T, P) = (1, 1), (3, 5) in the split form, (c + 1, 1): one workgroup per output"""
    T_, P = {"1x1": (1, 1), "3x5": (3, 5), "(c+1)x1": (_cus() + 1, 1)}[shape]
    seed = 104000 + 10 * T_ + P
    what = f"pack_dev T = {T_}, P = {P}, seed {seed}"
    words, pkey = _pack_key(ctx)
    rng = np.random.default_rng(seed)
    in_a, in_b = _rand32(rng, (T_, P, n_lwe)), _rand32(rng, (T_, P))
    pos = np.array([0, 1, 511, 512, 1023] if P == 5 else [777], np.int32)
    want = PO.pack_inputs(words, in_a, in_b, pos) if P == 1 else PO.pack_rows(words, in_a, in_b, pos)
    runs = _both(ctx, [("out", (T_, 2, N))], [("in_a", in_a), ("in_b", in_b), ("pos", pos)],
                 lambda v: ctx.pack_dev(pkey, v["in_a"], v["in_b"], v["out"], v["pos"]))
    _verdict(runs, {"out": (slice(None), want)}, what, (),
             exact_forms=("k_pack_digits", "k_pack_v4(split)" if T_ <= _cus() else "k_pack_v4"))


@pytest.mark.parametrize("log_w", [0, 10])
def test_box_fill_dev(ctx, log_w):
    T_ = 3
    seed = 105000 + log_w
    what = f"box_fill_dev T = {T_}, log_w = {log_w}, seed {seed}"
    rng = np.random.default_rng(seed)
    x = _rand32(rng, (T_, 2, N))
    x[-1, 1] = 0
    x[-1, 1, N - 1] = 0x12345678                                              # the wrap sign
    want = AO.box_fill(x, log_w)
    runs = _both(ctx, [("out", (T_, 2, N))], [("tlwe", x)], lambda v: ctx.box_fill_dev(v["tlwe"], v["out"], log_w))
    _verdict(runs, {"out": (slice(None), want)}, what + " (out of place)", (), exact_forms=("k_tlwe_box_fill",))
    runs = _both(ctx, [], [("tlwe", x)], lambda v: ctx.box_fill_dev(v["tlwe"], v["tlwe"], log_w), results=["tlwe"])
    _verdict(runs, {"tlwe": (slice(None), want)}, what + " (in place)", (), aliased=("tlwe",),
             exact_forms=("k_tlwe_box_fill",))


# ---------------------------------------------------------------- (f) circuits

def _circuit_runs(ctx, C, enc, B, pkey=None):
    """wires_a and wires_b from the arena (a band between and after them), the input wire rows filled
    from the host, every other row poison"""
    import torch
    n_w = C.info()["wires"]

    def fill(v):
        for w, (a, b) in enc.items():
            v["wires_a"][w].copy_(torch.from_numpy(np.ascontiguousarray(a)))
            v["wires_b"][w].copy_(torch.from_numpy(np.ascontiguousarray(b)))
    return _both(ctx, [("wires_a", (n_w, B, n_lwe)), ("wires_b", (n_w, B))], [],
                 lambda v: C.run_dev(ctx, B, v["wires_a"], v["wires_b"], pack_key=pkey), prepare=fill), n_w


def _wire_want(W, n_w, rows):
    """every wire (the input wires among them: they must be unchanged) at the compared instances"""
    at = (slice(None), rows)
    return {"wires_a": (at, np.stack([W[w][0] for w in range(n_w)])), "wires_b": (at, np.stack([W[w][1] for w in range(n_w)]))}


def test_circuit_small_level(ctx, okey):
    """circuit 1 at B = 3: one level with three gate rows, one MUX, one CONST wire (k_circuit_linear
    writes its 500 zeros), one NOT, one affine node and one wire nobody reads"""
    B, seed = 3, 106001
    what = f"circuit 1, B = {B}, seed {seed}"
    rng = np.random.default_rng(seed)
    C = T.Circuit()
    try:
        a, b, c = ins = C.inputs(3)
        one = C.gate("CONST", 1)
        nb = C.gate("NOT", b)
        af = C.affine(0x12345678, -3, c)
        g1, g2, g3 = C.gate("NAND", a, nb), C.gate("XOR", a, one), C.gate("OR", b, c)
        m = C.gate("MUX", a, b, c)
        C.gate("COPY", af)                                                     # nobody reads it
        assert C.info()["bootstraps"] == 5 and C.info()["depth"] == 1 and C.info()["wires"] == 11, C.info()
        enc = {w: (_rand32(rng, (B, n_lwe)), _rand32(rng, B)) for w in ins}
        W = DGO.eval_circuit(C, okey, enc, B)
        assert not W[one][0].any() and W[one][1][0] != 0, what                 # the CONST wire: a = 0
        runs, n_w = _circuit_runs(ctx, C, enc, B)
        _verdict(runs, _wire_want(W, n_w, np.arange(B)), what, ("k_blind_rotate_v6_rows", "lds-rotation", "guard"),
                 exact_forms=("k_circuit_linear", SMALL))
        assert len({g1, g2, g3, m}) == 4
    finally:
        C.close()


def test_circuit_unsplit_keyswitch_rows(ctx, okey):
    """circuit 2 at B = 225: 7 two-input gates and one MUX in one level, 1 800 key switches: the
    unsplit ks-v5 kernel in the circuit-rows form with a ragged last tile and r2 >= 0 on the MUX row"""
    B, seed = 225, 106002
    what = f"circuit 2, B = {B}, seed {seed}"
    rng = np.random.default_rng(seed)
    C = T.Circuit()
    try:
        a, b, c, d = ins = C.inputs(4)
        for g, x, y in (("NAND", a, b), ("OR", b, c), ("AND", c, d), ("XOR", a, d)):
            C.gate(g, x, y)
        C.gate("MUX", a, b, c)                                                 # key-switch rows 4 B .. 5 B - 1
        for g, x, y in (("XNOR", b, d), ("NOR", a, c), ("ANDNY", d, a)):
            C.gate(g, x, y)
        assert C.info()["bootstraps"] == 9 and C.info()["depth"] == 1 and 8 * B > 1792, C.info()
        enc = {w: (_rand32(rng, (B, n_lwe)), _rand32(rng, B)) for w in ins}
        seams = [s % B for s in _rot_seams(9 * B) + list(range(256, 8 * B, 256))]   # row r, instance i: index r B + i
        rows = _rows(B, seams, seed, False)
        W = DGO.eval_circuit(C, okey, {w: (x[0][rows], x[1][rows]) for w, x in enc.items()}, len(rows))
        runs, n_w = _circuit_runs(ctx, C, enc, B)
        want = _wire_want(W, n_w, rows)
        every = (list(ins), slice(None))                                       # the input wires: all 225 instances
        want["inputs_a"] = (every, np.stack([enc[w][0] for w in ins]))
        want["inputs_b"] = (every, np.stack([enc[w][1] for w in ins]))
        for _, got, _ in runs:
            got["inputs_a"], got["inputs_b"] = got["wires_a"], got["wires_b"]
        _verdict(runs, want, what, ("k_blind_rotate_v6_rows", "reg-rotation", "guard"), exact_forms=(UNSPLIT,))
    finally:
        C.close()


def test_circuit_select_level(ctx, okey):
    """circuit 3: select_dag_oracle.mixed_circuit at B = 3 through run_dev(..., pack_key=)"""
    B, seed = 3, 106003
    what = f"circuit 3 (mixed_circuit), B = {B}, seed {seed}"
    words, pkey = _pack_key(ctx)
    rng = np.random.default_rng(seed)
    C, ins, sels, others = SO.mixed_circuit()
    try:
        enc = {w: (_rand32(rng, (B, n_lwe)), _rand32(rng, B)) for w in ins}
        W = SO.eval_circuit(C, okey, enc, B, pack_key=words)
        runs, n_w = _circuit_runs(ctx, C, enc, B, pkey)
        _verdict(runs, _wire_want(W, n_w, np.arange(B)), what, ("k_blind_rotate_v6_rows", "tlwe", "guard"),
                 exact_forms=("k_circuit_linear", "k_pack_digits_rows", "k_pack_v4(split)", "k_tlwe_box_fill"))
    finally:
        C.close()


# ---------------------------------------------------------------- (g) host forms

def _host_verdict(runs, want, what, forms=(), exact_forms=()):
    (a0, got0, kern0), (a1, got1, kern1) = runs
    for name in got0:
        assert np.array_equal(got0[name], got1[name]), f"{what}: P1 {name} differs between the two poisons"
    for name, (rows, expected) in want.items():
        for poison, got in zip(DA.POISONS, (got0, got1)):
            assert np.array_equal(got[name][rows], expected), f"{what}: P2 {name} != oracle ({poison} poison)"
    for poison, arena in zip(DA.POISONS, (a0, a1)):
        try:
            arena.check()
        except AssertionError as e:
            raise AssertionError(f"{what}: P3 / P4 ({poison} poison): {e}") from None
    for kern in (kern0, kern1):
        for frag in forms:
            assert any(frag in k for k in kern), (what, frag, kern)
        for name in exact_forms:
            assert name in kern, (what, name, kern)


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
def test_gate_batch_host_nand(ctx, okey, keyset, memory):
    """B = 1025: slices of 1024 + 1; pageable arrays, and every array carved from one
    tfhe_amd_host_alloc buffer (the zero-copy path), whose bands are checked after the call returns"""
    B, seed = 1025, 107000
    what = f"gate_batch_host NAND B = {B} ({memory}), seed {seed}"
    host = _gate_case(keyset, "NAND", B, seed)
    names = ["ca_a", "ca_b", "cb_a", "cb_b"]
    outs = [("res_a", (B, n_lwe)), ("res_b", (B,))]
    runs = []
    for poison in DA.POISONS:
        backing = None
        if memory == "pinned":
            raw = T.host_empty(DA.words_for([s for _, s in outs] + [h.shape for h in host]) + DA.ALIGN)
            skip = (-raw.ctypes.data // 4) % DA.ALIGN
            backing = raw[skip:]
        arena, v = DA.Arena.of("cpu", poison, outs, list(zip(names, host)), backing=backing)
        arr = {k: arena.numpy(t) for k, t in v.items()}
        assert all(T.is_pinned(x) == (memory == "pinned") for x in arr.values()), what
        rc = T.lib.tfhe_amd_gate_batch_host(ctx.h, T.GATES["NAND"], B, T._p(arr["res_a"]), T._p(arr["res_b"]),
                                            *[T._p(arr[k]) for k in names], None, None)
        assert rc == 0, (what, rc)
        runs.append((arena, {k: arr[k].copy() for k, _ in outs}, ctx.last_kernels()))
    rows = _rows(B, _rot_seams(B) + [1024] + list(range(256, B, 256)), seed, False)
    o_a, o_b = okey.gate_batch("NAND", *[h[rows] for h in host])
    # the slice of 1024 (4 x 256 CUs: register rotation, split-2 key switch), then the slice of one
    _host_verdict(runs, {"res_a": (rows, o_a), "res_b": (rows, o_b)}, what, ("reg-rotation", "lds-rotation", "guard"),
                  (_ks_form(1024), _ks_form(1)))


def test_keyswitch_batch_host(ctx, okey):
    B, seed = 13, 107013
    what = f"keyswitch_batch_host B = {B}, seed {seed}"
    u_a, u_b = _ks_case(B, seed)
    runs = []
    for poison in DA.POISONS:
        arena, v = DA.Arena.of("cpu", poison, [("res_a", (B, n_lwe)), ("res_b", (B,))], [("u_a", u_a), ("u_b", u_b)])
        arr = {k: arena.numpy(t) for k, t in v.items()}
        rc = T.lib.tfhe_amd_keyswitch_batch_host(ctx.h, B, T._p(arr["u_a"]), T._p(arr["u_b"]), T._p(arr["res_a"]),
                                                 T._p(arr["res_b"]))
        assert rc == 0, (what, rc)
        runs.append((arena, {"res_a": arr["res_a"].copy(), "res_b": arr["res_b"].copy()}, ctx.last_kernels()))
    o_a, o_b = okey.keyswitch_batch(u_a, u_b)
    _host_verdict(runs, {"res_a": (np.arange(B), o_a), "res_b": (np.arange(B), o_b)}, what, (), (SPLIT8,))
    assert all(kern == [SPLIT8] for _, _, kern in runs), (what, [kern for _, _, kern in runs])


# ---------------------------------------------------------------- (h) history independence

def test_history_independence(ctx, okey, keyset):
    """NAND at B = 5; then a MUX batch of c + 1 with the guard threshold 0 (every flag set, every scratch
    buffer dirty) and a many-LUT bootstrap; the same NAND again at threshold 0.125 gives the same words
    and recomputes nothing"""
    seed = 108000
    what = f"history independence, seed {seed}"
    c = _cus()
    nand = _gate_case(keyset, "NAND", 5, seed)
    names = ["ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b"]

    def run_nand():
        arena, v = DA.Arena.of("cuda", "const", [("res_a", (5, n_lwe)), ("res_b", (5,))], list(zip(names, nand)))
        ctx.gate_dev("NAND", v["res_a"], v["res_b"], *[v[k] for k in names[:4]])
        ctx.sync()
        arena.check()
        return v["res_a"].cpu().numpy(), v["res_b"].cpu().numpy()

    first = run_nand()
    mux = _gate_case(keyset, "MUX", c + 1, seed + 1)
    try:
        T.set_guard_threshold(0.0)
        arena, v = DA.Arena.of("cuda", "index", [("res_a", (c + 1, n_lwe)), ("res_b", (c + 1,))], list(zip(names, mux)))
        ctx.gate_dev("MUX", v["res_a"], v["res_b"], *[v[k] for k in names])
        ctx.sync()
        arena.check()
    finally:
        T.set_guard_threshold(0.125)
    rng = np.random.default_rng(seed + 2)
    tvs, x_a, x_b = _rand32(rng, (1, N)), _rand32(rng, (3, n_lwe)), _rand32(rng, 3)
    arena, v = DA.Arena.of("cuda", "index", [("res_a", (3, 3, n_lwe)), ("res_b", (3, 3))],
                           [("tv", tvs), ("x_a", x_a), ("x_b", x_b)])
    ctx.lut_many_bootstrap_dev(v["tv"], 2, 3, v["res_a"], v["res_b"], v["x_a"], v["x_b"])
    ctx.sync()
    arena.check()
    ctx.guard_stats(reset=True)
    again = run_nand()
    _, redo = ctx.guard_stats()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), what
    want = okey.gate_batch("NAND", *nand)
    assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1]), what
    assert redo == 0, (what, redo)
