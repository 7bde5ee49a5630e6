"""Mixed-key circuits: one ring run of a circuit over instances of several cloud keys
against the same instances run key by key — each slot's instances gathered into [W][n_g] arrays, run
through Circuit.run_dev on that slot's own context, scattered back.

The engine is bit-exact and deterministic, so every comparison is word for word, on every wire.  Keys
as in tests/test_keyring_gpu.py: K0 the session keyset, K1 a second keyset, K2
guard_cases.head_key(K0.bk) with K0's key-switching key — the adversarial key on which the unguarded
fp64 rotation is wrong, so an instance rotated, recomputed or key-switched under another slot's key
shows as wrong words."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dev_arena as DA
import guard_cases as G
import tfhe_amd as T

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, n_lwe = 1024, 500
V6 = "k_blind_rotate_v6_rows("
V6_CONST = V6 + "multi-key+circuit+"
V6_LUT = V6 + "lut+multi-key+circuit+"
V6_MANY = V6 + "lut-many+multi-key+circuit+"
V4 = "k_blind_rotate_v4_rows("
KS_MK = "k_keyswitch_v5(int8-mfma+multi-key"
KS_LABEL = "keyring_circuit_keyswitch(level="
KEYS7 = [2, 0, 1, 0, 2, 1, 0]


def _torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def keyset1():
    K = T.SecretKeyset(seed=(2718, 2818, 2845))
    yield K
    K.close()


@pytest.fixture(scope="module")
def ctx1(keyset1):
    c = T.Context(keyset1.bk, keyset1.ksk, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2(keyset):
    c = T.Context(G.head_key(keyset.bk), keyset.ksk, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ring(ctx, ctx1, ctx2):
    r = T.KeyRing([ctx, ctx1, ctx2])
    yield r
    r.close()


def _dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def _table(C, B, inputs):
    """the host wire table of a run: inputs {wire: (a [B][500], b [B])} filled, every other word poison"""
    n_w = C.info()["wires"]
    wa = np.full((n_w, B, n_lwe), DA.POISON_I32, np.int32)
    wb = np.full((n_w, B), DA.POISON_I32, np.int32)
    for w, (a, b) in inputs.items():
        wa[w], wb[w] = a, b
    return wa, wb


def _per_key(ctxs, C, key_of, wa, wb):
    """the reference: slot by slot, that slot's instances through Circuit.run_dev on its own context"""
    key_of = np.asarray(key_of)
    out_a, out_b = wa.copy(), wb.copy()
    for slot, c in enumerate(ctxs):
        idx = np.flatnonzero(key_of == slot)
        if not idx.size:
            continue
        da, db = _dev(wa[:, idx]), _dev(wb[:, idx])
        C.run_dev(c, idx.size, da, db)
        c.sync()
        out_a[:, idx], out_b[:, idx] = da.cpu().numpy(), db.cpu().numpy()
    return out_a, out_b


def _ring_run(ring, C, key_of, wa, wb, stream=None):
    da, db = _dev(wa), _dev(wb)
    _torch().cuda.synchronize()
    ring.circuit_dev(C, key_of, da, db, stream=stream)
    c0 = ring.contexts[0]
    kern = c0.last_kernels()
    c0.sync()
    return da.cpu().numpy(), db.cpu().numpy(), kern


def _same(got, want, what, kern=()):
    bad = [w for w in range(want[0].shape[0])
           if not (np.array_equal(got[0][w], want[0][w]) and np.array_equal(got[1][w], want[1][w]))]
    assert not bad, (what, "wires that differ from the per-key runs", bad[:10], list(kern))
    assert not (got[0] == DA.POISON_I32).all(axis=2).any(), (what, "a wire row was never written")


def _levels(C):
    """the indices of the circuit's bootstrapped levels"""
    return [L for L, r in enumerate(C.level_sizes()) if r > 0]


def _ks_names(kern):
    """the key-switch kernels of a call (the launch trace keeps a name once)"""
    return [k for k in kern if k.startswith("k_keyswitch")]


def _ks_labels(kern):
    """the ring's label of every key-switch launch of a call: one per level (and per group)"""
    return [k for k in kern if k.startswith(KS_LABEL)]


# ---------------------------------------------------------------- the circuits

def _bit_circuit():
    """4-bit ripple add (XOR3 / MAJ rows), minmax (MUX rows), NOT and CONST"""
    C = T.Circuit()
    a, b = C.inputs(4), C.inputs(4)
    s, co = C.add(a, b)
    mn = C.minmax(a, b)
    nt = C.gate("NOT", s[1])
    k1 = C.gate("CONST", 1)
    return C, a, b, s + [co], mn, [nt, k1]


def _digit_circuit():
    """a lut node, a full_add cell (many-LUT row, two outputs), a lut_many with n_out = 4, and a second
    level of lut rows alone"""
    C = T.Circuit()
    d, ha, hb, hc = C.inputs(4)
    f1 = np.array([2, 0, 3, 1])
    fm = np.array([[1, 3, 0, 2], [3, 3, 1, 0], [0, 2, 2, 1], [2, 1, 0, 3]])
    t1 = C.lut_table(T.lut_table(4, T.lut_encode(f1, 4)))
    tm = C.lut_table(T.lut_table_many(4, T.lut_encode(fm, 4), 2))
    x1 = C.lut(t1, 0, 1, d)
    s, co = C.full_add(ha, hb, hc)
    y = C.lut_many(tm, 2, 4, 0, 1, d)
    z = C.lut(t1, 0, 1, x1)
    return C, (d, ha, hb, hc), (x1, s, co, y, z), f1, fm


def _nand_chain(rows, depth=1):
    """`rows` NAND gates over rows + 1 inputs per level, `depth` levels"""
    C = T.Circuit()
    cur = C.inputs(rows + 1)
    ins = list(cur)
    for _ in range(depth):
        cur = [C.gate("NAND", cur[i], cur[i + 1]) for i in range(len(cur) - 1)] + [cur[0]]
    return C, ins


def _random_inputs(rng, ins, B):
    return {w: (_rand32(rng, (B, n_lwe)), _rand32(rng, B)) for w in ins}


# ---------------------------------------------------------------- 1. parity and decryption

def test_bit_and_digit_circuits_parity_decryption_and_trace(ring, ctx, ctx1, ctx2, keyset, keyset1, rng):
    keysets = [keyset, keyset1, keyset]
    key_of = np.array(KEYS7)
    B = 7
    # the bit circuit
    C, a, b, s, mn, lin = _bit_circuit()
    x, y = rng.integers(0, 16, B), rng.integers(0, 16, B)
    bits = {**dict(zip(a, T.bits_of(x, 4))), **dict(zip(b, T.bits_of(y, 4)))}
    inputs = {}
    for w, v in bits.items():
        ea, eb = np.zeros((B, n_lwe), np.int32), np.zeros(B, np.int32)
        for k in range(B):
            ea[k:k + 1], eb[k:k + 1] = keysets[key_of[k]].encrypt(v[k:k + 1], rng)
        inputs[w] = (ea, eb)
    wa, wb = _table(C, B, inputs)
    got_a, got_b, kern = _ring_run(ring, C, key_of, wa, wb)
    _same((got_a, got_b), _per_key([ctx, ctx1, ctx2], C, key_of, wa, wb), "bit circuit", kern)
    ref = C.eval_plain(bits)
    for K, slot in ((keyset, 0), (keyset1, 1)):
        idx = np.flatnonzero(key_of == slot)
        for w in range(wa.shape[0]):
            dec = K.decrypt(got_a[w][idx], got_b[w][idx])
            assert np.array_equal(dec, np.broadcast_to(ref[w], (B,))[idx]), ("bit circuit", slot, w)
    assert np.array_equal(T.int_of([ref[w] for w in s]), x + y)
    assert any(k.startswith(V6_CONST) for k in kern) and V4 + "multi-key+circuit+guard)" in kern, kern
    assert not any(k.startswith(V6) and "multi-key+circuit" not in k for k in kern), kern
    # exactly one key-switch launch per bootstrapped level, the one over all key groups
    assert _ks_labels(kern) == [f"{KS_LABEL}{L}+tiles=3)" for L in _levels(C)], (kern, C.level_sizes())
    assert _ks_names(kern) and all(k.startswith(KS_MK) for k in _ks_names(kern)), kern
    C.close()

    # the digit circuit
    C, (d, ha, hb, hc), (x1, s1, co, yw, z), f1, fm = _digit_circuit()
    m = rng.integers(0, 4, B)
    hbits = [rng.integers(0, 2, B) for _ in range(3)]
    inputs = {}
    for w, v in zip((d, ha, hb, hc), [m] + hbits):
        ea, eb = np.zeros((B, n_lwe), np.int32), np.zeros(B, np.int32)
        for k in range(B):
            ea[k:k + 1], eb[k:k + 1] = keysets[key_of[k]].encrypt_digits(v[k:k + 1], 4, rng)
        inputs[w] = (ea, eb)
    wa, wb = _table(C, B, inputs)
    got_a, got_b, kern = _ring_run(ring, C, key_of, wa, wb)
    _same((got_a, got_b), _per_key([ctx, ctx1, ctx2], C, key_of, wa, wb), "digit circuit", kern)
    tot = hbits[0] + hbits[1] + hbits[2]
    for K, slot in ((keyset, 0), (keyset1, 1)):
        idx = np.flatnonzero(key_of == slot)
        dec = lambda w: T.lut_decode(K.phase(got_a[w][idx], got_b[w][idx]), 4)
        assert np.array_equal(dec(x1), f1[m[idx]]) and np.array_equal(dec(z), f1[f1[m[idx]]]), slot
        for f in range(4):
            assert np.array_equal(dec(yw + f), fm[f][m[idx]]), (slot, f)
        half = lambda w: T.half_decode(K.phase(got_a[w][idx], got_b[w][idx]))
        assert np.array_equal(half(s1), tot[idx] & 1) and np.array_equal(half(co), tot[idx] >> 1), slot
    assert C.level_sizes() == [0, 3, 1]
    assert any(k.startswith(V6_MANY) for k in kern) and any(k.startswith(V6_LUT) for k in kern), kern
    assert V4 + "lut-many+multi-key+circuit+guard)" in kern and V4 + "lut+multi-key+circuit+guard)" in kern, kern
    assert _ks_labels(kern) == [f"{KS_LABEL}1+tiles=3)", f"{KS_LABEL}2+tiles=3)"], kern
    assert _ks_names(kern) and all(k.startswith(KS_MK) for k in _ks_names(kern)), kern
    C.close()


# ---------------------------------------------------------------- 2. one key, one context twice

def test_one_key_ring_and_the_same_context_twice(ctx, rng):
    B = 6
    C, a, b, s, mn, lin = _bit_circuit()
    wa, wb = _table(C, B, _random_inputs(rng, a + b, B))
    want = _per_key([ctx], C, [0] * B, wa, wb)
    one, two = T.KeyRing([ctx]), T.KeyRing([ctx, ctx])
    try:
        got_a, got_b, kern = _ring_run(one, C, [0] * B, wa, wb)
        _same((got_a, got_b), want, "one-key ring", kern)
        assert _ks_labels(kern) == [f"{KS_LABEL}{L}+slot=0+n={B})" for L in _levels(C)], kern
        assert not any("multi-key" in k for k in _ks_names(kern)), kern
        for key_of in ([0, 1, 0, 1, 1, 0], [1] * B):
            got_a, got_b, kern = _ring_run(two, C, key_of, wa, wb)
            _same((got_a, got_b), want, ("one context in two slots", key_of), kern)
        # all instances in slot 1: one group, the per-group key switch
        assert _ks_labels(kern) == [f"{KS_LABEL}{L}+slot=1+n={B})" for L in _levels(C)], kern
        assert not any("multi-key" in k for k in _ks_names(kern)), kern
        assert C.state_count() >= 3     # ctx's own state and one per ring
    finally:
        one.close()
        two.close()
    assert C.state_count() == 1         # the rings' states went with the rings
    C.close()


# ---------------------------------------------------------------- 3. the guard under the right key

def test_guard_recomputes_under_the_instances_own_key(ring, ctx, ctx1, ctx2):
    rng = np.random.default_rng(4243)
    B = 6
    C, ins = _nand_chain(3, depth=2)
    inputs = {w: G.dirty(rng, B) for w in ins}
    wa, wb = _table(C, B, inputs)
    key_of = np.array([0, 2, 0, 2, 0, 2])
    ctxs = [ctx, ctx1, ctx2]
    for c in ctxs:
        c.guard_stats(reset=True)
    got_a, got_b, kern = _ring_run(ring, C, key_of, wa, wb)
    ring_redo = ctx.guard_stats(reset=True)[1]
    want = _per_key(ctxs, C, key_of, wa, wb)
    redo0, redo2 = ctx.guard_stats(reset=True)[1], ctx2.guard_stats(reset=True)[1]
    assert redo2 >= 1, "inconclusive: the per-key K2 run recomputed no row"
    _same((got_a, got_b), want, "guard", kern)
    assert ring_redo == redo0 + redo2, (ring_redo, redo0, redo2, kern)
    assert V4 + "multi-key+circuit+guard)" in kern, kern
    # the same words under K0 alone: nothing is flagged, and the K2 instances' words were another key's
    got0_a, got0_b, kern = _ring_run(ring, C, [0] * B, wa, wb)
    assert ctx.guard_stats(reset=True)[1] == 0, kern
    out = C.info()["wires"] - 1
    for k in np.flatnonzero(key_of == 2):
        assert (got0_a[out][k] != got_a[out][k]).any(), k
    C.close()


# ---------------------------------------------------------------- 4. geometry

@pytest.mark.parametrize("form", ["reg", "two_rounds"])
def test_launch_geometry(ctx, ctx1, ctx2, form):
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 8
    slots = cus + 4 if form == "reg" else 4 * cus + 6
    B = (slots + rows - 1) // rows
    rng = np.random.default_rng(slots)
    C, ins = _nand_chain(rows)
    wa, wb = _table(C, B, _random_inputs(rng, ins, B))
    key_of = np.arange(B) % 3
    ring3 = T.KeyRing([ctx, ctx1, ctx2])
    try:
        got_a, got_b, kern = _ring_run(ring3, C, key_of, wa, wb)
    finally:
        ring3.close()
    _same((got_a, got_b), _per_key([ctx, ctx1, ctx2], C, key_of, wa, wb), form, kern)
    v6 = [k for k in kern if k.startswith(V6)]
    if form == "reg":          # one round, more than one workgroup per CU
        assert cus < rows * B <= 4 * cus
        assert v6 == [V6_CONST + "reg-rotation)"], kern
    else:                      # a full round of 4 CUs slots, then the 6 .. 13 slots left (8 B - 4 CUs by the choice of B)
        first = 4 * cus
        assert v6 == [V6_CONST + "reg-rotation)", V6_CONST + "lds-rotation)"], kern
        # every key group has slots on both sides of the round boundary (slot r B + k is under key_of[k])
        slot_key = key_of[np.arange(rows * B) % B]
        for g in range(3):
            assert (slot_key[:first] == g).any() and (slot_key[first:] == g).any(), (g, B, cus)
    ks = _ks_names(kern)
    assert len(ks) == 1 and ks[0].startswith(KS_MK) and len(_ks_labels(kern)) == 1, kern
    C.close()


# ---------------------------------------------------------------- 5. key-switch forms

def test_keyswitch_forms(ring, ctx, ctx1, ctx2):
    rng = np.random.default_rng(5511)
    tile = T.KeyRing.circuit_tile()
    ctxs = [ctx, ctx1, ctx2]

    def case(what, r, members, C, ins, key_of, name):
        B = len(key_of)
        wa, wb = _table(C, B, _random_inputs(rng, ins, B))
        got_a, got_b, kern = _ring_run(r, C, key_of, wa, wb)
        _same((got_a, got_b), _per_key(members, C, key_of, wa, wb), what, kern)
        assert _ks_names(kern) == [name], (what, kern)

    # a level of <= 12 lanes in all: two outputs x four instances over two keys, two tiles -> split 4
    C2, ins2 = _nand_chain(2)
    case("8 lanes", ring, ctxs, C2, ins2, [1, 0, 0, 1], KS_MK + "+split4)")
    # an empty middle group
    case("empty middle group", ring, ctxs, C2, ins2, [2, 0, 0, 2, 2], KS_MK + "+split4)")
    # a group of exactly one tile beside a group of one tile + 1 lane: three tiles -> split 4
    C1, ins1 = _nand_chain(1)
    case("one tile | one tile + 1", ring, ctxs, C1, ins1, [1] * (tile + 1) + [0] * tile, KS_MK + "+split4)")
    # eight tiles give the 512 workgroups of the unsplit form: eight groups of one instance each
    ring8 = T.KeyRing([ctx, ctx1] * 4)
    try:
        case("unsplit", ring8, [ctx, ctx1] * 4, C1, ins1, [3, 0, 7, 1, 2, 6, 5, 4], KS_MK + ")")
        case("split 2", ring8, [ctx, ctx1] * 4, C1, ins1, [3, 0, 7, 1], KS_MK + "+split2)")
    finally:
        ring8.close()
    C1.close()
    C2.close()


# ---------------------------------------------------------------- 6. the exact generation

def test_exact_generation(ring, ctx, ctx1, ctx2, rng):
    B = 7
    C, (d, ha, hb, hc), outs, f1, fm = _digit_circuit()
    wa, wb = _table(C, B, _random_inputs(rng, (d, ha, hb, hc), B))
    want = _per_key([ctx, ctx1, ctx2], C, KEYS7, wa, wb)
    T.select_kernel(4)
    try:
        got_a, got_b, kern = _ring_run(ring, C, KEYS7, wa, wb)
    finally:
        T.select_kernel(0)
    _same((got_a, got_b), want, "exact generation", kern)
    br = [k for k in kern if "blind_rotate" in k]   # (a name once: one per level's mode here)
    assert br == [V4 + "lut-many+multi-key+circuit)", V4 + "lut+multi-key+circuit)"], kern
    assert not any("v6" in k or "guard" in k for k in kern), kern
    C.close()


# ---------------------------------------------------------------- 7. TFHE_AMD_KS5=0

def test_ks_v4_layout_subprocess():
    """TFHE_AMD_KS5=0 (read once per process): no member has the int8 key layout, every level takes one
    launch of the single-key kernels per non-empty group; ring against per-key inside the child"""
    code = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
import torch, tfhe_amd as T
K0 = T.SecretKeyset(); K1 = T.SecretKeyset(seed=(2718, 2818, 2845))
c0 = T.Context(K0.bk, K0.ksk, device=0); c1 = T.Context(K1.bk, K1.ksk, device=0)
ring = T.KeyRing([c0, c1])
rng = np.random.default_rng(7)
C = T.Circuit(); a, b = C.inputs(3), C.inputs(3); s, co = C.add(a, b); mn = C.minmax(a, b)
n_w = C.info()["wires"]
for key_of in ([1, 0, 0, 1, 1], [0, 1] * 60):
    key_of = np.array(key_of); B = len(key_of)
    wa = np.full((n_w, B, 500), -0x5A5A5A5B, np.int32); wb = np.full((n_w, B), -0x5A5A5A5B, np.int32)
    for w in a + b:
        wa[w] = rng.integers(-2**31, 2**31, (B, 500), dtype=np.int64).astype(np.int32)
        wb[w] = rng.integers(-2**31, 2**31, B, dtype=np.int64).astype(np.int32)
    da, db = torch.from_numpy(wa).cuda(), torch.from_numpy(wb).cuda()
    torch.cuda.synchronize()
    ring.circuit_dev(C, key_of, da, db); kern = c0.last_kernels(); c0.sync()
    got_a, got_b = da.cpu().numpy(), db.cpu().numpy()
    for slot, c in enumerate((c0, c1)):
        idx = np.flatnonzero(key_of == slot)
        ra, rb = torch.from_numpy(wa[:, idx].copy()).cuda(), torch.from_numpy(wb[:, idx].copy()).cuda()
        torch.cuda.synchronize()
        C.run_dev(c, idx.size, ra, rb); c.sync()
        assert np.array_equal(got_a[:, idx], ra.cpu().numpy()) and np.array_equal(got_b[:, idx], rb.cpu().numpy()), (B, slot)
    ks = [k for k in kern if "keyswitch" in k]
    assert not any("v5" in k or "multi-key" in k for k in ks), ks
    assert sum(k.startswith("keyring_circuit_keyswitch(level=") for k in ks) == 2 * sum(r > 0 for r in C.level_sizes()), ks
    assert any(k == "k_keyswitch_v4" for k in ks) == (B > 5), (B, ks)
ring.close()
print("ring circuit ks-v4 ok")
""" % (os.path.join(REPO, "cpu-gpu-tfhe_amd"), os.path.join(REPO, "tests"))
    env = dict(os.environ, TFHE_AMD_KS5="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ring circuit ks-v4 ok" in r.stdout


# ---------------------------------------------------------------- 8. write discipline

def _arena_table(wa, wb, ins, poison):
    """the wire table inside an arena: the input wires hold their words, every other word the poison"""
    n_w, B = wb.shape
    arena, v = DA.Arena.of("cuda", poison, [("wa", (n_w, B, n_lwe)), ("wb", (n_w, B))])
    for w in ins:
        v["wa"][w].copy_(_dev(wa[w]))
        v["wb"][w].copy_(_dev(wb[w]))
    _torch().cuda.synchronize()
    return arena, v


def test_write_discipline(ring, ctx, ctx1, ctx2):
    torch = _torch()
    rng = np.random.default_rng(8811)
    B = 7
    C, (d, ha, hb, hc), outs, f1, fm = _digit_circuit()
    ins = (d, ha, hb, hc)
    wa, wb = _table(C, B, _random_inputs(rng, ins, B))
    want = _per_key([ctx, ctx1, ctx2], C, KEYS7, wa, wb)
    gots = []
    for poison in DA.POISONS:
        arena, v = _arena_table(wa, wb, ins, poison)
        ring.circuit_dev(C, KEYS7, v["wa"], v["wb"])
        ctx.sync()
        got = v["wa"].cpu().numpy(), v["wb"].cpu().numpy()
        arena.check()
        for w in ins:      # the input wires are unchanged
            assert np.array_equal(got[0][w], wa[w]) and np.array_equal(got[1][w], wb[w]), (poison, w)
        gots.append(got)
    assert np.array_equal(gots[0][0], gots[1][0]) and np.array_equal(gots[0][1], gots[1][1]), \
        "a wire depends on what the wire arrays held before the call"
    _same(gots[0], want, "write discipline")
    # refused calls write nothing: a slot out of range, and a circuit with a select node
    S = T.Circuit()
    x, y, sel = S.inputs(3)
    S.select([x, y], sel)
    arena, v = _arena_table(wa, wb, ins, "index")
    before = v["wa"].clone(), v["wb"].clone()
    for key_of in (KEYS7[:6] + [3], KEYS7[:6] + [-1]):
        with pytest.raises(T.TfheAmdError):
            ring.circuit_dev(C, key_of, v["wa"], v["wb"])
    n_s = S.info()["wires"]
    with pytest.raises(T.TfheAmdError):
        ring.circuit_dev(S, KEYS7, v["wa"][:n_s].contiguous(), v["wb"][:n_s].contiguous())
    assert T.lib.tfhe_amd_keyring_circuit_run_dev(ring.h, S.h, B, T._ip(np.array(KEYS7, np.int32)),
                                                  v["wa"].data_ptr(), v["wb"].data_ptr(), None) == -1
    assert T.lib.tfhe_amd_keyring_circuit_run_dev(ring.h, C.h, B, T._ip(np.array(KEYS7, np.int32)), None, None,
                                                  None) == -1
    assert T.lib.tfhe_amd_keyring_circuit_run_dev(ring.h, C.h, -1, T._ip(np.array(KEYS7, np.int32)),
                                                  v["wa"].data_ptr(), v["wb"].data_ptr(), None) == -1
    assert T.lib.tfhe_amd_keyring_circuit_run_dev(ring.h, C.h, B, None, v["wa"].data_ptr(), v["wb"].data_ptr(),
                                                  None) == -1
    torch.cuda.synchronize()
    assert torch.equal(v["wa"], before[0]) and torch.equal(v["wb"], before[1])
    arena.check()
    S.close()
    C.close()


# ---------------------------------------------------------------- 9. edge cases

def test_edge_cases(ring, ctx, ctx1, ctx2, rng):
    torch = _torch()
    B = 7
    C, a, b, s, mn, lin = _bit_circuit()
    wa, wb = _table(C, B, _random_inputs(rng, a + b, B))
    want = _per_key([ctx, ctx1, ctx2], C, KEYS7, wa, wb)
    got_a, got_b, kern = _ring_run(ring, C, KEYS7, wa, wb)
    _same((got_a, got_b), want, "default stream", kern)
    # B = 0: nothing launched, member 0's trace of the previous call stands
    before = ctx.last_kernels()
    ring.circuit_dev(C, [], None, None)
    assert T.lib.tfhe_amd_keyring_circuit_run_dev(ring.h, C.h, 0, T._ip(np.zeros(1, np.int32)), None, None, None) == 0
    assert ctx.last_kernels() == before
    # a caller's stream: the wire table arrives on that stream, ahead of the call, and only it is waited for
    st = torch.cuda.Stream()
    ha, hb = torch.from_numpy(wa).pin_memory(), torch.from_numpy(wb).pin_memory()
    da, db = torch.empty_like(ha, device="cuda"), torch.empty_like(hb, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        da.copy_(ha, non_blocking=True)
        db.copy_(hb, non_blocking=True)
    ring.circuit_dev(C, KEYS7, da, db, stream=st.cuda_stream)
    st.synchronize()
    _same((da.cpu().numpy(), db.cpu().numpy()), want, "caller's stream")
    # the host form equals the device form
    ins, outs = a + b, s + mn + lin
    out_a, out_b = ring.circuit_host(C, KEYS7, ins, wa[ins], wb[ins], outs)
    assert np.array_equal(out_a, want[0][outs]) and np.array_equal(out_b, want[1][outs])
    assert ring.circuit_host(C, [], ins, wa[ins][:, :0], wb[ins][:, :0], outs)[0].shape == (len(outs), 0, n_lwe)
    with pytest.raises(T.TfheAmdError):
        ring.circuit_host(C, KEYS7[:6] + [3], ins, wa[ins], wb[ins], outs)
    C.close()
