"""Mixed-key batches: one ring call over ciphertexts of several cloud keys against
the same ciphertexts run key by key through the single-key entry points.

The engine is bit-exact and deterministic, so every comparison is word for word.  Keys: K0 the
session keyset, K1 a second keyset (another seed), K2 guard_cases.head_key(K0.bk) with K0's
key-switching key — the adversarial key on which the unguarded fp64 rotation is wrong, so a row
rotated, or recomputed by the guard, under another slot's key shows as wrong words."""
import numpy as np
import pytest

import dev_arena as DA
import guard_cases as G
import tfhe_amd as T

pytestmark = pytest.mark.gpu

N, n_lwe = 1024, 500
BINARY = ["NAND", "OR", "AND", "XOR", "XNOR", "NOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
TRUTH = {"NAND": lambda a, b, c: 1 - (a & b), "OR": lambda a, b, c: a | b, "AND": lambda a, b, c: a & b,
         "XOR": lambda a, b, c: a ^ b, "XNOR": lambda a, b, c: 1 - (a ^ b), "NOR": lambda a, b, c: 1 - (a | b),
         "ANDNY": lambda a, b, c: (1 - a) & b, "ANDYN": lambda a, b, c: a & (1 - b), "ORNY": lambda a, b, c: (1 - a) | b,
         "ORYN": lambda a, b, c: a | (1 - b), "MUX": lambda a, b, c: np.where(a == 1, b, c), "NOT": lambda a, b, c: 1 - a,
         "COPY": lambda a, b, c: a}
MK6 = "k_blind_rotate_v6_rows(multi-key+"
MK4_GUARD = "k_blind_rotate_v4_rows(multi-key+guard)"
MK4_EXACT = "k_blind_rotate_v4_rows(multi-key)"


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


def _both(ctx, outs, inps, call):
    """call(views) once per poison on fresh arenas (tests/dev_arena.py) holding outs [(name, shape)]
    and inps [(name, host array)] -> [(arena, {name: host copy of the out}, kernels)] per poison"""
    runs = []
    for poison in DA.POISONS:
        arena, v = DA.Arena.of("cuda", poison, outs, inps)
        call(v)
        kern = ctx.last_kernels()
        ctx.sync()
        runs.append((arena, {name: v[name].cpu().numpy() for name, _ in outs}, kern))
    return runs


def _verdict(runs, want, what, forms):
    """the outputs do not depend on what they held before the call; they equal `want` word for word;
    no band word changed and every input is unchanged; every name of `forms` begins some kernel name"""
    (a0, got0, kern0), (a1, got1, kern1) = runs
    for name in got0:
        assert np.array_equal(got0[name], got1[name]), f"{what}: {name} depends on what it held before the call"
        assert np.array_equal(got0[name], want[name]), f"{what}: {name} differs from the per-key contexts"
    for poison, arena in zip(DA.POISONS, (a0, a1)):
        try:
            arena.check()
        except AssertionError as e:
            raise AssertionError(f"{what} ({poison} poison): {e}") from None
    for kern in (kern0, kern1):
        for frag in forms:
            assert any(k.startswith(frag) for k in kern), (what, frag, kern)


def _per_key(ctxs, gates, key_of, ins):
    """the batch key by key through each context's own single-key entry points: gate_mixed_host on the
    slot's bootstrapped gates; NOT / COPY are the reference's lweNegate / lweCopy of ca"""
    gates, key_of = list(gates), np.asarray(key_of)
    B = len(gates)
    r_a, r_b = np.zeros((B, n_lwe), np.int32), np.zeros(B, np.int32)
    for slot, c in enumerate(ctxs):
        idx = np.array([i for i in range(B) if key_of[i] == slot and gates[i] not in ("NOT", "COPY")], dtype=np.int64)
        if idx.size:
            sub = [None if x is None else np.ascontiguousarray(x[idx]) for x in ins]
            r_a[idx], r_b[idx] = c.gate_mixed_host([gates[i] for i in idx], *sub)
    for i, g in enumerate(gates):
        if g in ("NOT", "COPY"):
            s = -1 if g == "NOT" else 1
            r_a[i], r_b[i] = G.wrap(s * ins[0][i].astype(np.int64)), G.wrap(s * int(ins[1][i]))
    return r_a, r_b


GATES7 = ["NAND", "MUX", "NOT", "XOR", "MUX", "ORNY", "AND"]
KEYS7 = [2, 0, 1, 0, 2, 1, 0]


def _batch7(keysets, rng):
    """test 1's batch: valid encryptions of random bits, entry i under the secret key of its slot"""
    bits = rng.integers(0, 2, (3, 7))
    ins = [np.zeros((7, n_lwe) if k % 2 == 0 else 7, np.int32) for k in range(6)]
    for i, slot in enumerate(KEYS7):
        for k in range(3):
            a, b = keysets[slot].encrypt(bits[k, i:i + 1], rng)
            ins[2 * k][i], ins[2 * k + 1][i] = a[0], b[0]
    return bits, ins


def test_mixed_key_mixed_gate_parity_and_decryption(ring, ctx, ctx1, ctx2, keyset, keyset1, okey, rng):
    """(1) B = 7 over three keys out of order, MUX and NOT among the kinds: every word equals each key's
    own gate_mixed_host on its subset, the K0 subset also the CPU oracle; (2) the K0 and K1 results
    decrypt under their own secret keys to the truth tables (K2 shares K0's secret key: its
    bootstrapping key is not a valid one, nothing is decrypted there)"""
    bits, ins = _batch7([keyset, keyset1, keyset], rng)
    got = ring.gate_host(GATES7, KEYS7, *ins)
    kern = ctx.last_kernels()
    want = _per_key([ctx, ctx1, ctx2], GATES7, KEYS7, ins)
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1] != want[1]))
    assert bad.size == 0, (bad, kern)
    assert any(k.startswith(MK6) and "lds-rotation" in k for k in kern) and MK4_GUARD in kern, kern
    for i in (1, 3, 6):      # slot 0's bootstrapped gates against the oracle
        cc = (ins[4][i:i + 1], ins[5][i:i + 1]) if GATES7[i] == "MUX" else ()
        o_a, o_b = okey.gate_batch(GATES7[i], *[x[i:i + 1] for x in ins[:4]], *cc)
        assert np.array_equal(got[0][i], o_a[0]) and got[1][i] == o_b[0], (i, GATES7[i])
    for K, slot in ((keyset, 0), (keyset1, 1)):
        idx = [i for i in range(7) if KEYS7[i] == slot]
        dec = K.decrypt(got[0][idx], got[1][idx])
        for j, i in enumerate(idx):
            assert dec[j] == TRUTH[GATES7[i]](bits[0, i], bits[1, i], bits[2, i]), (slot, i, GATES7[i])


def test_one_key_ring_and_the_same_context_twice(ctx, keyset, rng):
    """(3) a ring of one key is gate_mixed_host exactly; a ring naming K0 in two slots gives the same
    words whichever slot a ciphertext names"""
    B = 5
    gates = ["XNOR", "MUX", "NAND", "MUX", "ANDYN"]
    ins = []
    for _ in range(3):
        ins += list(keyset.encrypt(rng.integers(0, 2, B), rng))
    want = ctx.gate_mixed_host(gates, *ins)
    one = T.KeyRing([ctx])
    two = T.KeyRing([ctx, ctx])
    try:
        assert len(one) == 1 and len(two) == 2 and one.device == 0
        got = one.gate_host(gates, [0] * B, *ins)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        for key_of in ([0, 1, 0, 1, 1], [1, 1, 1, 1, 1], [1, 0, 0, 0, 1]):
            got = two.gate_host(gates, key_of, *ins)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), key_of
    finally:
        one.close()
        two.close()


def test_guard_recomputes_under_the_rows_own_key(ring, ctx, ctx2):
    """(4) the same dirty samples (random words everywhere) on slot K2, where the fp64 rotation is
    flagged and the exact kernel recomputes it, and on slot K0, where nothing is flagged: the K2
    outputs equal those of the single context on K2 (whose own guard recomputes them), the K0 outputs
    K0's own, and the recomputed count is exactly the K2 rows.  A recomputation under member 0's key
    would give the K2 rows K0's words."""
    rng = np.random.default_rng(4242)
    nd = 4
    d_a, d_b = G.dirty(rng, nd)
    c_a, c_b = G.clean(rng, 1)
    # (sample, slot) per entry: every dirty sample once on K2 and once on K0, interleaved; a clean one on K2
    entries = [(0, 2), (0, 0), (1, 2), (None, 2), (1, 0), (2, 2), (2, 0), (3, 2), (3, 0)]
    x_a = np.stack([c_a[0] if k is None else d_a[k] for k, _ in entries])
    x_b = np.array([c_b[0] if k is None else d_b[k] for k, _ in entries], np.int32)
    key_of = np.array([slot for _, slot in entries])
    ins = G.gate_inputs("NAND", x_a, x_b)
    gates = ["NAND"] * len(entries)
    for c in (ctx, ctx2):
        c.guard_stats(reset=True)
    got = ring.gate_host(gates, key_of, *ins)
    kern = ctx.last_kernels()
    dist, redo = ctx.guard_stats(reset=True)
    want_a, want_b = np.zeros_like(got[0]), np.zeros_like(got[1])
    for slot, c in ((0, ctx), (2, ctx2)):
        idx = np.flatnonzero(key_of == slot)
        want_a[idx], want_b[idx] = c.gate_mixed_host(["NAND"] * idx.size, *[x[idx] for x in ins])
    assert ctx2.guard_stats(reset=True)[1] == nd     # the reference side did recompute the dirty rows
    assert ctx.guard_stats(reset=True)[1] == 0       # and K0's own run flagged none of them
    bad = np.flatnonzero((got[0] != want_a).any(axis=1) | (got[1] != want_b))
    assert bad.size == 0, (bad, key_of[bad], kern)
    # the same sample gives other words under K2 than under K0: the comparison tells the keys apart
    for k in range(nd):
        i, j = entries.index((k, 2)), entries.index((k, 0))
        assert (got[0][i] != got[0][j]).any(), k
    assert redo == nd and dist >= 0.125, (redo, dist, kern)
    assert MK4_GUARD in kern, kern


@pytest.mark.parametrize("form", ["reg", "two_rounds"])
def test_launch_geometry(ctx, ctx1, form):
    """(5) CUs + 4 rows take the register rotation; 4 CUs + 6 rows take two rounds, with the second
    round's base offset and a key group straddling the round boundary (slot = i mod 3 over
    [K0, K1, K0]: the last group covers rows 2/3 .. 1 of the batch).  Random input words (bit-exact
    paths need no valid encryption), MUX entries among them so rows and entries differ; compared
    with the per-key contexts."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = cus + 4 if form == "reg" else 4 * cus + 6
    n_mux = 5
    B = rows - n_mux
    rng = np.random.default_rng(rows)
    gates = [BINARY[i % len(BINARY)] for i in range(B)]
    for i in rng.choice(B, n_mux, replace=False):
        gates[int(i)] = "MUX"
    key_of = np.arange(B) % 3
    ins = []
    for _ in range(3):
        ins += [_rand32(rng, (B, n_lwe)), _rand32(rng, B)]
    ring3 = T.KeyRing([ctx, ctx1, ctx])
    try:
        assert ring3.plan(key_of, gates)[2] == rows
        d = [_dev(x) for x in ins]
        r_a, r_b = DA.poisoned((B, n_lwe)), DA.poisoned((B,))
        torch.cuda.synchronize()
        ring3.gate_dev(gates, key_of, r_a, r_b, *d)
        kern = ctx.last_kernels()
        ctx.sync()
        got = r_a.cpu().numpy(), r_b.cpu().numpy()
    finally:
        ring3.close()
    want = _per_key([ctx, ctx1, ctx], gates, key_of, ins)
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1] != want[1]))
    assert bad.size == 0, (form, bad[:10], bad.size, kern)
    assert MK6 + "reg-rotation)" in kern, kern
    if form == "two_rounds":   # the second round: 6 rows, lds rotation
        assert MK6 + "lds-rotation)" in kern, kern
    assert [k for k in kern if k.startswith("keyring_keyswitch")] == [
        f"keyring_keyswitch(slot={s}+n={int((key_of == s).sum())})" for s in range(3)], kern


def test_exact_generation(ring, ctx, ctx1, ctx2, keyset, keyset1, rng):
    """(6) select_kernel(4): the ring runs through the exact kernel alone and gives the same words"""
    bits, ins = _batch7([keyset, keyset1, keyset], rng)
    want = ring.gate_host(GATES7, KEYS7, *ins)
    T.select_kernel(4)
    try:
        got = ring.gate_host(GATES7, KEYS7, *ins)
        kern = ctx.last_kernels()
    finally:
        T.select_kernel(0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert MK4_EXACT in kern and not any("v6" in k or "guard" in k for k in kern), kern


def test_lut_form(ring, ctx, ctx1, keyset, keyset1, rng):
    """(7) p = 4 tables, B = 6 over K0 and K1, two tables and a lut_index: host and device forms equal
    each key's lut_bootstrap_host"""
    torch = _torch()
    p = 4
    tv = np.stack([T.lut_table(p, T.lut_encode(np.array([1, 3, 0, 2]), p)),
                   T.lut_table(p, T.lut_encode(np.array([2, 2, 1, 0]), p))])
    key_of = np.array([1, 0, 0, 1, 1, 0])
    lut_index = np.array([0, 1, 1, 0, 1, 0], np.int32)
    m = rng.integers(0, p, 6)
    x_a, x_b = np.zeros((6, n_lwe), np.int32), np.zeros(6, np.int32)
    for i in range(6):
        a, b = (keyset, keyset1)[key_of[i]].encrypt_digits(m[i:i + 1], p, rng)
        x_a[i], x_b[i] = a[0], b[0]
    want_a, want_b = np.zeros_like(x_a), np.zeros_like(x_b)
    for slot, c in ((0, ctx), (1, ctx1)):
        idx = np.flatnonzero(key_of == slot)
        want_a[idx], want_b[idx] = c.lut_bootstrap_host(tv, x_a[idx], x_b[idx], lut_index=lut_index[idx])
    got = ring.lut_bootstrap_host(tv, key_of, x_a, x_b, lut_index=lut_index)
    kern = ctx.last_kernels()
    assert np.array_equal(got[0], want_a) and np.array_equal(got[1], want_b), kern
    assert any(k.startswith("k_blind_rotate_v6_rows(lut+multi-key+") for k in kern), kern
    r_a, r_b = DA.poisoned((6, n_lwe)), DA.poisoned((6,))
    torch.cuda.synchronize()
    ring.lut_bootstrap_dev(_dev(tv), key_of, r_a, r_b, _dev(x_a), _dev(x_b), lut_index=_dev(lut_index))
    ctx.sync()
    assert np.array_equal(r_a.cpu().numpy(), want_a) and np.array_equal(r_b.cpu().numpy(), want_b)
    # no lut_index: table 0 for everyone
    got0 = ring.lut_bootstrap_host(tv, key_of, x_a, x_b)
    for slot, c in ((0, ctx), (1, ctx1)):
        idx = np.flatnonzero(key_of == slot)
        w = c.lut_bootstrap_host(tv, x_a[idx], x_b[idx])
        assert np.array_equal(got0[0][idx], w[0]) and np.array_equal(got0[1][idx], w[1])
    # and the results decrypt to the tables' values under each key
    f = np.array([[1, 3, 0, 2], [2, 2, 1, 0]])
    for slot, K in ((0, keyset), (1, keyset1)):
        idx = np.flatnonzero(key_of == slot)
        assert np.array_equal(T.lut_decode(K.phase(got[0][idx], got[1][idx]), p), f[lut_index[idx], m[idx]])


def test_write_discipline_gate_dev(ring, ctx, ctx1, ctx2, keyset, keyset1):
    """(8) the device gate form under both poisons (tests/dev_arena.py): res [0, B) written and nothing
    beyond, independent of what res held, inputs unchanged"""
    rng = np.random.default_rng(8801)
    _, ins = _batch7([keyset, keyset1, keyset], rng)
    names = ["ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b"]
    runs = _both(ctx, [("res_a", (7, n_lwe)), ("res_b", (7,))], list(zip(names, ins)),
                    lambda v: ring.gate_dev(GATES7, KEYS7, v["res_a"], v["res_b"], *[v[n] for n in names]))
    want = _per_key([ctx, ctx1, ctx2], GATES7, KEYS7, ins)
    _verdict(runs, {"res_a": want[0], "res_b": want[1]}, "keyring gate_dev seed 8801",
             (MK6, MK4_GUARD, "k_ring_linear", "k_keyswitch_small"))


def test_write_discipline_lut_dev(ring, ctx, ctx1, keyset, keyset1):
    rng = np.random.default_rng(8802)
    B = 5
    tv = np.stack([T.lut_table(4, T.lut_encode(np.array([3, 0, 1, 2]), 4)), _rand32(rng, N)])
    key_of = [1, 0, 1, 1, 0]
    lut_index = np.array([1, 0, 0, 1, 1], np.int32)
    x_a, x_b = _rand32(rng, (B, n_lwe)), _rand32(rng, B)
    inps = [("tv", tv), ("lut_index", lut_index), ("x_a", x_a), ("x_b", x_b)]
    runs = _both(ctx, [("res_a", (B, n_lwe)), ("res_b", (B,))], inps,
                    lambda v: ring.lut_bootstrap_dev(v["tv"], key_of, v["res_a"], v["res_b"], v["x_a"], v["x_b"],
                                                     lut_index=v["lut_index"]))
    want_a, want_b = np.zeros_like(x_a), np.zeros_like(x_b)
    for slot, c in ((0, ctx), (1, ctx1)):
        idx = np.flatnonzero(np.array(key_of) == slot)
        want_a[idx], want_b[idx] = c.lut_bootstrap_host(tv, x_a[idx], x_b[idx], lut_index=lut_index[idx])
    _verdict(runs, {"res_a": want_a, "res_b": want_b}, "keyring lut_dev seed 8802",
             ("k_blind_rotate_v6_rows(lut+multi-key+", "k_blind_rotate_v4_rows(lut+multi-key+guard)"))


def test_refused_call_writes_nothing(ring, ctx, keyset, keyset1):
    torch = _torch()
    rng = np.random.default_rng(8803)
    _, ins = _batch7([keyset, keyset1, keyset], rng)
    names = ["ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b"]
    arena, v = DA.Arena.of("cuda", "index", [("res_a", (7, n_lwe)), ("res_b", (7,))], list(zip(names, ins)))
    before = v["res_a"].clone(), v["res_b"].clone()
    torch.cuda.synchronize()
    for key_of, gates in ((KEYS7[:6] + [3], GATES7), (KEYS7[:6] + [-1], GATES7), (KEYS7, GATES7[:6] + [99]),
                          (KEYS7, GATES7[:6] + ["CONST"])):
        with pytest.raises(T.TfheAmdError):
            ring.gate_dev(gates, key_of, v["res_a"], v["res_b"], *[v[n] for n in names])
    with pytest.raises(T.TfheAmdError):
        ring.lut_bootstrap_dev(torch.zeros((1, N), dtype=torch.int32, device="cuda"), [0] * 6 + [5], v["res_a"],
                               v["res_b"], v["ca_a"], v["ca_b"])
    torch.cuda.synchronize()
    assert torch.equal(v["res_a"], before[0]) and torch.equal(v["res_b"], before[1])
    arena.check()


def test_edge_cases(ring, ctx, ctx1, ctx2, keyset, keyset1, rng):
    """(9) B = 0 is OK with no launch; an empty middle group gets no key-switch launch; a caller's
    stream is honoured by gate_dev"""
    torch = _torch()
    _, ins = _batch7([keyset, keyset1, keyset], rng)
    # B = 0: nothing launched, member 0's trace of the previous call stands
    ring.gate_host(GATES7, KEYS7, *ins)
    before = ctx.last_kernels()
    empty = [x[:0] for x in ins]
    r = ring.gate_host([], [], *empty)
    assert r[0].shape == (0, n_lwe) and ctx.last_kernels() == before
    assert T.lib.tfhe_amd_keyring_gate_batch_dev(ring.h, 0, None, None, *([None] * 8), None) == 0
    assert T.lib.tfhe_amd_keyring_bootstrap_lut_batch_dev(ring.h, 0, None, 1, 1, *([None] * 5), None) == 0
    # an empty middle group: slots 0 and 2 only
    key_of = [2, 0, 0, 0, 2, 2, 0]
    got = ring.gate_host(GATES7, key_of, *ins)
    kern = ctx.last_kernels()
    want = _per_key([ctx, ctx1, ctx2], GATES7, key_of, ins)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert [k for k in kern if k.startswith("keyring_keyswitch")] == ["keyring_keyswitch(slot=0+n=3)",
                                                                      "keyring_keyswitch(slot=2+n=3)"], kern
    # a caller's stream: the inputs arrive on that stream, in stream order ahead of the call, and only
    # that stream is waited for
    st = torch.cuda.Stream()
    host = [torch.from_numpy(x).pin_memory() for x in ins]
    d = [torch.empty_like(h, device="cuda") for h in host]
    r_a, r_b = DA.poisoned((7, n_lwe)), DA.poisoned((7,))
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for dst, src in zip(d, host):
            dst.copy_(src, non_blocking=True)
    ring.gate_dev(GATES7, KEYS7, r_a, r_b, *d, stream=st.cuda_stream)
    st.synchronize()
    want = _per_key([ctx, ctx1, ctx2], GATES7, KEYS7, ins)
    assert np.array_equal(r_a.cpu().numpy(), want[0]) and np.array_equal(r_b.cpu().numpy(), want[1])
