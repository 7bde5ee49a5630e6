"""BASELINE.json configs at their stated sizes on the MI355X (through the C ABI), each
decrypted against integer arithmetic and, where the oracle can afford
it, compared Torus32 bit for bit (P1):

  configs[1]: 1024 independent bootsNAND — ALL 1024 outputs bit-exact vs the oracle; the
              4096 batch of the metric: ALL 4096 outputs bit-exact;
  configs[2]: one 32-bit ripple-carry addition, through the circuit API and through the
              reference's unchanged Cipher::operator+ (cpuParallel/Cipher.cpp:348-392);
  configs[3]: 16 x 16-bit multiplication, batch 256 (multiplication.cu circuit's size);
  configs[4]: rows of the 64 x 64 16-bit matrix-vector product (matrixUtility path);
plus a Torus32 check of the circuit-row kernel (k_blind_rotate_v6_rows) against the oracle
for the three-input MAJ / XOR3 rows and the prefix adder's 2/1/1 threshold row."""
import json
import os
import subprocess

import numpy as np
import pytest

import dev_arena as DA
import matvec
import tfhe_amd as T

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLERS = os.path.join(REPO, "oracle", "_ref", "callers")
N, n = 1024, 500
E8 = 1 << 29


def _torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _gate_dev(ctx, gate, host):
    torch = _torch()
    B = host[0].shape[0]
    dev = [torch.from_numpy(v).cuda() for v in host]
    r_a = torch.empty((B, n), dtype=torch.int32, device="cuda")
    r_b = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.reserve(B)
    ctx.gate_dev(gate, r_a, r_b, *dev)
    ctx.sync()
    return r_a.cpu().numpy(), r_b.cpu().numpy()


def test_config1_batch_1024_all_bit_exact(ctx, okey, keyset, rng):
    """configs[1]: every one of the 1024 gates equals the oracle word for word."""
    B = 1024
    x, y = rng.integers(0, 2, B), rng.integers(0, 2, B)
    host = keyset.encrypt(x, rng) + keyset.encrypt(y, rng)
    ra, rb = _gate_dev(ctx, "NAND", host)
    assert np.array_equal(keyset.decrypt(ra, rb), 1 - (x & y))
    oa, ob = okey.gate_batch("NAND", *host)
    assert np.array_equal(ra, oa) and np.array_equal(rb, ob)


def test_metric_batch_4096_all_bit_exact(ctx, okey, keyset, rng):
    """The metric's batch 4096 (four one-round launches of 1024, the register-rotation kernel):
    truth table on all, and every one of the 4096 outputs — the launch seams included — equal
    to the oracle word for word."""
    B = 4096
    x, y = rng.integers(0, 2, B), rng.integers(0, 2, B)
    host = keyset.encrypt(x, rng) + keyset.encrypt(y, rng)
    ra, rb = _gate_dev(ctx, "NAND", host)
    assert np.array_equal(keyset.decrypt(ra, rb), 1 - (x & y))
    oa, ob = okey.gate_batch("NAND", *host)
    bad = np.flatnonzero((ra != oa).any(axis=1) | (rb != ob))
    assert bad.size == 0, f"{bad.size} ciphertexts differ, first {bad[:8]}"


def _bits(wires, x, nb):
    return dict(zip(wires, T.bits_of(x, nb)))


def test_config3_ripple_add_32bit_circuit(ctx, keyset, rng):
    """configs[2]: one 32-bit ripple-carry addition (depth 32) through the circuit API, plus
    a few more instances in the same launch sequence, incl. the carry-chain worst cases."""
    nb = 32
    C = T.Circuit()
    a, b = C.inputs(nb), C.inputs(nb)
    s, co = C.add(a, b)
    x = np.array([0xFFFFFFFF, 0x89ABCDEF, 1, 0x7FFFFFFF], dtype=np.int64)
    y = np.array([1, 0x76543211, 0xFFFFFFFF, 0x7FFFFFFF], dtype=np.int64)
    for B in (1, 4):
        got = C.run(ctx, B, {**_bits(a, x[:B], nb), **_bits(b, y[:B], nb)}, s + [co], keyset, rng)
        assert np.array_equal(T.int_of([got[w] for w in s + [co]]), x[:B] + y[:B])


def _callers_env():
    """Environment for the binaries in oracle/_ref/callers: their run path finds libtfhe_amd.so
    relative to the directory they were built into; this tree's library directory is named as well,
    so that binaries built in another checkout, or reached through a linked oracle/_ref, load the
    library under test."""
    lib = os.path.join(REPO, "cpu-gpu-tfhe_amd", "lib")
    old = os.environ.get("LD_LIBRARY_PATH")
    return dict(os.environ, LD_LIBRARY_PATH=lib + (os.pathsep + old if old else ""))


def _run_main(tmp_path, a, b):
    """The reference's client (main.cpp): key generation, encryption of a and b, the three files."""
    r = subprocess.run([os.path.join(CALLERS, "main"), str(a), str(b)], cwd=tmp_path,
                       env=_callers_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])


def _callers_built():
    return all(os.path.exists(os.path.join(CALLERS, f)) for f in ("main", "cipher_ops"))


def test_config3_cipher_operator_plus_32bit(tmp_path):
    """configs[2] on the reference's own caller: Cipher::operator+ (Cipher.cpp:348-392, 5 gates
    per bit through the TFHE C API, one gate at a time) on 32-bit operands, compiled unchanged
    against libtfhe_amd and run on the MI355X."""
    if not _callers_built():
        pytest.skip("oracle/_ref/callers not built (needs the reference sources at build time)")
    _run_main(tmp_path, 1, 2)
    for av, bv in ((3000000000, 1234567890), (0xFFFFFFFF, 1)):
        r = subprocess.run([os.path.join(CALLERS, "cipher_ops"), "add32", str(av), str(bv)], cwd=tmp_path,
                           env=_callers_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out["a"] == av and out["b"] == bv
        assert out["sum"] == (av + bv) % 2**32
        print(f"Cipher::operator+ 32-bit on the MI355X: {out['seconds']:.3f} s for 160 gates "
              f"({out['ms_per_gate']:.2f} ms each); context set-up (tfhe_amd_tier1_prepare) "
              f"{out['prepare_seconds']:.3f} s, then the first gate {out['first_gate_seconds'] * 1e3:.2f} ms")
        assert out["first_gate_seconds"] < 0.02, out   # the set-up is all in prepare
        # 160 dependent single gates at the B = 1 latency (~1.75 ms): the context set-up of the
        # first call (HIP init, key upload + conversion) is outside the timed addition
        assert out["seconds"] < 0.40, out


def test_cipher_operator_times_16bit_openmp(tmp_path):
    """The unchanged Cipher::operator* (Cipher.cpp:83-112) on 16-bit operands: sequential
    (Cipher.cpp as shipped) and with its own OpenMP loop switched on (-DPARALLEL, nThreads 4 and
    16), whose concurrent single-gate calls the Tier-1 coalescing queue batches; every product is
    right, and the team is not markedly slower than the sequential loop: with 16 threads the
    OpenMP reduction's serial combine (15 private sums folded by 160 dependent gates each, on one
    thread) is 2 400 of the 5 376 gates, so both runs are bound by the single-gate latency and
    their times are close (4.4-5.1 s vs 4.9 s measured); the bound leaves room for box-to-box
    variation."""
    if not (_callers_built() and os.path.exists(os.path.join(CALLERS, "cipher_ops_par"))):
        pytest.skip("oracle/_ref/callers not built (needs the reference sources at build time)")
    _run_main(tmp_path, 1, 2)
    av, bv = 0xBEEF, 0xFACE
    res = {}
    for exe, th in (("cipher_ops", 1), ("cipher_ops_par", 4), ("cipher_ops_par", 16)):
        r = subprocess.run([os.path.join(CALLERS, exe), "mul16", str(av), str(bv), str(th)], cwd=tmp_path,
                           env=_callers_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out["prod"] == av * bv, out
        res[f"{exe}:{th}"] = out
    print(json.dumps(res))
    assert res["cipher_ops_par:16"]["seconds"] <= res["cipher_ops:1"]["seconds"] * 1.3, res
    assert res["cipher_ops_par:4"]["seconds"] <= res["cipher_ops:1"]["seconds"] * 1.1, res


def test_config4_mul_16x16_batch256(ctx, keyset, rng):
    """configs[3]: 256 independent 16 x 16 -> 32-bit products in one circuit evaluation."""
    nb, B = 16, 256
    C = T.Circuit()
    a, b = C.inputs(nb), C.inputs(nb)
    p = C.mul(a, b)
    x = rng.integers(0, 2**nb, B)
    y = rng.integers(0, 2**nb, B)
    x[:2] = [2**nb - 1, 0]
    y[:2] = [2**nb - 1, 2**nb - 1]
    got = C.run(ctx, B, {**_bits(a, x, nb), **_bits(b, y, nb)}, p, keyset, rng)
    assert np.array_equal(T.int_of([got[w] for w in p]), x * y)


def test_config5_matvec_rows_64x64_16bit(ctx, keyset, rng):
    """configs[4]: two rows of y = A x for a 64 x 64 16-bit matrix (each row one 64-term dot
    product circuit; the rows are the circuit's instances, as one rank's shard would be)."""
    torch = _torch()
    cols, nbits = 64, 16
    C, a_w, x_w, y_w = matvec.build(T, cols, nbits)
    A = rng.integers(0, 2**nbits, (2, cols))
    A[0] = 2**nbits - 1                              # the largest row sum
    xv = rng.integers(0, 2**nbits, cols)
    xv[:8] = 2**nbits - 1
    y, _ = matvec.run_rows_gpu(T, torch, ctx, keyset, C, a_w, x_w, y_w, A, xv, nbits, rng, reps=1)
    assert np.array_equal(y, (A.astype(object) @ xv.astype(object)).astype(np.int64))


def test_config5_matvec_64x64_16bit_all_rows_multi_device(okey, keyset, rng):
    """configs[4] in full: all 64 rows of y = A x (64 x 64, 16-bit) from one host process through
    the library's multi-device circuit run (tfhe_amd_multi_circuit_run_host), the rows sharded over
    the device slots — every visible GPU, or two contexts on device 0 of a one-GPU box.  Every row
    decrypts to the integer product; the level-1 partial products (AND rows of input bits) of a
    sample of rows, both shards' seam included, equal the oracle's bootsAND word for word."""
    torch = _torch()
    n_dev = torch.cuda.device_count()
    slots = list(range(n_dev)) if n_dev > 1 else [0, 0]
    cols, nbits, R = 64, 16, 64
    C, a_w, x_w, y_w = matvec.build(T, cols, nbits)
    A = rng.integers(0, 2**nbits, (R, cols))
    A[0] = 2**nbits - 1
    xv = rng.integers(0, 2**nbits, cols)
    xv[:8] = 2**nbits - 1
    inputs = set(a_w[0] + x_w[0])
    ands = []   # AND rows whose inputs are both input wires
    for w in range(C.info()["wires"]):
        kind, gate, _, _, ins = C.node(w)
        if kind == 1 and gate == T.GATES["AND"] and ins[0] in inputs and ins[1] in inputs:
            ands.append((w, ins[0], ins[1]))
        if len(ands) == 6:
            break
    assert ands, "no level-1 partial products found"
    m = T.MultiContext(keyset.bk, keyset.ksk, slots)
    try:
        y, dt, extra, (wires, in_a, in_b) = matvec.run_rows_multi(
            T, m, keyset, C, a_w, x_w, y_w, A, xv, nbits, rng, extra_out=[w for w, _, _ in ands])
    finally:
        m.close()
    assert np.array_equal(y, (A.astype(object) @ xv.astype(object)).astype(np.int64))
    pos = {w: k for k, w in enumerate(wires)}
    half = T.shard_range(R, 1, len(slots))[0]
    rows = np.unique([0, half - 1, half, R - 1])
    for w, i0, i1 in ands:
        o_a, o_b = okey.gate_batch("AND", in_a[pos[i0]][rows], in_b[pos[i0]][rows], in_a[pos[i1]][rows],
                                   in_b[pos[i1]][rows])
        assert np.array_equal(extra[w][0][rows], o_a) and np.array_equal(extra[w][1][rows], o_b), w
    print(f"64x64 16-bit matvec, all 64 rows over {len(slots)} device slots: {dt:.2f} s")


def _circuits_for_torus32():
    """(name, circuit, {input wire: bit plane}) cases: BASELINE config 3 at its size (one 32-bit
    ripple-carry addition), and config 4's multiplier, the comparison, min and division builders
    at 8 / 6 bits so that the oracle checks every wire within seconds."""
    r = np.random.default_rng(77)
    B = 2
    out = []
    C = T.Circuit(); a, b = C.inputs(32), C.inputs(32); C.add(a, b)
    x = np.array([0xFFFFFFFF, 0x89ABCDEF]); y = np.array([1, 0x76543211])
    out.append(("config3 add32", C, {**_bits(a, x, 32), **_bits(b, y, 32)}, B))
    for name, nb, build in (("mul8x8", 8, lambda C, a, b: C.mul(a, b)),
                            ("signed a > b", 8, lambda C, a, b: C.compare(a, b, "GT", signed=True)),
                            ("minimum", 8, lambda C, a, b: C.minmax(a, b)),
                            ("divu 6-bit", 6, lambda C, a, b: C.divu(a, b))):
        C = T.Circuit(); a, b = C.inputs(nb), C.inputs(nb); build(C, a, b)
        x = r.integers(0, 2**nb, B); y = r.integers(1, 2**nb, B)
        x[0] = 2**nb - 1
        out.append((name, C, {**_bits(a, x, nb), **_bits(b, y, nb)}, B))
    return out


def test_circuits_every_wire_torus32_vs_oracle(ctx, okey, keyset, rng):
    """Whole circuits Torus32-exact: every wire of config 3's 32-bit ripple-carry addition (depth
    32) and of the 8x8 multiplier, signed comparison, minimum and 6-bit division, evaluated on the
    GPU (level-batched rows, bootstrap-free nodes folded in) equals a node-by-node evaluation with
    the exact oracle's bootstraps and key switches (tests/circuit_oracle.py), word for word."""
    import circuit_oracle
    torch = _torch()
    for name, C, bits, B in _circuits_for_torus32():
        n_w = C.info()["wires"]
        enc = {w: keyset.encrypt(v, rng) for w, v in bits.items()}
        wa = DA.poisoned((n_w, B, n))      # every wire the run does not write stays poison
        wb = DA.poisoned((n_w, B))
        for w, (ea, eb) in enc.items():
            wa[w] = torch.from_numpy(ea).cuda()
            wb[w] = torch.from_numpy(eb).cuda()
        C.run_dev(ctx, B, wa, wb)
        torch.cuda.synchronize()
        ha, hb = wa.cpu().numpy(), wb.cpu().numpy()
        W = circuit_oracle.eval_circuit(C, okey, enc, B)
        bad = [w for w in range(n_w) if not (np.array_equal(ha[w], W[w][0]) and np.array_equal(hb[w], W[w][1]))]
        assert not bad, (name, bad[:10])
        ref = C.eval_plain(bits)
        for w in range(n_w):
            dec = keyset.decrypt(ha[w], hb[w])
            assert np.array_equal(dec, np.broadcast_to(ref[w], dec.shape)), (name, w)


def test_config4_mul_16x16_batch256_wires_torus32_sampled(ctx, okey, keyset, rng):
    """configs[3] at its size (256 independent 16 x 16 products, 931 bootstraps each, one circuit
    run): every wire of instances 0, 127 and 255 equals the exact oracle's node-by-node evaluation
    of those instances word for word, and all 256 products decrypt right."""
    import circuit_oracle
    torch = _torch()
    nb, B = 16, 256
    C = T.Circuit()
    a, b = C.inputs(nb), C.inputs(nb)
    p = C.mul(a, b)
    x = rng.integers(0, 2**nb, B)
    y = rng.integers(0, 2**nb, B)
    x[0], y[0] = 2**nb - 1, 2**nb - 1
    bits = {**_bits(a, x, nb), **_bits(b, y, nb)}
    n_w = C.info()["wires"]
    enc = {w: keyset.encrypt(v, rng) for w, v in bits.items()}
    wa = DA.poisoned((n_w, B, n))      # every wire the run does not write stays poison
    wb = DA.poisoned((n_w, B))
    for w, (ea, eb) in enc.items():
        wa[w] = torch.from_numpy(ea).cuda()
        wb[w] = torch.from_numpy(eb).cuda()
    C.run_dev(ctx, B, wa, wb)
    torch.cuda.synchronize()
    ha, hb = wa.cpu().numpy(), wb.cpu().numpy()
    assert np.array_equal(T.int_of([keyset.decrypt(ha[w], hb[w]) for w in p]), x * y)
    k = np.array([0, 127, 255])
    W = circuit_oracle.eval_circuit(C, okey, {w: (ea[k], eb[k]) for w, (ea, eb) in enc.items()}, len(k))
    bad = [w for w in range(n_w) if not (np.array_equal(ha[w][k], W[w][0]) and np.array_equal(hb[w][k], W[w][1]))]
    assert not bad, bad[:10]


def test_circuit_rows_torus32_vs_oracle(ctx, okey, keyset, rng):
    """k_blind_rotate_v6_rows + the circuit key switch: each bootstrapped row's output equals
    the oracle's bootstrap + key switch of the same linear combination, word for word, for
    MAJ (1, 1, 1), XOR3 (-2, -2, -2) and the 2/1/1 threshold row of the prefix adder."""
    torch = _torch()
    C = T.Circuit()
    x, y, z = C.inputs(3)
    rows = {"MAJ": (C.gate("MAJ", x, y, z), 0, (1, 1, 1)),
            "XOR3": (C.gate("XOR3", x, y, z), 0, (-2, -2, -2)),
            "THRESH_2_1_1": (C.lincomb(E8, 2, x, 1, y, 1, z), E8, (2, 1, 1))}
    B = 24
    bits = [rng.integers(0, 2, B) for _ in range(3)]
    n_w = C.info()["wires"]
    wa = DA.poisoned((n_w, B, n))      # every wire the run does not write stays poison
    wb = DA.poisoned((n_w, B))
    enc = [keyset.encrypt(v, rng) for v in bits]
    for w, (ea, eb) in zip((x, y, z), enc):
        wa[w] = torch.from_numpy(ea).cuda()
        wb[w] = torch.from_numpy(eb).cuda()
    C.run_dev(ctx, B, wa, wb)
    torch.cuda.synchronize()
    ha, hb = wa.cpu().numpy(), wb.cpu().numpy()
    for name, (w, c0, s) in rows.items():
        la = sum(np.int64(si) * e[0].astype(np.int64) for si, e in zip(s, enc))
        lb = np.int64(c0) + sum(np.int64(si) * e[1].astype(np.int64) for si, e in zip(s, enc))
        u_a, u_b = okey.woks_batch(E8, la, lb)
        oa, ob = okey.keyswitch_batch(u_a, u_b)
        assert np.array_equal(ha[w], oa) and np.array_equal(hb[w], ob), name
    ref = C.eval_plain({x: bits[0], y: bits[1], z: bits[2]})
    for name, (w, _, _) in rows.items():
        assert np.array_equal(keyset.decrypt(ha[w], hb[w]), ref[w]), name


def test_matmat_4x4_16bit(ctx, keyset, rng):
    """§8(f) row 4: the encrypted 4 x 4 16-bit matrix product (the paper's Table IX size), one
    dot-product circuit per output element, all 16 elements as the circuit's instances."""
    import matmat
    torch = _torch()
    m = k = n = 4
    nbits = 16
    A = rng.integers(0, 2**nbits, (m, k))
    Bm = rng.integers(0, 2**nbits, (k, n))
    A[0] = 2**nbits - 1
    C, a_w, b_w, c_w = matmat.build(T, k, nbits)
    got, t = matmat.run_block_gpu(T, torch, ctx, keyset, C, a_w, b_w, c_w, A, Bm, nbits, rng)
    want = ((A.astype(object) @ Bm.astype(object)) % 2**nbits).astype(np.int64)
    assert np.array_equal(got, want)
    print(f"4x4 16-bit encrypted matrix product: {t:.3f} s (paper, GTX 1080: 5.90 min)")
