"""The launch forms of the constant (gate) blind rotation: which kernels each batch size takes, by the
names tfhe_amd_last_kernels reports, together with the results those launches produced, Torus32 for
Torus32 against the CPU oracle on a fixed sample: the first and last ciphertexts and both sides of
the half seam and of the pair seam."""
import numpy as np
import pytest

import dev_arena as DA
import tfhe_amd as T

pytestmark = pytest.mark.gpu

GUARD = "k_blind_rotate_v4(guard)"
KS_LARGE = {"k_keyswitch_v4", "k_keyswitch_v5(int8-mfma)", "k_keyswitch_v5(int8-mfma+split2)",
            "k_keyswitch_v5(int8-mfma+split4)", "k_keyswitch_v5(int8-mfma+split8)"}


def _cus():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nand_dev(ctx, keyset, rng, B):
    import torch
    x, y = rng.integers(0, 2, B), rng.integers(0, 2, B)
    (a_a, a_b), (b_a, b_b) = keyset.encrypt(x, rng), keyset.encrypt(y, rng)
    d = [torch.from_numpy(v).cuda() for v in (a_a, a_b, b_a, b_b)]
    r_a = torch.empty((B, T.n_lwe), dtype=torch.int32, device="cuda")
    r_b = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.gate_dev("NAND", r_a, r_b, *d)
    kern = ctx.last_kernels()
    ctx.sync()
    return (a_a, a_b, b_a, b_b), (r_a.cpu().numpy(), r_b.cpu().numpy()), kern


def _check_sample(okey, gate, ins, res, sample):
    idx = np.unique(np.clip(np.asarray(sample), 0, res[1].shape[0] - 1))
    assert len(idx) <= 16
    o_a, o_b = okey.gate_batch(gate, *(v[idx] for v in ins))
    assert np.array_equal(res[0][idx], o_a) and np.array_equal(res[1][idx], o_b), idx


def test_one_ciphertext_takes_the_lds_rotation(ctx, okey, keyset, rng):
    ins, res, kern = _nand_dev(ctx, keyset, rng, 1)
    _check_sample(okey, "NAND", ins, res, [0])
    assert kern == ["k_blind_rotate_v6(lds-rotation)", GUARD, "k_keyswitch_small"], kern


def test_above_one_per_cu_takes_the_paired_kernel(ctx, okey, keyset, rng):
    B = _cus() + 1   # odd: the last workgroup holds a padding ciphertext
    ins, res, kern = _nand_dev(ctx, keyset, rng, B)
    mid = (B // 2) & ~1   # ciphertexts mid, mid + 1 share a workgroup; mid - 1 | mid and mid + 1 | mid + 2 do not
    _check_sample(okey, "NAND", ins, res, [0, 1, 2, mid - 1, mid, mid + 1, mid + 2, B - 3, B - 2, B - 1])
    assert kern[:2] == ["k_blind_rotate_v6p(paired+reg-rotation+pair-sync)", GUARD], kern
    assert len(kern) == 3 and kern[2] in KS_LARGE, kern


def test_above_two_per_cu_takes_the_register_rotation(ctx, okey, keyset, rng):
    B = 2 * _cus() + 1
    ins, res, kern = _nand_dev(ctx, keyset, rng, B)
    mid = (B // 2) & ~1
    _check_sample(okey, "NAND", ins, res, [0, 1, 2, mid - 1, mid, mid + 1, mid + 2, B - 3, B - 2, B - 1])
    assert kern[:2] == ["k_blind_rotate_v6(reg-rotation)", GUARD], kern
    assert len(kern) == 3 and kern[2] in KS_LARGE, kern


def test_mux_halves_share_one_launch(ctx, okey, keyset, rng):
    """B = 1, two halves: rotations 0 | 1 are the half seam; one launch, each name once"""
    s, x, y = (rng.integers(0, 2, 1) for _ in range(3))
    ins = sum((keyset.encrypt(v, rng) for v in (s, x, y)), ())
    res = ctx.gate_host("MUX", *ins)
    kern = ctx.last_kernels()
    _check_sample(okey, "MUX", ins, res, [0])
    assert kern == ["k_blind_rotate_v6(lds-rotation)", GUARD, "k_keyswitch_small"], kern


def test_exact_generation_has_a_bare_name(ctx, okey, keyset, rng):
    try:
        T.select_kernel(4)
        ins, res, kern = _nand_dev(ctx, keyset, rng, 1)
    finally:
        T.select_kernel(0)
    _check_sample(okey, "NAND", ins, res, [0])
    assert kern == ["k_blind_rotate_v4", "k_keyswitch_small"], kern


def test_constant_circuit_level_takes_the_constant_rows_kernels(ctx, okey, keyset, rng):
    """one level of two constant gates, 5 instances: 10 rows x instances, 10 key switches"""
    import torch
    C = T.Circuit()
    a, b = C.inputs(2)
    outs = {"NAND": C.gate("NAND", a, b), "XOR": C.gate("XOR", a, b)}
    B = 5
    x, y = rng.integers(0, 2, B), rng.integers(0, 2, B)
    enc = {a: keyset.encrypt(x, rng), b: keyset.encrypt(y, rng)}
    wa = DA.poisoned((C.info()["wires"], B, T.n_lwe))
    wb = DA.poisoned((C.info()["wires"], B))
    for w, (e_a, e_b) in enc.items():
        wa[w] = torch.from_numpy(e_a).cuda()
        wb[w] = torch.from_numpy(e_b).cuda()
    torch.cuda.synchronize()   # the wires are filled on torch's stream, the circuit runs on the context's
    C.run_dev(ctx, B, wa, wb)
    kern = ctx.last_kernels()
    ctx.sync()
    ha, hb = wa.cpu().numpy(), wb.cpu().numpy()
    for gate, w in outs.items():
        o_a, o_b = okey.gate_batch(gate, *enc[a], *enc[b])
        assert np.array_equal(ha[w], o_a) and np.array_equal(hb[w], o_b), gate
    assert kern == ["k_blind_rotate_v6_rows(lds-rotation)", "k_blind_rotate_v4_rows(guard)", "k_keyswitch_small"], kern
    assert not any("lut" in k for k in kern), kern
