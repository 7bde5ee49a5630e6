"""Differential fuzz of the circuit compiler on the GPU: seeded random DAGs that mix gate rows, MUX
pairs, LUT rows, many-LUT rows of several log_nu with their further outputs, adder cells and
bootstrap-free nodes in one level (tests/dag_fuzz.py), run through run_dev, and EVERY wire's 501
words per instance compared with the node-by-node evaluation of tests/dag_oracle.py, which folds
nothing.  Results are bit-exact: there is no tolerance.  Every assertion carries its seed.

Oracle results are computed once per (seed, profile, B) and shared by the modes below: the default
guarded path, the guard at threshold 0, the exact kernel generation, a two-slot MultiContext with
an uneven shard, and a circuit that regrows its scratch and then grows three nodes."""
import time

import numpy as np
import pytest

import dev_arena as DA
import dag_fuzz as DF
import dag_oracle as DO
import tfhe_amd as T

pytestmark = pytest.mark.gpu

n_lwe = 500


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_cache = {}


def _case(okey, seed, profile, B):
    """(C, input wires, schedule, inputs, oracle wires) of a case at B instances, once per process"""
    ck = (seed, profile)
    if ck not in _cache:
        C, ins, F = DF.make_case(seed, profile, _cus())
        _cache[ck] = (C, ins, DF.schedule(C))
    C, ins, sched = _cache[ck]
    key = (seed, profile, B)
    if key not in _cache:
        enc = DF.random_inputs(seed, ins, B)
        t = time.time()
        W = DO.eval_circuit(C, okey, enc, B)
        print(f"dag_oracle seed {seed} ({profile}) B = {B}: {sched['bootstraps'] * B} bootstraps, "
              f"{time.time() - t:.2f} s")
        _cache[key] = (enc, W)
    return (C, ins, sched) + _cache[key]


def _shape(profile):
    return {"wide": DF.wide_B(_cus()), "seam": DF.seam_shape(_cus())[1]}[profile]


def _run(ctx, C, enc, B, n_w=None):
    import torch
    n_w = C.info()["wires"] if n_w is None else n_w
    wa = DA.poisoned((n_w, B, n_lwe))      # every wire the run does not write stays poison
    wb = DA.poisoned((n_w, B))
    for w, (a, b) in enc.items():
        wa[w] = torch.from_numpy(a).cuda()
        wb[w] = torch.from_numpy(b).cuda()
    C.run_dev(ctx, B, wa, wb)
    ctx.sync()
    return wa.cpu().numpy(), wb.cpu().numpy(), ctx.last_kernels()


def _check_wires(C, W, ha, hb, what):
    """every wire, every instance, all 501 words"""
    assert len(W) == ha.shape[0] == hb.shape[0], what
    bad = [w for w in range(ha.shape[0]) if not (np.array_equal(ha[w], W[w][0]) and np.array_equal(hb[w], W[w][1]))]
    if bad:
        depth = DF.schedule(C)["depth"]
        first = [(w, "depth %d" % depth[w], C.node(w)) for w in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {len(W)} wires differ from the oracle; the first: {first}")


def _check_kernels(sched, B, kern, what, guard=True):
    for name in DF.expected_kernels(sched, B, _cus(), guard):
        assert any(k.startswith(name) for k in kern) if name.endswith("(") else name in kern, (what, name, kern)


# ---------------------------------------------------------------- the default guarded path

@pytest.mark.parametrize("B", DF.SMALL_B)
@pytest.mark.parametrize("seed", DF.SMALL_SEEDS)
def test_small(ctx, okey, seed, B):
    what = f"seed {seed} (small), B = {B}"
    C, ins, sched, enc, W = _case(okey, seed, "small", B)
    ha, hb, kern = _run(ctx, C, enc, B)
    _check_wires(C, W, ha, hb, what)
    _check_kernels(sched, B, kern, what)
    assert "k_keyswitch_small" in kern and "k_blind_rotate_v6_rows(lut-many+lds-rotation)" in kern, (what, kern)


@pytest.mark.parametrize("seed", DF.WIDE_SEEDS)
def test_wide(ctx, okey, seed):
    """one level of every row kind, rows x B just above one workgroup per CU: the register rotation,
    and the int8 MFMA key switch with a split"""
    B = _shape("wide")
    what = f"seed {seed} (wide), B = {B}"
    C, ins, sched, enc, W = _case(okey, seed, "wide", B)
    ha, hb, kern = _run(ctx, C, enc, B)
    _check_wires(C, W, ha, hb, what)
    _check_kernels(sched, B, kern, what)
    assert "k_blind_rotate_v6_rows(lut-many+reg-rotation)" in kern, (what, kern)
    assert any(k.startswith("k_keyswitch_v5(int8-mfma+split") for k in kern), (what, kern)


@pytest.mark.parametrize("seed", DF.SEAM_SEEDS)
def test_seam(ctx, okey, seed):
    """rows x B = 4 CUs + 3: the level takes two launches and the second (base > 0, 3 workgroups,
    LDS rotation) starts inside the instances of the level's last row — the second half of a MUX
    (odd seed) or a many-LUT row (even seed); a second level reads that row"""
    B = _shape("seam")
    what = f"seed {seed} (seam), B = {B}"
    C, ins, sched, enc, W = _case(okey, seed, "seam", B)
    assert sched["rows"][1] * B == 4 * _cus() + 3, what
    ha, hb, kern = _run(ctx, C, enc, B)
    _check_wires(C, W, ha, hb, what)
    _check_kernels(sched, B, kern, what)
    for name in ("k_blind_rotate_v6_rows(lut-many+reg-rotation)", "k_blind_rotate_v6_rows(lut-many+lds-rotation)"):
        assert name in kern, (what, kern)
    assert any(k.startswith("k_keyswitch_v5(") for k in kern), (what, kern)


# ---------------------------------------------------------------- the other modes, on the cached cases

def _guard_zero(ctx, okey, seed, profile, B):
    """threshold 0: every row — MUX halves and many-LUT rows with all their outputs — is rewritten by
    the exact rows kernel; the counter counts rows x instances"""
    what = f"seed {seed} ({profile}), B = {B}, guard threshold 0"
    C, ins, sched, enc, W = _case(okey, seed, profile, B)
    try:
        T.set_guard_threshold(0.0)
        ctx.guard_stats(reset=True)
        ha, hb, kern = _run(ctx, C, enc, B)
        _, recomputed = ctx.guard_stats(reset=True)
    finally:
        T.set_guard_threshold(0.125)
    _check_wires(C, W, ha, hb, what)
    assert recomputed == sched["bootstraps"] * B, (what, recomputed)
    assert "k_blind_rotate_v4_rows(lut-many+guard)" in kern, (what, kern)
    _check_kernels(sched, B, kern, what)


@pytest.mark.parametrize("seed", DF.SMALL_SEEDS[:2])
def test_guard_threshold_zero_small(ctx, okey, seed):
    _guard_zero(ctx, okey, seed, "small", 3)


def test_guard_threshold_zero_wide(ctx, okey):
    _guard_zero(ctx, okey, DF.WIDE_SEEDS[0], "wide", _shape("wide"))


@pytest.mark.parametrize("seed", DF.SMALL_SEEDS[4:6])
def test_exact_kernel_generation(ctx, okey, seed):
    what = f"seed {seed} (small), B = 3, select_kernel(4)"
    C, ins, sched, enc, W = _case(okey, seed, "small", 3)
    try:
        T.select_kernel(4)
        ha, hb, kern = _run(ctx, C, enc, 3)
    finally:
        T.select_kernel(0)
    _check_wires(C, W, ha, hb, what)
    assert "k_blind_rotate_v4_rows(lut-many)" in kern and not any("v6" in k for k in kern), (what, kern)


def test_multi_context_uneven_shard(okey, keyset):
    """two slots on one GPU, B = 5: shards of 3 and 2 instances, each with its own device state"""
    seed, B = DF.SMALL_SEEDS[3], 5
    what = f"seed {seed} (small), B = {B}, MultiContext"
    C, ins, sched, enc, W = _case(okey, seed, "small", B)
    wires = [w for w in range(sched["wires"]) if w not in ins]
    m = T.MultiContext(keyset.bk, keyset.ksk, [0, 0])
    try:
        out_a, out_b = m.circuit_host(C, B, ins, np.stack([enc[w][0] for w in ins]), np.stack([enc[w][1] for w in ins]),
                                      wires)
    finally:
        m.close()
    ha = np.zeros((sched["wires"], B, n_lwe), np.int32)
    hb = np.zeros((sched["wires"], B), np.int32)
    for w in ins:
        ha[w], hb[w] = enc[w]
    ha[wires], hb[wires] = out_a, out_b
    _check_wires(C, W, ha, hb, what)


def test_lifecycle_regrow_scratch_then_grow_the_circuit(ctx, okey):
    """one circuit object: B = 1, then B = 3 (the u scratch regrows), then three more nodes — a MUX,
    a many-LUT row and an affine node — and B = 3 again (the schedule and the device tables are
    rebuilt); all wires of all runs.  The circuit grows twice: once with info() between the growth
    and the run, so that info() compiles the new schedule and the run finds it compiled (this ran on
    the device tables of the old schedule and faulted: whichever call compiles now drops them), and
    once with the run itself compiling."""
    seed = DF.SMALL_SEEDS[2]
    C, ins, F = DF.make_case(seed, "small", _cus())         # its own object: the cached one stays as it is
    for B in DF.SMALL_B:
        _, _, sched, enc, W = _case(okey, seed, "small", B)
        ha, hb, kern = _run(ctx, C, enc, B)
        _check_wires(C, W, ha, hb, f"seed {seed} (small), B = {B}, lifecycle")
    assert C.state_count() == 1
    new = DF.grow(C, seed)
    assert C.info()["wires"] == sched["wires"] + len(new) and new[0] == sched["wires"], f"seed {seed}"
    assert C.state_count() == 0, f"seed {seed}: device tables of the schedule before the growth are still held"
    W2 = DO.eval_circuit(C, okey, enc, 3, known=W)
    assert len(W2) == len(W) + len(new)
    ha, hb, kern = _run(ctx, C, enc, 3)
    _check_wires(C, W2, ha, hb, f"seed {seed} (small), B = 3, lifecycle, grown by a MUX, a many-LUT row and an affine")
    assert C.state_count() == 1
    new = DF.grow(C, seed + 1)                              # no call that compiles before the run
    ha, hb, kern = _run(ctx, C, enc, 3, n_w=len(W2) + len(new))
    _check_wires(C, DO.eval_circuit(C, okey, enc, 3, known=W2), ha, hb, f"seed {seed} (small), B = 3, lifecycle, grown twice")
    assert C.state_count() == 1
    C.close()
