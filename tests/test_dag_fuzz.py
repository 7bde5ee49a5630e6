"""The fuzz generator of tests/dag_fuzz.py and the compiler's schedule, without a GPU: seeds are
reproducible, the fixed seed list covers every corner the fuzz is for, and for every case the
compiler's level sizes, bootstrap count and wire count equal what an independent leveller computes
from the node list."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import dag_fuzz as DF
import dag_oracle as DO
import tfhe_amd as T

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASES = [(s, "small") for s in DF.SMALL_SEEDS] + [(s, "wide") for s in DF.WIDE_SEEDS] + \
        [(s, "seam") for s in DF.SEAM_SEEDS]


def _node_list(C):
    out = []
    for w in range(DO.count_wires(C)):
        node = C.node(w)
        extra = ()
        if node[1] == DF.LUT_GATE:
            extra = C.lut_node(w)
        elif node[1] == DF.LUT_MANY_GATE:
            extra = C.lut_many_node(w)
        out.append((node, extra))
    return out


def _digest(seed, profile):
    C, ins, F = DF.make_case(seed, profile)
    h = hashlib.sha256(repr((_node_list(C), ins, sorted(F))).encode())
    t = 0
    while True:
        try:
            h.update(C.lut_table_get(t).tobytes())
        except T.TfheAmdError:
            break
        t += 1
    return h.hexdigest()


@pytest.mark.parametrize("seed,profile", CASES)
def test_same_seed_same_circuit(seed, profile):
    assert _digest(seed, profile) == _digest(seed, profile), f"seed {seed} ({profile})"
    other = _digest(seed + 1000, profile)
    assert other != _digest(seed, profile), f"seed {seed} ({profile}): another seed gave the same circuit"


def test_same_seed_same_circuit_in_another_process():
    """nothing in the generator depends on the process (string hashing, dict order of sets)"""
    seed = DF.SMALL_SEEDS[0]
    code = "import sys; sys.path[:0] = [%r, %r]; import test_dag_fuzz as t; print(t._digest(%d, 'small'))" % (
        os.path.join(REPO, "cpu-gpu-tfhe_amd"), HERE, seed)
    env = dict(os.environ, PYTHONHASHSEED="12345")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[-1] == _digest(seed, "small"), f"seed {seed}"


def test_seed_list_covers_every_feature():
    union, per_seed = set(), {}
    for seed, profile in CASES:
        per_seed[(seed, profile)] = DF.make_case(seed, profile)[2]
        union |= per_seed[(seed, profile)]
    assert union == set(DF.FEATURES), (sorted(set(DF.FEATURES) - union), sorted(union - set(DF.FEATURES)))
    assert len(DF.FEATURES) == 22
    # every MUX-beside-a-table-row mix is also in the one-level profiles, where a launch holds them all
    for key in [(s, "wide") for s in DF.WIDE_SEEDS] + [(s, "seam") for s in DF.SEAM_SEEDS]:
        assert {"mux+lut-row", "mux+many-row", "mux+full-add", "two-log-nu+gate-row", "many(1,2)", "many(2,3)",
                "many(4,16)"} <= per_seed[key], key


@pytest.mark.parametrize("seed,profile", CASES)
def test_compiler_schedule_equals_the_independent_leveller(seed, profile):
    C, ins, F = DF.make_case(seed, profile)
    s = DF.schedule(C)
    info = C.info()
    assert C.level_sizes() == s["rows"], f"seed {seed} ({profile})"
    assert info["bootstraps"] == s["bootstraps"], f"seed {seed} ({profile})"
    assert info["wires"] == s["wires"], f"seed {seed} ({profile})"
    assert info["depth"] == len(s["rows"]) - 1, f"seed {seed} ({profile})"


@pytest.mark.parametrize("seed", DF.SMALL_SEEDS)
def test_small_profile_sizes(seed):
    """about 12 inputs, 30 to 40 bootstraps, depth 4 to 6; at B = 1 and B = 3 some level's key
    switches number <= 4 and some 5 .. 12 (the two small kernels)"""
    C, ins, F = DF.make_case(seed, "small")
    s = DF.schedule(C)
    assert 11 <= len(ins) <= 13, f"seed {seed}"
    assert 30 <= s["bootstraps"] <= 40, f"seed {seed}: {s['bootstraps']}"
    assert 4 <= len(s["rows"]) - 1 <= 6, f"seed {seed}"
    for B in DF.SMALL_B:
        counts = [k * B for k in s["ks"][1:]]
        assert any(k <= 4 for k in counts) and any(5 <= k <= 12 for k in counts), f"seed {seed}, B = {B}: {counts}"


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_wide_and_seam_shapes(cus):
    for seed in DF.WIDE_SEEDS:
        C, ins, F = DF.make_case(seed, "wide", cus)
        s = DF.schedule(C)
        B = DF.wide_B(cus)
        assert s["rows"] == [0, 13], f"seed {seed}"
        assert cus < 13 * B <= cus + 13 and s["ks"][1] * B > 12, f"seed {seed}"
        assert DF.expected_kernels(s, B, cus) == {"k_blind_rotate_v6_rows(lut-many+reg-rotation)",
                                                  "k_blind_rotate_v4_rows(lut-many+guard)", "k_keyswitch_v5("}, f"seed {seed}"
    R, B = DF.seam_shape(cus)
    assert R * B == 4 * cus + 3
    for seed in DF.SEAM_SEEDS:
        C, ins, F = DF.make_case(seed, "seam", cus)
        s = DF.schedule(C)
        assert s["rows"][1] == R and len(s["rows"]) == 3 and 0 < s["rows"][2] <= 4, f"seed {seed}"
        # the last row of level 1 (its instances hold slot 4 CUs, where the second launch starts):
        # the second half of a MUX for odd seeds, a many-LUT row for even ones; level 2 reads it
        last = max(w for w in range(s["wires"]) if s["depth"][w] == 1 and C.node(w)[0] == 1 and
                   (C.node(w)[1] != DF.LUT_MANY_GATE or C.lut_many_node(w)[4] == 0))
        assert C.node(last)[1] == (DF.MUX if seed % 2 else DF.LUT_MANY_GATE), f"seed {seed}"
        assert (R - 1) * B <= 4 * cus < R * B
        assert {"k_blind_rotate_v6_rows(lut-many+reg-rotation)", "k_blind_rotate_v6_rows(lut-many+lds-rotation)",
                "k_keyswitch_v5("} <= DF.expected_kernels(s, B, cus), f"seed {seed}"
        assert any(last in C.node(w)[4] for w in range(s["wires"]) if s["depth"][w] == 2), f"seed {seed}"


def test_compile_errors_through_the_public_calls():
    """a level of more than 65535 u rows (rows plus further many-LUT outputs) is refused by every
    call that compiles, one of exactly 65535 is not; a node that reads a wire not yet defined
    (SSA order) is refused where it is added"""
    C = T.Circuit()
    a, b = C.inputs(2)
    t = C.lut_table(np.zeros(DF.N, np.int32))
    for _ in range(4095):
        C.lut_many(t, 4, 16, 0, 1, a, 1, b)            # 16 u rows each
    for _ in range(15):
        C.gate("AND", a, b)
    assert C.level_sizes() == [0, 4095 + 15] and C.info()["bootstraps"] == 4110     # 65535 u rows
    C.gate("AND", a, b)
    with pytest.raises(T.TfheAmdError):
        C.info()
    with pytest.raises(T.TfheAmdError):
        C.level_sizes()
    C.close()
    C = T.Circuit()
    a, b = C.inputs(2)
    t = C.lut_table(np.zeros(DF.N, np.int32))
    for bad in (2, 3, 100):                            # wire 2 is the node being added
        for call in (lambda: C.gate("AND", a, bad), lambda: C.gate("MUX", bad, a, b), lambda: C.gate("NOT", bad),
                     lambda: C.lincomb(0, 1, a, 1, b, 1, bad), lambda: C.lut(t, 0, 1, bad),
                     lambda: C.lut_many(t, 1, 2, 0, 1, a, 1, bad), lambda: C.affine(0, 1, bad),
                     lambda: C.full_add(a, b, bad)):
            with pytest.raises(T.TfheAmdError):
                call()
    assert DO.count_wires(C) == 2 and C.info()["wires"] == 2
    C.close()
