"""Select nodes of the circuit engine, host side: the argument rules, the compiler's
levelling and accounting against an independent count, the evaluator of tests/select_dag_oracle.py
pinned to tests/dag_oracle.py, and the lut2 builder decoded on the oracle.  No GPU.

(The refusal of a circuit with a select node by tfhe_amd_circuit_run_dev and the two
tfhe_amd_multi_circuit_run_* forms needs a context to tell it from the refusal of a null context,
so it is asserted in tests/test_circuit_select_gpu.py.)"""
import ctypes

import numpy as np
import pytest

import dag_fuzz as DF
import dag_oracle as DO
import select_dag_oracle as SO
import tfhe_amd as T

E_ARG = -1
E4 = 1 << 30


def _ids(v):
    return (ctypes.c_int * len(v))(*v)


def _select(C, p, cand, c0, s, sel):
    return T.lib.tfhe_amd_circuit_select(C.h, p, cand, c0, s, sel)


# ------------------------------------------------------------------ argument rules

@pytest.fixture
def circ():
    C = T.Circuit()
    C.inputs(4)
    yield C
    C.close()


@pytest.mark.parametrize("p", [0, 1, 3, 5, 6, 12, 17, 32, -2])
def test_p_outside_2_4_8_16_is_refused(circ, p):
    assert _select(circ, p, _ids([0] * 32), 0, 1, 1) == E_ARG
    assert circ.info()["wires"] == 4


@pytest.mark.parametrize("p", [2, 4, 8, 16])
def test_every_p_of_the_set_is_taken(circ, p):
    assert _select(circ, p, _ids([0] * p), 0, 1, 1) == 4


def test_null_candidates_are_refused(circ):
    assert _select(circ, 2, None, 0, 1, 1) == E_ARG


def test_null_circuit_is_refused():
    assert T.lib.tfhe_amd_circuit_select(None, 2, _ids([0, 1]), 0, 1, 1) == E_ARG


def test_candidate_not_yet_defined_is_refused(circ):
    assert _select(circ, 2, _ids([0, 4]), 0, 1, 1) == E_ARG      # wire 4 would be the node itself


def test_negative_candidate_is_refused(circ):
    assert _select(circ, 4, _ids([0, 1, -1, 2]), 0, 1, 1) == E_ARG


def test_selector_not_yet_defined_is_refused(circ):
    assert _select(circ, 2, _ids([0, 1]), 0, 1, 4) == E_ARG


def test_negative_selector_is_refused(circ):
    assert _select(circ, 2, _ids([0, 1]), 0, 1, -1) == E_ARG


def test_a_refused_node_adds_nothing(circ):
    for bad in ((3, [0, 1, 2]), (2, [0, 9])):
        assert _select(circ, bad[0], _ids(bad[1]), 0, 1, 1) == E_ARG
    assert circ.info()["wires"] == 4 and circ.select_count() == 0


def test_introspection(circ):
    w = circ.select([3, 0, 0, 2], 1, c0=-7, s=5)
    assert w == 4 and circ.select_count() == 1
    assert circ.node(w) == (1, SO.SELECT_GATE, -7, [5, 0, 0], [1, -1, -1])
    assert circ.select_node(w) == (4, [3, 0, 0, 2], -7)
    cand = (ctypes.c_int * 16)()
    assert T.lib.tfhe_amd_circuit_select_node(circ.h, w, None, cand, None) == 0
    assert list(cand) == [3, 0, 0, 2] + [-1] * 12


def test_select_node_refuses_other_nodes(circ):
    g = circ.gate("NAND", 0, 1)
    for w in (0, g, 99, -1):
        assert T.lib.tfhe_amd_circuit_select_node(circ.h, w, None, None, None) == E_ARG
    assert T.lib.tfhe_amd_circuit_select_node(None, 0, None, None, None) == E_ARG


def test_eval_plain_refuses_a_select_node(circ):
    circ.select([0, 1], 2)
    with pytest.raises(T.TfheAmdError, match="select"):
        circ.eval_plain({w: np.zeros(1) for w in range(4)})


def test_lut2_argument_rules(circ):
    v = np.zeros(16, np.int32)
    lib, p = T.lib, T._p
    assert lib.tfhe_amd_circuit_lut2(None, p(v), 0, 1) == E_ARG
    assert lib.tfhe_amd_circuit_lut2(circ.h, None, 0, 1) == E_ARG
    assert lib.tfhe_amd_circuit_lut2(circ.h, p(v), 4, 1) == E_ARG
    assert lib.tfhe_amd_circuit_lut2(circ.h, p(v), 0, -1) == E_ARG
    assert circ.info()["wires"] == 4
    with pytest.raises(T.TfheAmdError):
        circ.lut2(np.zeros(15, np.int32), 0, 1)


def test_run_with_pack_key_refuses_null_handles():
    assert T.lib.tfhe_amd_circuit_run_pk_dev(None, None, None, 1, None, None, None) == E_ARG


def test_lut2_lowers_to_a_many_lut_row_and_a_select_node(circ):
    rng = np.random.default_rng(5)
    values = rng.integers(-2**31, 2**31, 16, dtype=np.int64).astype(np.int32)
    w = circ.lut2(values, 2, 3)
    assert w == 8 and circ.info() == dict(wires=9, gates=2, bootstraps=2, depth=2)
    for f in range(4):
        t, c0, log_nu, n_out, index = circ.lut_many_node(4 + f)
        assert (c0, log_nu, n_out, index) == (0, 2, 4, f)
        assert circ.node(4 + f)[3:] == ([1, 0, 0], [2, -1, -1])
    assert np.array_equal(circ.lut_table_get(t), T.lut_table_many(4, values.reshape(4, 4), 2))
    assert circ.select_node(w) == (4, [4, 5, 6, 7], 0) and circ.node(w)[3:] == ([1, 0, 0], [3, -1, -1])


# ------------------------------------------------------------------ levels and counts

def levels(C):
    """An independent leveller over node() / lut_many_node() / select_node(), with the rules of
    dag_fuzz.schedule and one more: a select node sits one level above the deepest of its selector's
    source and its candidate WIRES as written (a bootstrap-free candidate has its source's depth, a
    constant one depth 0).  -> (depth [wire], rows [level] counting a select node as one row,
    bootstraps)"""
    n_w = DO.count_wires(C)
    src, scale, depth = [None] * n_w, [0] * n_w, [0] * n_w
    rows = [0]
    for w in range(n_w):
        kind, gate, c0, s, ins = C.node(w)
        if kind == 0:
            src[w], scale[w] = w, 1
            continue
        if kind == 2:
            if gate != DO.CONST:
                k = {DO.NOT: -1, DO.COPY: 1}.get(gate, s[0])
                scale[w] = (scale[ins[0]] * k) % 2**32
                src[w] = src[ins[0]] if scale[w] else None
            depth[w] = depth[src[w]] if src[w] is not None else 0
            continue
        src[w], scale[w] = w, 1
        if gate == DO.LUT_MANY_GATE and C.lut_many_node(w)[4]:
            depth[w] = depth[w - C.lut_many_node(w)[4]]
            continue
        below = [depth[src[i]] for i in ins if i >= 0 and src[i] is not None]
        if gate == SO.SELECT_GATE:
            below += [depth[c] for c in C.select_node(w)[1]]
        depth[w] = 1 + max(below, default=0)
        rows += [0] * (depth[w] + 1 - len(rows))
        rows[depth[w]] += 2 if gate == DO.MUX else 1
    return depth, rows, sum(rows)


def _chain(C, x, y, n):
    """n NAND levels on top of x"""
    for _ in range(n):
        x = C.gate("NAND", x, y)
    return x


def test_level_candidates_two_levels_above_the_selector():
    C = T.Circuit()
    a, b, c = C.inputs(3)
    sel = C.gate("AND", a, b)                              # level 1
    deep = _chain(C, sel, c, 2)                            # level 3
    w = C.select([deep, C.gate("NOT", deep)], sel, c0=E4)  # candidates at 3, selector at 1 -> level 4
    after = C.gate("OR", w, a)                             # level 5
    depth, rows, boots = levels(C)
    assert depth[w] == 4 and depth[after] == 5
    assert C.level_sizes() == rows == [0, 1, 1, 1, 1, 1]
    assert C.info() == dict(wires=9, gates=6, bootstraps=boots, depth=5)
    C.close()


def test_level_selector_two_levels_above_the_candidates():
    C = T.Circuit()
    a, b, c = C.inputs(3)
    low = C.gate("AND", a, b)                              # level 1
    sel = _chain(C, low, c, 2)                             # level 3
    w = C.select([low, a, C.gate("CONST", 1), C.affine(5, 3, low)], C.gate("NOT", sel))   # -> level 4
    depth, rows, boots = levels(C)
    assert depth[w] == 4
    assert C.level_sizes() == rows == [0, 1, 1, 1, 1]
    assert C.info()["bootstraps"] == boots == 4
    C.close()


def test_level_of_a_select_over_inputs_and_constants_is_one():
    C = T.Circuit()
    a, b = C.inputs(2)
    k = C.gate("CONST", 0)
    w = C.select([a, k], C.affine(7, 0, b))                # the selector folds to a constant
    assert levels(C)[0][w] == 1 and C.level_sizes() == [0, 1]
    C.close()


def test_info_and_level_sizes_of_a_mixed_circuit():
    C, ins, sels, _ = SO.mixed_circuit()
    depth, rows, boots = levels(C)
    # gates 2 + MUX 2 + LUT 1 + many-LUT 1 + select 3 | select 2 + gate 1 + LUT 1
    assert rows == [0, 9, 4] and boots == 13
    assert C.level_sizes() == rows
    info = C.info()
    assert info["bootstraps"] == boots and info["depth"] == 2 and info["wires"] == DO.count_wires(C)
    assert [depth[w] for w in sels] == [1, 1, 1, 2, 2] and C.select_count() == 5
    assert DF.schedule(C)["wires"] == info["wires"]
    C.close()


# ------------------------------------------------------------------ the evaluator

def test_select_free_circuit_equals_dag_oracle_word_for_word(okey):
    """every wire of a fuzz circuit (gate rows, MUX, LUT, many-LUT, adder cells, bootstrap-free nodes)"""
    seed, B = DF.SMALL_SEEDS[0], 1
    C, ins, _ = DF.make_case(seed, "small")
    enc = DF.random_inputs(seed, ins, B)
    want = DO.eval_circuit(C, okey, enc, B)
    got = SO.eval_circuit(C, okey, enc, B)
    assert sorted(got) == sorted(want) == list(range(C.info()["wires"]))
    for w in want:
        assert np.array_equal(got[w][0], want[w][0]) and np.array_equal(got[w][1], want[w][1]), w
    C.close()


def test_select_node_of_the_evaluator_is_the_batch_oracle(okey, keyset):
    """one select node over inputs: the evaluator's wire equals acc_oracle.select on the same words; and
    it asks for the packing key"""
    import acc_oracle as AO
    rng = np.random.default_rng(12)
    r32 = lambda shape: rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)
    key = r32((500, 6, 2, 1024))
    B = 2
    C = T.Circuit()
    ins = C.inputs(5)
    w = C.select(ins[:4], ins[4], c0=-9, s=3)
    enc = {i: (r32((B, 500)), r32(B)) for i in ins}
    got = SO.eval_circuit(C, okey, enc, B, pack_key=key)[w]
    want = AO.select(okey, key, np.stack([enc[i][0] for i in ins[:4]]), np.stack([enc[i][1] for i in ins[:4]]), -9, 3,
                     *enc[ins[4]])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(AssertionError, match="packing key"):
        SO.eval_circuit(C, okey, enc, B)
    C.close()


def test_lut2_decodes_on_the_oracle(keyset, okey):
    """Two fresh p = 4 digits x, y at the key-switch noise, B = 32, a random 4-bit -> 2-bit table, data
    seed 3909 (SO.lut2_case; the packing key is acc_oracle.chain_pack_key's, generator seed 2025, 38);
    the first seed tried, none was discarded.  The four many-LUT outputs decode to values[4 j + x], the
    select output to values[4 y + x], for every one of the 32 samples.  Prints the deviations from the
    box centres that DESIGN.md §3.9 quotes (margin 1/16 = 0.0625).
    Measured on the oracle: candidates largest 0.0108, r.m.s. 0.0040; output largest 0.0147, r.m.s. 0.0072."""
    c = SO.lut2_case(keyset, okey)
    f, x, y, W = c["f"], c["x"], c["y"], c["W"]

    def deviation(wire, m):
        ph = keyset.phase(*W[wire]).astype(np.int64)
        d = ((ph - T.lut_encode(m, 4).astype(np.int64) + 2**31) % 2**32 - 2**31).astype(np.float64) / 2**32
        return np.abs(d)
    cand = np.concatenate([deviation(c["many"] + j, f[j, x]) for j in range(4)])
    out = deviation(c["out"], f[y, x])
    print(f"lut2 B = {c['B']}: candidates largest {cand.max():.4f} r.m.s. {np.sqrt(np.mean(cand**2)):.4f}; "
          f"output largest {out.max():.4f} r.m.s. {np.sqrt(np.mean(out**2)):.4f}; margin {1 / 16:.4f}")
    for j in range(4):
        assert np.array_equal(T.lut_decode(keyset.phase(*W[c["many"] + j]), 4), f[j, x]), j
    assert np.array_equal(T.lut_decode(keyset.phase(*W[c["out"]]), 4), f[y, x])
