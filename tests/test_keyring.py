"""Key ring, host side (no GPU): tfhe_amd_keyring_plan, the order a mixed-key batch is worked in,
against a numpy stable argsort, and the argument checks of tfhe_amd_keyring_create that need no
device."""
import ctypes

import numpy as np
import pytest

import tfhe_amd as T

ROWS = {"MUX": 2, "NOT": 0, "COPY": 0}   # blind rotations per gate; every binary gate: 1
BINARY = ["NAND", "OR", "AND", "XOR", "XNOR", "NOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]


def _want(n_keys, key_of, gates):
    key_of = np.asarray(key_of, dtype=np.int64)
    order = np.argsort(key_of, kind="stable")
    offsets = np.searchsorted(key_of[order], np.arange(n_keys + 1), side="left")
    rows = len(key_of) if gates is None else sum(ROWS.get(g, 1) for g in gates)
    return order, offsets, rows


def _check(n_keys, key_of, gates):
    order, offsets, rows = T.KeyRing.plan_of(n_keys, key_of, gates)
    w_order, w_offsets, w_rows = _want(n_keys, key_of, gates)
    assert np.array_equal(order, w_order), (n_keys, key_of, order, w_order)
    assert np.array_equal(offsets, w_offsets), (n_keys, key_of, offsets, w_offsets)
    assert rows == w_rows, (gates, rows, w_rows)


def test_plan_issue_batch():
    """the batch of the GPU parity test: three slots out of order, a MUX and a NOT among the gates"""
    _check(3, [2, 0, 1, 0, 2, 1, 0], ["NAND", "MUX", "NOT", "AND", "MUX", "OR", "XOR"])


def test_plan_empty_groups():
    _check(5, [4, 1, 4, 1, 1], ["NAND"] * 5)            # slots 0, 2, 3 empty (first, middle)
    _check(4, [0, 0, 2], ["OR", "MUX", "XOR"])          # an empty middle group and an empty last one
    order, offsets, rows = T.KeyRing.plan_of(4, [0, 0, 2], ["OR", "MUX", "XOR"])
    assert list(offsets) == [0, 2, 2, 3, 3] and rows == 4


def test_plan_one_key_and_single():
    _check(1, [0] * 9, ["XNOR"] * 9)
    _check(3, [1] * 6, BINARY[:6])                       # all one key of a larger ring
    _check(1, [0], ["MUX"])                              # B = 1
    _check(256, [255], ["NAND"])
    _check(2, [], [])                                    # B = 0


def test_plan_mux_counts_two_rows_and_linear_none():
    gates = ["MUX", "NAND", "MUX", "NOT", "COPY", "MUX"]
    order, offsets, rows = T.KeyRing.plan_of(2, [1, 0, 1, 0, 1, 0], gates)
    assert rows == 3 * 2 + 1 and list(offsets) == [0, 3, 6] and list(order) == [1, 3, 5, 0, 2, 4]
    # the LUT form passes no gates: one row per ciphertext
    _check(3, [2, 2, 0, 1], None)


def test_plan_random_against_stable_argsort():
    rng = np.random.default_rng(20261021)
    kinds = BINARY + ["MUX", "NOT", "COPY"]
    for _ in range(50):
        n_keys = int(rng.integers(1, 257))
        B = int(rng.integers(0, 400))
        key_of = rng.integers(0, n_keys, B)
        _check(n_keys, key_of, [kinds[i] for i in rng.integers(0, len(kinds), B)])


@pytest.mark.parametrize("key_of", [[3], [0, -1], [0, 1, 2, 3]])
def test_plan_refuses_a_slot_out_of_range(key_of):
    with pytest.raises(T.TfheAmdError):
        T.KeyRing.plan_of(3, key_of, ["NAND"] * len(key_of))


@pytest.mark.parametrize("code", [-1, 16, 99, T.GATES["MAJ"], T.GATES["XOR3"], T.GATES["CONST"]])
def test_plan_refuses_a_bad_gate_code(code):
    """codes outside the enum, and the circuit-only kinds the batch forms have no inputs for"""
    with pytest.raises(T.TfheAmdError):
        T.KeyRing.plan_of(2, [0, 1], [T.GATES["NAND"], code])


def test_plan_refuses_bad_sizes_and_writes_nothing():
    IP = ctypes.POINTER(ctypes.c_int)
    key_of = np.array([0, 5, 1], np.int32)
    order = np.full(3, -7, np.int32); offsets = np.full(4, -7, np.int32); rows = ctypes.c_int(-7)
    args = (key_of.ctypes.data_as(IP), None, order.ctypes.data_as(IP), offsets.ctypes.data_as(IP), ctypes.byref(rows))
    assert T.lib.tfhe_amd_keyring_plan(3, 3, *args) == -1          # slot 5 of 3
    assert (order == -7).all() and (offsets == -7).all() and rows.value == -7
    assert T.lib.tfhe_amd_keyring_plan(3, 0, *args) == -1
    assert T.lib.tfhe_amd_keyring_plan(3, 257, *args) == -1
    assert T.lib.tfhe_amd_keyring_plan(-1, 3, *args) == -1
    # every output is optional
    assert T.lib.tfhe_amd_keyring_plan(3, 6, key_of.ctypes.data_as(IP), None, None, None, None) == 0


def test_create_refuses_null_and_bad_counts():
    VP = ctypes.c_void_p
    out = VP(0xdead)
    assert T.lib.tfhe_amd_keyring_create(None, 1, ctypes.byref(out)) == -1 and not out.value
    one = (VP * 1)(None)
    assert T.lib.tfhe_amd_keyring_create(one, 1, ctypes.byref(out)) == -1          # a null member
    assert T.lib.tfhe_amd_keyring_create(one, 0, ctypes.byref(out)) == -1
    many = (VP * 257)()
    assert T.lib.tfhe_amd_keyring_create(many, 257, ctypes.byref(out)) == -1
    assert T.lib.tfhe_amd_keyring_create(one, 1, None) == -1
    assert T.lib.tfhe_amd_keyring_count(None) == -1 and T.lib.tfhe_amd_keyring_device(None) == -1
    assert T.lib.tfhe_amd_keyring_destroy(None) == 0
    with pytest.raises(T.TfheAmdError):
        T.KeyRing([])
