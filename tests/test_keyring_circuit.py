"""Mixed-key circuits, host side (no GPU): tfhe_amd_keyring_circuit_plan — the order of the instances
and the key-switch tiles of a level — against a numpy restatement, the properties every plan has, the
refusals that need no device, and the new symbols' export and declaration."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tfhe_amd as T

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "tfhe_amd.h")
NEW = ["tfhe_amd_keyring_circuit_plan", "tfhe_amd_keyring_circuit_tile", "tfhe_amd_keyring_circuit_run_dev",
       "tfhe_amd_keyring_circuit_run_host"]
IP = ctypes.POINTER(ctypes.c_int)


def _want(n_keys, key_of, nks, tile):
    key_of = np.asarray(key_of, dtype=np.int64)
    order = np.argsort(key_of, kind="stable")
    offsets = np.searchsorted(key_of[order], np.arange(n_keys + 1), side="left")
    tiles = []
    for g in range(n_keys):
        lanes, base = nks * int(offsets[g + 1] - offsets[g]), nks * int(offsets[g])
        tiles += [(g, base + l0, min(tile, lanes - l0)) for l0 in range(0, lanes, tile)]
    return order, offsets, np.array(tiles, np.int64).reshape(-1, 3)


def _check(n_keys, key_of, nks, tile):
    key_of = np.asarray(key_of, dtype=np.int64)
    B = len(key_of)
    order, offsets, tiles = T.KeyRing.circuit_plan_of(n_keys, key_of, nks, tile)
    w_order, w_offsets, w_tiles = _want(n_keys, key_of, nks, tile)
    what = (n_keys, list(key_of), nks, tile)
    assert np.array_equal(order, w_order), what
    assert np.array_equal(offsets, w_offsets), what
    assert np.array_equal(tiles, w_tiles), (what, tiles, w_tiles)
    # the order inside a group is stable
    for g in range(n_keys):
        grp = order[offsets[g]:offsets[g + 1]]
        assert (key_of[grp] == g).all() and (np.diff(grp) > 0).all(), (what, g)
    # no tile spans two groups, every tile has 1 .. tile live lanes
    seen = np.zeros((nks, B), np.int64)
    for g, first, live in tiles:
        assert 1 <= live <= tile, what
        assert nks * offsets[g] <= first and first + live <= nks * offsets[g + 1], (what, g, first, live)
        # every (output, instance) lane exactly once, decoded as the kernel's lane map does
        n_g = int(offsets[g + 1] - offsets[g])
        q = np.arange(first, first + live) - nks * int(offsets[g])
        np.add.at(seen, (q // n_g, order[offsets[g] + q % n_g]), 1)
    assert (seen == 1).all(), what
    return tiles


def test_plan_issue_batch():
    tiles = _check(3, [2, 0, 1, 0, 2, 1, 0], 5, 256)
    assert [tuple(t) for t in tiles] == [(0, 0, 15), (1, 15, 10), (2, 25, 10)]


def test_plan_empty_groups_one_key_and_singles():
    _check(5, [4, 1, 4, 1, 1], 3, 4)                 # slots 0, 2, 3 empty (first, middle)
    tiles = _check(4, [0, 0, 2], 2, 256)             # an empty middle group and an empty last one
    assert [int(t[0]) for t in tiles] == [0, 2]
    _check(1, [0] * 9, 7, 8)                         # one key
    _check(3, [1] * 6, 2, 5)                         # all one key of a larger ring
    _check(1, [0], 4, 256)                           # B = 1
    _check(3, [2, 0, 1, 1], 1, 2)                    # nks = 1
    _check(256, [255], 1, 256)
    _check(2, [], 3, 256)                            # B = 0: no tile
    _check(2, [0, 1, 1], 0, 256)                     # a level that key-switches nothing: no tile


def test_plan_a_group_of_exactly_one_tile_and_of_one_tile_plus_one_lane():
    tile = T.KeyRing.circuit_tile()
    assert tile >= 8 and tile % 8 == 0      # the engine's M-tile (256 lanes today)
    nks = 8
    n0, n1 = tile // nks, tile // nks + 1            # one tile of lanes, and one tile + one instance's 8 lanes
    tiles = _check(2, [0] * n0 + [1] * n1, nks, tile)
    assert [tuple(t) for t in tiles] == [(0, 0, tile), (1, tile, tile), (1, 2 * tile, nks)]
    tiles = _check(2, [1] * (tile + 1) + [0] * tile, 1, tile)
    assert [tuple(t) for t in tiles] == [(0, 0, tile), (1, tile, tile), (1, 2 * tile, 1)]
    tiles = _check(2, [0, 1] * 3 + [1], 1, 3)         # the same at a tile of 3 lanes
    assert [tuple(t) for t in tiles] == [(0, 0, 3), (1, 3, 3), (1, 6, 1)]


def test_plan_random_against_the_restatement():
    rng = np.random.default_rng(20261021)
    for _ in range(50):
        n_keys = int(rng.integers(1, 40)) if rng.integers(0, 4) else int(rng.integers(1, 257))
        B = int(rng.integers(0, 300))
        _check(n_keys, rng.integers(0, n_keys, B), int(rng.integers(0, 9)), int(rng.choice([1, 3, 32, 256])))


@pytest.mark.parametrize("key_of", [[3], [0, -1], [0, 1, 2, 3]])
def test_plan_refuses_a_slot_out_of_range(key_of):
    with pytest.raises(T.TfheAmdError):
        T.KeyRing.circuit_plan_of(3, key_of, 2)


def test_plan_refuses_bad_sizes_and_writes_nothing():
    key_of = np.array([0, 5, 1], np.int32)
    order = np.full(3, -7, np.int32); offsets = np.full(4, -7, np.int32); tiles = np.full(30, -7, np.int32)
    nt = ctypes.c_int(-7)
    p = lambda a: a.ctypes.data_as(IP)
    plan = T.lib.tfhe_amd_keyring_circuit_plan
    out = (p(order), p(offsets), p(tiles), 10, ctypes.byref(nt))
    assert plan(3, 3, p(key_of), 2, 256, *out) == -1            # slot 5 of 3
    assert plan(3, 0, p(key_of), 2, 256, *out) == -1
    assert plan(3, 257, p(key_of), 2, 256, *out) == -1
    assert plan(-1, 6, p(key_of), 2, 256, *out) == -1
    assert plan(3, 6, p(key_of), -1, 256, *out) == -1
    assert plan(3, 6, p(key_of), 2, 0, *out) == -1
    assert plan(3, 6, None, 2, 256, *out) == -1
    assert plan(3, 6, p(key_of), 1 << 30, 256, *out) == -1      # nks B above 2^30 - 1
    assert (order == -7).all() and (offsets == -7).all() and nt.value == -7
    # more tiles than the caller has room for
    assert plan(3, 6, p(key_of), 2, 1, p(order), p(offsets), p(tiles), 5, ctypes.byref(nt)) == -1
    # every output is optional; tiles == NULL counts
    assert plan(3, 6, p(key_of), 2, 256, None, None, None, 0, None) == 0
    assert plan(3, 6, p(key_of), 2, 1, None, None, None, 0, ctypes.byref(nt)) == 0 and nt.value == 6


def test_run_refuses_null_handles_without_a_device():
    k = np.zeros(2, np.int32)
    one = np.zeros(1, np.int32)
    i32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    circ = T.Circuit()
    try:
        x = circ.inputs(2)
        circ.gate("NAND", x[0], x[1])
        dev = T.lib.tfhe_amd_keyring_circuit_run_dev
        assert dev(None, circ.h, 2, k.ctypes.data_as(IP), 1, 1, None) == -1       # no ring
        assert dev(None, circ.h, 0, k.ctypes.data_as(IP), None, None, None) == -1
        assert dev(None, None, 2, None, None, None, None) == -1
        host = T.lib.tfhe_amd_keyring_circuit_run_host
        w = (ctypes.c_int * 1)(0)
        assert host(None, circ.h, 1, k.ctypes.data_as(IP), 1, w, i32p(one), i32p(one), 1, w, i32p(one), i32p(one)) == -1
        assert host(None, None, 0, None, 0, None, None, None, 0, None, None, None) == -1
    finally:
        circ.close()


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\bint\s+(tfhe_amd_keyring_circuit_\w+)\s*\(", src))


def test_new_symbols_are_exported_and_declared():
    out = subprocess.check_output(["nm", "-D", "--defined-only", T.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported, sorted(set(NEW) - exported)
    assert _declared() == set(NEW), sorted(_declared() ^ set(NEW))
    # and nothing of the runner's internals leaks into the C ABI's namespace by accident
    leaked = {s for s in exported if s.startswith("tfhe_amd_keyring_circuit_")} - set(NEW)
    assert not leaked, sorted(leaked)
