"""The program generator of tests/seq_fuzz.py and its feature analysis, without a GPU: the program of a
seed is reproducible, the committed seed list covers the named feature list item by item, programs
are well formed (chains, thresholds, placement), and features_of sees what hand-written programs
contain and does not see what they lack."""
import hashlib
import os
import subprocess
import sys

import pytest

import seq_fuzz as SF

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _digest(seed, start_kernel=0):
    return hashlib.sha256(repr(SF.make_program(seed, start_kernel)).encode()).hexdigest()


@pytest.mark.parametrize("seed", SF.SEEDS)
def test_same_seed_same_program(seed):
    assert _digest(seed) == _digest(seed), f"seed {seed}"
    assert _digest(seed + 1000) != _digest(seed), f"seed {seed}: another seed gave the same program"
    a, b = SF.make_program(seed, 0), SF.make_program(seed, 4)
    assert a["steps"] == b["steps"] and (a["start_kernel"], b["start_kernel"]) == (0, 4), f"seed {seed}"


def test_same_seed_same_program_in_another_process():
    """nothing in the generator depends on the process (string hashing, dict order of sets)"""
    seed = SF.SEEDS[0]
    code = "import sys; sys.path[:0] = [%r, %r]; import test_seq_fuzz as t; print(t._digest(%d))" % (
        os.path.join(REPO, "cpu-gpu-tfhe_amd"), HERE, seed)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONHASHSEED="12345"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[-1] == _digest(seed), f"seed {seed}"


PER_SEED = {seed: SF.features_of(SF.make_program(seed)) for seed in SF.SEEDS}


@pytest.mark.parametrize("feature", SF.FEATURES)
def test_seed_list_covers(feature):
    assert any(feature in f for f in PER_SEED.values()), f"no seed of {SF.SEEDS} has {feature!r}"


def test_feature_list_is_the_named_one():
    assert len(SF.CALL_KINDS) == 26 and len(SF.FEATURES) == 26 + 5 + 5 + 4 + 10 == len(set(SF.FEATURES))
    union = set().union(*PER_SEED.values())
    assert union == set(SF.FEATURES), (sorted(set(SF.FEATURES) - union), sorted(union - set(SF.FEATURES)))
    assert set(SF.SKEW_SEEDS) <= set(SF.SEEDS) and len(SF.SKEW_SEEDS) == 2 and 5 <= len(SF.SEEDS) <= 8
    # what the skewed runs and the exact-kernel runs are for is in them as well
    for seed in SF.SKEW_SEEDS:
        assert {"chain:same-stream", "chain:cross-stream"} & PER_SEED[seed], seed


@pytest.mark.parametrize("seed", SF.SEEDS + [1, 2, 3, 4, 5, 6, 7, 8])
def test_programs_are_well_formed(seed):
    p = SF.make_program(seed)
    steps = p["steps"]
    assert SF.STEPS <= len(steps) <= SF.STEPS + 4, f"seed {seed}: {len(steps)} steps"
    assert sum(1 for s in steps if s["step"] == "call" and isinstance(s["B"], str)) <= 2, f"seed {seed}: thresholds"
    for i, s in enumerate(steps):
        if s["step"] == "state":
            assert s["op"] in SF.STATE_OPS, (seed, i, s)
            assert s["op"] != "reimport" or s["obj"] in SF.OBJECTS, (seed, i, s)
            continue
        kind = SF._K[s["kind"]]
        assert s["ctx"] in ("A", "B") and s["stream"] in (0, 1, 2, 3), (seed, i, s)
        assert not kind["host"] or s["stream"] == 0, (seed, i, s)              # the host forms take no stream
        if isinstance(s["B"], str):
            assert s["B"] in ("rot", "ks") and s["kind"] in SF.ROWWISE and s["chain"] is None, (seed, i, s)
        else:
            assert 1 <= s["B"] <= 5, (seed, i, s)
        if s["chain"] is not None:
            src, mode = s["chain"]
            q = steps[src]
            assert src < i and q["step"] == "call" and not isinstance(q["B"], str), (seed, i, s)
            assert SF._K[q["kind"]]["cout"] == kind["cin"] is not None, (seed, i, s)
            assert (SF.stream_key(q) == SF.stream_key(s)) == (mode == "same"), (seed, i, s)
            if kind["cin"] == "tlwe" and s["kind"].startswith("acc"):
                assert s["P"]["n_acc"] == q["B"], (seed, i, s)
            else:
                assert s["B"] == q["B"], (seed, i, s)
            # no synchronising step of the program lies between a same-stream chain's two ends
            if mode == "same":
                assert all(t["step"] == "call" or t["op"] not in ("guard_stats", "ctx_cycle", "reimport")
                           for t in steps[src + 1:i]), (seed, i, s)
    assert "tfhe_amd_blind_rotate_dev" not in repr(p) and "blind_rotate" not in SF.CALL_KINDS


def _call(kind, B=2, ctx="A", stream=1, chain=None, **P):
    g = SF._Gen(0)
    params = g.params(kind)
    params.update(P)
    return {"step": "call", "kind": kind, "B": B, "ctx": ctx, "stream": stream, "P": params, "chain": chain}


def _state(op, **kw):
    return dict({"step": "state", "op": op}, **kw)


def _features(steps):
    return SF.features_of({"seed": 0, "start_kernel": 0, "steps": steps})


def test_features_of_two_streams_and_what_breaks_it():
    two = [_call("gate", stream=1), _call("bootstrap", stream=2)]
    assert "two-streams:context" in _features(two)
    assert "two-streams:context" not in _features([two[0], _state("guard_stats", ctx="A"), two[1]])       # a device sync
    assert "two-streams:context" not in _features([two[0], _call("bootstrap", stream=1)])                  # one stream
    assert "two-streams:context" not in _features([two[0], _call("bootstrap", ctx="B", stream=2)])         # two contexts
    assert "two-streams:context" not in _features([two[0], _call("keyswitch", stream=2)])                  # no context fence
    # ctx.sync() waits for the context's own stream only
    own = [_call("gate", stream=0), _state("sync", ctx="A"), _call("gate", stream=2)]
    assert "two-streams:context" not in _features(own)
    assert "two-streams:context" in _features([_call("gate", stream=3), _state("sync", ctx="A"), _call("gate", stream=2)])


def test_features_of_regrowth():
    grow = [_call("gate", ctx="B", stream=1), _call("gate", B="rot", ctx="B", stream=2)]
    assert {"regrow:context", "threshold:rot"} <= _features(grow)
    assert "regrow:context" not in _features([_call("gate", ctx="A", stream=1), _call("gate", B="rot", ctx="A", stream=2)])
    assert "regrow:context" not in _features([grow[0], _state("guard_stats", ctx="B"), grow[1]])
    assert "regrow:context" not in _features([_call("gate", ctx="B", stream=2), grow[1]])                  # its own stream
    assert "regrow:context" in _features([grow[0], _state("reserve", ctx="B", B=100)])
    assert "regrow:context" not in _features([grow[0], _state("reserve", ctx="B", B=16)])
    # growth synchronises the device: the call that grew is not "back to back" with the one before it
    assert "two-streams:context" not in _features(grow)
    assert "two-streams:context" in _features(grow + [_call("gate", ctx="B", stream=3)])
    for owner, a, b in (("pack", _call("select", B=1), _call("select", B=4, stream=2)),
                        ("pack", _call("pack", B=1), _call("select_circuit", B=1, stream=2)),
                        ("tgsw", _call("lookup_tree", B=1, n_poly=2), _call("lookup_tree_woks", B=1, stream=2, n_poly=4)),
                        ("dfa", _call("dfa", B=1), _call("dfa_woks", B=2, stream=3)),
                        ("circuit", _call("circuit", B=1), _call("circuit", B=2, stream=2))):
        assert f"regrow:{owner}" in _features([a, b]), owner
        assert f"regrow:{owner}" not in _features([b, a]), owner                 # shrinking is no growth
        assert f"regrow:{owner}" not in _features([b]), owner                    # nor is the first allocation
    assert "regrow:circuit" not in _features([_call("circuit", B=1, ctx="A"), _call("circuit", B=2, ctx="B", stream=2)])
    assert "regrow:tgsw" not in _features([_call("lookup", B=1), _call("lookup_woks", B=5, stream=2)])     # no tree


def test_features_of_objects_switches_and_chains():
    for obj, kind in (("pack", "pack"), ("tgsw", "cmux"), ("dfa", "dfa_woks"), ("circuit", "circuit")):
        assert f"reimport:{obj}" in _features([_call(kind), _state("reimport", obj=obj)]), obj
        assert f"reimport:{obj}" not in _features([_call(kind), _state("ctx_cycle"), _state("reimport", obj=obj)]), obj
        assert f"reimport:{obj}" not in _features([_call("gate"), _state("reimport", obj=obj)]), obj
    # a fresh object has no scratch: the first call after the import allocates, it does not regrow
    assert "regrow:pack" not in _features([_call("pack", B=1), _state("reimport", obj="pack"), _call("gate", stream=3),
                                           _call("pack", B=4, stream=2)])
    for sw in ("guard", "kernel"):
        prog = [_call("gate"), _state(sw + "_flip"), _call("gate", stream=2), _state(sw + "_back")]
        assert f"toggle:{sw}" in _features(prog)
        assert f"toggle:{sw}" not in _features([prog[0], _state("guard_stats", ctx="A")] + prog[1:3])
        assert f"toggle:{sw}" not in _features(prog[1:])
    a = _call("woks", stream=2)
    assert "chain:same-stream" in _features([a, _call("keyswitch", stream=2, chain=(0, "same"))])
    assert "chain:cross-stream" in _features([a, _call("keyswitch", stream=3, chain=(0, "cross"))])
    own_a, own_b = _call("woks", ctx="A", stream=0), _call("keyswitch", ctx="B", stream=0, chain=(0, "cross"))
    assert _features([own_a, own_b]) >= {"chain:cross-stream"}                   # two contexts' own streams differ
    assert "host-between-dev" in _features([_call("gate"), _call("gate_host", stream=0), _call("mux", stream=0)])
    assert "host-between-dev" not in _features([_call("gate"), _call("gate_host", ctx="B", stream=0), _call("mux")])
    assert "host-between-dev" not in _features([_call("gate", stream=0), _call("gate_host", stream=0), _call("mux")])
    warm = [_call("select", B=5, stream=0), _call("select_circuit", B=1, stream=0)]
    trio = [_call("select", B=1, stream=1), _call("select_circuit", B=1, stream=2), _call("pack", B=2, stream=3)]
    assert "pack-key-three-streams" in _features(warm + trio)
    assert "pack-key-three-streams" not in _features(trio)                       # the circuit grows the key's scratch: a sync
    assert "pack-key-three-streams" not in _features(warm[:1] + trio)            # ... and allocates its own: a sync too
    assert "pack-key-three-streams" not in _features(warm + trio[:2] + [_call("pack", B=2, stream=2)])
    assert "object-two-contexts" in _features([_call("cmux", ctx="A"), _call("lookup", ctx="B", stream=2)])
    assert "object-two-contexts" not in _features([_call("cmux", ctx="A"), _call("lookup", ctx="A", stream=2)])
    pair = [_call("lookup_woks", stream=1), _call("bootstrap", stream=2)]
    assert "woks-lookup-next-to-ks" in _features(pair) and "woks-lookup-next-to-ks" in _features(pair[::-1])
    assert "woks-lookup-next-to-ks" not in _features([pair[0], _call("keyswitch", stream=2)])
    assert "woks-lookup-next-to-ks" not in _features([pair[0], _call("bootstrap", ctx="B", stream=2)])


def test_needs_follow_the_growth_rules_of_the_sources():
    """engine.cpp tfhe_amd_reserve: 64 2^k slots; the slots a call reserves; pack.cpp / acc.cpp /
    circuit_select.cpp: digit and accumulator outputs"""
    assert [SF._ctx_cap(n, c) for n, c in ((1, 0), (64, 64), (65, 64), (257, 64), (513, 512), (3, 128))] == \
        [64, 64, 128, 512, 1024, 128]
    assert SF._need("gate", 5, {}) == {"context": 5} and SF._need("keyswitch", 5, {}) == {}
    assert SF._need("many_boot", 5, {"log_nu": 2, "n_out": 3}) == {"context": 15}
    assert SF._need("full_add", 4, {"third": 1}) == {"context": 8}
    assert SF._need("select", 3, {"p": 4}) == {"context": 3, "pack.dig": 3, "pack.acc": 3}
    assert SF._need("select_circuit", 2, {}) == {"pack.dig": 6, "pack.acc": 6, "circuit": 2}
    assert SF._need("lookup_woks", 3, {"n_poly": 1, "n_out": 2}) == {}
    assert SF._need("lookup_tree", 3, {"n_poly": 4, "n_out": 1}) == {"context": 3, "tgsw": 36}
    assert SF._need("dfa_woks", 3, {"n_out": 2}) == {"dfa": 3}
    assert SF.resolve_B("rot", 304) == 305 and SF.resolve_B("ks") == 13 and SF.resolve_B(4) == 4
