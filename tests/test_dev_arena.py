"""tests/dev_arena.py on host memory: the layout it promises, and that check() sees one planted word at
either end of every band and in an input, names the right view, and passes an untouched arena."""
import numpy as np
import pytest

import dev_arena as DA

SEED = 20261
OUTS = [("res_a", (5, 500)), ("res_b", (5,))]


def _arena(poison):
    rng = np.random.default_rng(SEED)
    inps = [("u_a", rng.integers(-2**31, 2**31, (5, 1024), dtype=np.int64).astype(np.int32)),
            ("u_b", rng.integers(-2**31, 2**31, 5, dtype=np.int64).astype(np.int32)),
            ("idx", np.arange(7, dtype=np.int32))]
    a, v = DA.Arena.of("cpu", poison, OUTS, inps)
    return a, v, dict(inps)


@pytest.mark.parametrize("poison", DA.POISONS)
def test_layout(poison):
    a, v, host = _arena(poison)
    shapes = dict(OUTS, **{k: h.shape for k, h in host.items()})
    assert [n for n, *_ in a.views] == ["res_a", "res_b", "u_a", "u_b", "idx"]     # the order asked for
    prev_end = 0
    for name, start, end, is_input, _ in a.views:
        assert start % DA.ALIGN == 0, (name, start)
        assert v[name].data_ptr() == a.buf.data_ptr() + 4 * start
        assert v[name].data_ptr() % (4 * DA.ALIGN) == 0, name
        assert v[name].is_contiguous() and tuple(v[name].shape) == tuple(shapes[name]), name
        assert end - start == int(np.prod(shapes[name])) and start - prev_end >= DA.BAND, (name, start, prev_end)
        assert is_input == (name in host)
        prev_end = end
    assert a.cur - prev_end >= DA.BAND and a.cur <= a.words          # the last view has its band too
    bands = a.bands()
    assert [b[0] for b in bands] == [DA.START, "res_a", "res_b", "u_a", "u_b", "idx"]
    assert bands[0][1] == 0 and all(e - s >= DA.BAND for _, s, e in bands)
    # bands and views tile the arena: the alignment slack behind a view is band
    edges = sorted([(s, e) for _, s, e in bands] + [(s, e) for _, s, e, _, _ in a.views])
    assert edges[0][0] == 0 and edges[-1][1] == a.cur
    assert all(edges[i][1] == edges[i + 1][0] for i in range(len(edges) - 1))
    # outputs are poison, inputs hold their data, and neither poison has a zero word
    want = DA._poison_words(poison, a.words, "cpu").numpy()
    assert not np.any(want == 0)
    if poison == "const":
        assert np.all(want.view(np.uint32) == DA.POISON)
    else:
        i = np.arange(a.words, dtype=np.uint64)
        prod = (i * np.uint64(DA.GOLDEN)) & np.uint64(0xFFFFFFFF)
        special = (prod == 0) | (prod == DA.POISON)
        assert special[0] and np.array_equal(want.view(np.uint32)[~special], prod[~special].astype(np.uint32))
        assert np.all(want.view(np.uint32)[special] == DA.INDEX_FALLBACK) and not np.any(want.view(np.uint32) == DA.POISON)
    for name, start, end, is_input, _ in a.views:
        got = v[name].numpy().reshape(-1)
        assert np.array_equal(got, host[name].reshape(-1) if is_input else want[start:end]), name
    a.check()


@pytest.mark.parametrize("poison", DA.POISONS)
def test_untouched_arena_passes_and_outputs_may_change(poison):
    a, v, _ = _arena(poison)
    a.check()
    v["res_a"].zero_()
    v["res_b"].fill_(7)
    a.check()


@pytest.mark.parametrize("poison", DA.POISONS)
@pytest.mark.parametrize("edge", ["first", "last"])
def test_planted_band_word_is_reported_by_name(poison, edge):
    a, _, _ = _arena(poison)
    for name, start, end in a.bands():
        w = start if edge == "first" else end - 1
        keep = int(a.buf[w])
        a.buf[w] = 0                      # a stray zero: neither poison has a zero word
        with pytest.raises(AssertionError) as e:
            a.check()
        msg = str(e.value)
        assert f"band after {name!r} damaged at offset {w - start} " in msg, (name, edge, msg)
        assert f"arena word {w})" in msg and "1 band words damaged" in msg, msg
        a.buf[w] = keep
        a.check()


def test_first_damaged_band_is_the_one_reported():
    a, _, _ = _arena("index")
    bands = a.bands()
    a.buf[bands[3][1] + 5] = 1
    a.buf[bands[1][2] - 1] = 1
    with pytest.raises(AssertionError, match=r"band after 'res_a' damaged at offset \d+ .*2 band words damaged"):
        a.check()


@pytest.mark.parametrize("poison", DA.POISONS)
def test_planted_input_word_is_reported_and_aliased_exempts_only_the_named_input(poison):
    a, v, host = _arena(poison)
    for name in host:
        flat = v[name].view(-1)
        at = flat.numel() - 1
        keep = int(flat[at])
        flat[at] = keep ^ 1
        with pytest.raises(AssertionError) as e:
            a.check()
        assert f"input {name!r} changed at word {at}:" in str(e.value), str(e.value)
        a.check(aliased=(name,))                                        # exempt when named ...
        others = tuple(k for k in host if k != name)
        with pytest.raises(AssertionError, match=f"input '{name}' changed"):
            a.check(aliased=others)                                     # ... and only then
        flat[at] = keep
        a.check()
    with pytest.raises(AssertionError, match="not an input view"):
        a.check(aliased=("res_a",))


@pytest.mark.parametrize("poison", DA.POISONS)
def test_skewed_views_are_word_aligned_only(poison):
    """skew=True: view k starts 1 + k mod 3 words behind a 512-byte multiple, so no view is 16-byte
    aligned and the offsets 1, 2, 3 take turns; the views named in `aligned` keep
    the multiple; bands and views still tile the arena, every band is still at least BAND words, the
    data is where the views say, and a planted word at either end of every band is reported"""
    rng = np.random.default_rng(SEED)
    inps = [("u_a", rng.integers(-2**31, 2**31, (5, 1024), dtype=np.int64).astype(np.int32)),
            ("u_b", rng.integers(-2**31, 2**31, 5, dtype=np.int64).astype(np.int32)),
            ("idx", np.arange(7, dtype=np.int32))]
    a, v = DA.Arena.of("cpu", poison, OUTS, inps, skew=True, aligned=("u_a",))
    assert a.words == DA.words_for([s for _, s in OUTS] + [h.shape for _, h in inps], skew=True)
    assert [DA.skew_of(k) for k in range(5)] == [1, 2, 3, 1, 2]
    want_skew = {"res_a": 1, "res_b": 2, "u_a": 0, "u_b": 1, "idx": 2}        # by position; u_a exempt
    prev_end = 0
    for name, start, end, is_input, _ in a.views:
        assert start % DA.ALIGN == want_skew[name], (name, start)
        assert (v[name].data_ptr() - a.buf.data_ptr()) == 4 * start and a.buf.data_ptr() % (4 * DA.ALIGN) == 0
        assert v[name].data_ptr() % 4 == 0 and (v[name].data_ptr() % 16 == 0) == (name == "u_a"), name
        assert v[name].is_contiguous() and start - prev_end >= DA.BAND, (name, start, prev_end)
        prev_end = end
    assert {s % DA.ALIGN for _, s, *_ in a.views} == {0, 1, 2}                # u_a took offset 3's place
    assert a.cur - prev_end >= DA.BAND and a.cur <= a.words
    bands = a.bands()
    edges = sorted([(s, e) for _, s, e in bands] + [(s, e) for _, s, e, _, _ in a.views])
    assert edges[0][0] == 0 and edges[-1][1] == a.cur
    assert all(edges[i][1] == edges[i + 1][0] for i in range(len(edges) - 1))
    assert all(e - s >= DA.BAND for _, s, e in bands)
    for name, host in inps:
        assert np.array_equal(v[name].numpy(), host), name
    a.check()
    for name, start, end in bands:
        for w in (start, end - 1):
            keep = int(a.buf[w])
            a.buf[w] = 0
            with pytest.raises(AssertionError, match=f"band after {name!r} damaged at offset {w - start} "):
                a.check()
            a.buf[w] = keep
    flat = v["u_b"].view(-1)
    flat[0] ^= 1
    with pytest.raises(AssertionError, match="input 'u_b' changed at word 0:"):
        a.check()
    flat[0] ^= 1
    a.check()


def test_skew_is_off_by_default():
    """the default layout is what it was: the same size and the same starts with and without the argument"""
    shapes = [s for _, s in OUTS]
    assert DA.words_for(shapes) == DA.words_for(shapes, skew=False) <= DA.words_for(shapes, skew=True)
    assert DA.words_for([(DA.ALIGN - 2,)] * 4) < DA.words_for([(DA.ALIGN - 2,)] * 4, skew=True)    # the offsets need room
    a, v = DA.Arena.of("cpu", "const", OUTS)
    b, w = DA.Arena.of("cpu", "const", OUTS, skew=False)
    assert [x[1:3] for x in a.views] == [x[1:3] for x in b.views] and all(x[1] % DA.ALIGN == 0 for x in a.views)
    assert not a.skew and a.words == b.words


def test_host_backing_and_shared_poison_function():
    """an arena over caller-owned memory (the pinned host buffers of the host entry points) lies in
    that memory; poisoned() is the constant poison"""
    words = DA.words_for([(3, 500), (3,)])
    raw = np.zeros(words + DA.ALIGN, np.int32)
    skip = (-raw.ctypes.data // 4) % DA.ALIGN
    backing = raw[skip:skip + words]
    a, v = DA.Arena.of("cpu", "const", [("r_a", (3, 500)), ("r_b", (3,))], backing=backing)
    assert a.numpy(v["r_a"]).ctypes.data == backing.ctypes.data + 4 * a.offset("r_a")
    assert np.all(backing.view(np.uint32) == DA.POISON)
    backing[a.offset("r_a") + 1500] = 0          # the first band word behind r_a, through the caller's array
    with pytest.raises(AssertionError, match="band after 'r_a' damaged at offset 0 "):
        a.check()
    with pytest.raises(ValueError, match="too small"):
        DA.Arena("cpu", "const", DA.BAND + DA.ALIGN).out((3, 500), "x")
    t = DA.poisoned((2, 3), device="cpu")
    assert t.dtype.is_signed and np.all(t.numpy().view(np.uint32) == DA.POISON)
