"""Poisoned outputs and guard bands for the device entry points (TEST INFRASTRUCTURE: the helper of
tests/test_write_discipline_gpu.py and the poisoned output allocations of the other GPU tests).

An Arena is ONE int32 allocation that holds every tensor of one call under test:

    band | view | band | view | band | ...

  - every view starts at a multiple of ALIGN = 128 words (512 B), the alignment a fresh torch
    allocation has, so no 16-byte vector load of a kernel behaves differently on a view; with
    skew=True view k starts 1 + k mod 3 words behind that multiple instead (the words skipped belong
    to the band in front of it), so its pointer is word-aligned only, as a caller's tightly packed
    arrays are — except the views named in `aligned`, for the one pointer the library wants 16-byte
    aligned (include/tfhe_amd.h: the u_a of tfhe_amd_keyswitch_batch_dev);
  - every view is followed by a band of at least BAND = 2048 poisoned words (two of the widest rows,
    1024 words, and more than the 512-thread key-switch block), the arena begins with such a band,
    and the alignment slack behind a view belongs to its band;
  - views lie in the order they are asked for: the outputs `a` and `b` of a call, asked for one after
    the other, have one band between them, so an overrun of one is a hit on that band or on the other.

out(shape) is filled with poison as the bands are; inp(host_array) holds the data and the arena keeps
the host copy.  Two poisons, neither ever zero:

  "const"  every word 0xA5A5A5A5;
  "index"  word i of the arena holds i * 0x9E3779B9 mod 2^32 (0x5A5A5A5B where that product is 0 or
           the constant poison), so a copy of a band word to another place is seen too.

check(aliased=()) — after the caller has synchronised — asserts that every band word still holds its
poison (the first damaged band is reported by the name of the view it follows and the offset in the
band) and that every input view not named in `aliased` equals its host copy.

The module needs no GPU to import; device="cpu" runs the same code on host memory (tests/test_dev_arena.py,
and the host entry points: a.numpy(view) is the numpy array over a view's words).  `backing` is a
caller-owned int32 array the arena lies in instead of a fresh allocation (pinned host memory)."""
import bisect

import numpy as np
import torch

ALIGN = 128
BAND = 2048
POISON = 0xA5A5A5A5
POISON_I32 = POISON - (1 << 32)        # the same word as int32
GOLDEN = 0x9E3779B9
INDEX_FALLBACK = 0x5A5A5A5B            # where i * GOLDEN mod 2^32 is 0 or POISON
POISONS = ("const", "index")
START = "<arena start>"


def poisoned(shape, device="cuda", dtype=torch.int32):
    """a fresh tensor whose every word is the constant poison: what a GPU test hands the library as
    an output (torch.zeros would hide a row that was never written when the right answer is 0)"""
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), POISON_I32, dtype=dtype, device=device)


def _round_up(x, m):
    return (x + m - 1) // m * m


def _count(shape):
    shape = (shape,) if isinstance(shape, int) else tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    return shape, n


SKEW_MAX = 3


def skew_of(k):
    """words view k of a skewed arena starts behind its 512-byte multiple: 1, 2, 3, 1, ..."""
    return 1 + k % SKEW_MAX


def words_for(shapes, skew=False):
    """arena words for views of these shapes, in this order (skew: room for every view's offset)"""
    cur = BAND
    for s in shapes:
        cur = _round_up(cur + (SKEW_MAX if skew else 0) + _count(s)[1] + BAND, ALIGN)
    return cur


def _poison_words(kind, n, device):
    if kind == "const":
        return torch.full((n,), POISON_I32, dtype=torch.int32, device=device)
    if kind != "index":
        raise ValueError(f"poison: need one of {POISONS}, got {kind!r}")
    w = (torch.arange(n, dtype=torch.int64, device=device) * GOLDEN) & 0xFFFFFFFF
    w = torch.where((w == 0) | (w == POISON), torch.full_like(w, INDEX_FALLBACK), w)
    return torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)


class Arena:
    def __init__(self, device, poison, words, backing=None, skew=False, aligned=()):
        """words: the arena's size (words_for(shapes, skew) of the views that will be asked for)"""
        self.device = torch.device(device)
        self.skew = bool(skew)
        self.aligned = frozenset(aligned)
        self.kind = poison
        self.words = int(words)
        if backing is None:
            raw = torch.empty(self.words + ALIGN, dtype=torch.int32, device=self.device)
            skip = (-raw.data_ptr() // 4) % ALIGN       # host allocators promise less than 512 B
            self.buf = raw[skip:skip + self.words]
        else:
            assert backing.dtype == np.int32 and backing.ndim == 1 and backing.flags["C_CONTIGUOUS"]
            assert backing.shape[0] >= self.words and backing.ctypes.data % (4 * ALIGN) == 0, "backing: size / alignment"
            self.buf = torch.from_numpy(backing)[:self.words]
        self.poison = _poison_words(poison, self.words, self.device)
        self.buf.copy_(self.poison)
        self.cur = BAND
        self.views = []                 # (name, start, end, is_input, host copy or None)
        self.band_starts = [0]          # band k lies in [band_starts[k], start of view k), the last one to self.cur
        self.band_names = [START]
        self._sync()

    @classmethod
    def of(cls, device, poison, outs=(), inps=(), backing=None, skew=False, aligned=()):
        """the arena of one call: outs [(name, shape)], then inps [(name, host array)], in that order ->
        (arena, {name: view})"""
        shapes = [s for _, s in outs] + [np.asarray(h).shape for _, h in inps]
        a = cls(device, poison, words_for(shapes, skew), backing, skew, aligned)
        v = {name: a.out(shape, name) for name, shape in outs}
        v.update(a.inp_many(inps))
        return a, v

    def _sync(self):
        # the fills run on torch's stream, the library on its own non-blocking one
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def _carve(self, shape, name):
        shape, n = _count(shape)
        name = name if name is not None else f"view{len(self.views)}"
        start = self.cur + (skew_of(len(self.views)) if self.skew and name not in self.aligned else 0)
        end = start + n
        nxt = _round_up(end + BAND, ALIGN)
        if nxt > self.words:
            raise ValueError(f"arena of {self.words} words is too small for view {name!r} {shape}")
        assert name != START and all(name != v[0] for v in self.views), f"view name {name!r} taken"
        self.cur = nxt
        self.band_starts.append(end)
        self.band_names.append(name)
        return name, start, end, self.buf[start:end].view(shape)

    def out(self, shape, name=None):
        """a contiguous view of this shape, every word poison"""
        name, start, end, view = self._carve(shape, name)
        self.views.append((name, start, end, False, None))
        return view

    def inp_many(self, inps):
        """inp for several arrays with one synchronisation -> {name: view}"""
        got = {}
        for name, host in inps:
            host = np.ascontiguousarray(np.asarray(host)).astype(np.int32, copy=True)
            name, start, end, view = self._carve(host.shape, name)
            view.copy_(torch.from_numpy(host))
            self.views.append((name, start, end, True, host))
            got[name] = view
        self._sync()
        return got

    def inp(self, host_array, name=None):
        """a contiguous view that holds the array's words; the arena keeps the host copy"""
        name = name if name is not None else f"view{len(self.views)}"
        return self.inp_many([(name, host_array)])[name]

    def offset(self, name):
        """the first word of a view in the arena"""
        return next(v[1] for v in self.views if v[0] == name)

    def bands(self):
        """[(name of the view the band follows, first word, end)] over the words handed out so far"""
        ends = [v[1] for v in self.views] + [self.cur]
        return [(self.band_names[k], self.band_starts[k], ends[k]) for k in range(len(self.band_starts))]

    def numpy(self, view):
        """host arenas: the numpy array over a view's words (shares memory)"""
        return view.numpy()

    def check(self, aliased=()):
        """every band word still poison, every input not in `aliased` equal to its host copy"""
        unknown = set(aliased) - {v[0] for v in self.views if v[3]}
        assert not unknown, f"aliased: not an input view: {sorted(unknown)}"
        is_band = torch.ones(self.cur, dtype=torch.bool, device=self.device)
        for _, start, end, _, _ in self.views:
            is_band[start:end] = False
        bad = torch.nonzero((self.buf[:self.cur] != self.poison[:self.cur]) & is_band)
        if bad.numel():
            w = int(bad[0])
            k = bisect.bisect_right(self.band_starts, w) - 1
            got = int(self.buf[w]) & 0xFFFFFFFF
            want = int(self.poison[w]) & 0xFFFFFFFF
            raise AssertionError(
                f"band after {self.band_names[k]!r} damaged at offset {w - self.band_starts[k]} (arena word {w}): "
                f"0x{got:08X}, poison 0x{want:08X} ({self.kind}); {int(bad.numel())} band words damaged in all")
        for name, start, end, is_input, host in self.views:
            if not is_input or name in aliased:
                continue
            now = self.buf[start:end].cpu().numpy()
            diff = np.flatnonzero(now != host.reshape(-1))
            if diff.size:
                raise AssertionError(f"input {name!r} changed at word {int(diff[0])}: 0x{int(now[diff[0]]) & 0xFFFFFFFF:08X}, "
                                     f"was 0x{int(host.reshape(-1)[diff[0]]) & 0xFFFFFFFF:08X}; {diff.size} words changed")
