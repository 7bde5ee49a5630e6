"""Seeded random circuits for the differential fuzz of the circuit compiler (TEST INFRASTRUCTURE:
tests/test_dag_fuzz.py checks the generator and the compiler's schedule without a GPU,
tests/test_circuit_fuzz_gpu.py runs the cases against tests/dag_oracle.py).

make_case(seed, profile) builds a circuit from np.random.default_rng(seed) alone: the same seed
gives the same node list in every process.  Inputs and tables are uniformly random Torus32 words —
the GPU and the oracle are exact integer maps, so nothing has to decrypt — coefficients come from
{0, +-1, +-2, 3, 2^16, 2^31 - 1, -2^31} and random words, constants from the edges of the negacyclic
rotation and random words.

schedule(C) is an independent leveller over node() (rules in its docstring): the compiler's
level_sizes(), bootstraps and wires must agree with it, and the GPU test derives from it which
kernels a run must have launched.  features_of(C, full_add_wires) names what a circuit contains,
by inspection of its node list, never by what the generator meant to build.

Adding a seed: append it to SMALL_SEEDS (or to WIDE_SEEDS / SEAM_SEEDS); a seed that once failed
stays in the list."""
import numpy as np

import dag_oracle as DO

N, n_lwe = 1024, 500
E8 = 1 << 29
MUX, NOT, COPY, CONST = 10, 13, 14, 15
LUT_GATE, LUT_MANY_GATE, AFFINE_GATE = -2, -3, -4
GATES2 = ["NAND", "OR", "AND", "XOR", "XNOR", "NOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
GATES3 = ["MAJ", "XOR3"]
MANY_SHAPES = [(1, 2), (2, 3), (4, 16)]

FEATURES = (
    "mux+lut-row",              # MUX in one level with a plain LUT row
    "mux+many-row",             # ... with a many-LUT row
    "mux+full-add",             # ... with a full_add cell
    "mux-one-wire",             # MUX whose three inputs are one wire
    "mux-const-select",         # MUX whose select is a CONST
    "mux-over-not-affine",      # MUX over NOT / affine of wires
    "row-const-inputs",         # a bootstrapped row with only constant inputs
    "row-one-wire-x3",          # a row with one wire in all three slots
    "row-cancel",               # a row whose coefficients on a wire cancel (x and NOT x)
    "affine-s0",                # affine with s = 0
    "affine-chain-2^16",        # two chained affine with s = 2^16 (product 0 mod 2^32)
    "free-chain-depth3",        # a NOT / COPY / affine chain of depth >= 3
    "free-on-many-extra",       # a bootstrap-free node on a many-LUT output of index >= 1
    "free-on-inputs",           # a bootstrap-free node over inputs only (level 0)
    "many(1,2)", "many(2,3)", "many(4,16)",
    "two-log-nu+gate-row",      # two many-LUT rows of different log_nu plus a gate row in one level
    "extra-next-level",         # a many-LUT output of index >= 1 consumed in the next level,
    "extra-two-levels-later",   # two levels later,
    "extra-never",              # never
    "wire-unread",              # a wire nobody reads
)

SMALL_SEEDS = [101, 102, 103, 104, 105, 106, 107, 114]
WIDE_SEEDS = [201]
SEAM_SEEDS = [301, 302]          # odd: the launch seam inside a MUX pair, even: inside a many-LUT row
SMALL_B = (1, 3)


def _i32(v):
    return int((int(v) + 2**31) % 2**32 - 2**31)


# ---------------------------------------------------------------- the independent leveller

def schedule(C):
    """Levels of a circuit from node() alone.

    Every wire has a source: itself for an input and for a bootstrapped output, none for a constant,
    and for a bootstrap-free node the source of its input — unless the scales composed along the
    chain multiply to 0 mod 2^32 (s = 0, or 2^16 twice), which makes the wire a constant by value.
    depth(wire) = depth(source), 0 without one; a bootstrapped node has depth 1 + the largest depth
    among its inputs' sources (1 when all are constants).  A zero coefficient of a row on a live
    wire is still a read.  A MUX is 2 rows and 1 key switch, any other bootstrapped node 1 row and
    1 key switch; a many-LUT node is 1 row, and its n_out - 1 further outputs are counted apart
    (extras) with one key switch each.  A level's launch form is "lut-many" when it holds a many-LUT
    row, else "lut" when it holds a LUT row, else "" (the constant test vector).
    -> dict(wires, depth [wire], rows [level], extras [level], ks [level], form [level], bootstraps)"""
    n_w = DO.count_wires(C)
    src, scale, depth = [None] * n_w, [0] * n_w, [0] * n_w
    rows, extras, ks, form = [0], [0], [0], [""]

    def level(d):
        while len(rows) <= d:
            rows.append(0); extras.append(0); ks.append(0); form.append("")
    for w in range(n_w):
        kind, gate, c0, s, ins = C.node(w)
        if kind == 0:
            src[w], scale[w] = w, 1
        elif kind == 2:
            if gate != CONST:
                k = {NOT: -1, COPY: 1}.get(gate, s[0])
                scale[w] = (scale[ins[0]] * k) % 2**32
                src[w] = src[ins[0]] if scale[w] else None
            depth[w] = depth[src[w]] if src[w] is not None else 0
            level(depth[w])
        else:
            src[w], scale[w] = w, 1
            if gate == LUT_MANY_GATE:
                _, _, _, n_out, index = C.lut_many_node(w)
                if index:
                    depth[w] = depth[w - index]
                    continue
            d = 1 + max([depth[src[i]] for i in ins if i >= 0 and src[i] is not None], default=0)
            depth[w] = d
            level(d)
            rows[d] += 2 if gate == MUX else 1
            ks[d] += 1
            if gate == LUT_GATE and form[d] == "":
                form[d] = "lut"
            if gate == LUT_MANY_GATE:
                extras[d] += n_out - 1
                ks[d] += n_out - 1
                form[d] = "lut-many"
    return dict(wires=n_w, depth=depth, rows=rows, extras=extras, ks=ks, bootstraps=sum(rows), src=src, form=form)


def expected_kernels(sched, B, cus, guard=True):
    """the trace names a run of B instances on the default path must hold, from the launchers'
    documented thresholds: a rows launch covers at most 4 CUs slots and rotates in registers above
    one workgroup per CU, the guard's exact launch follows with the level's form; up to 12 key
    switches take the small kernel, more the int8 MFMA one ("k_keyswitch_v5(": any split)"""
    want = set()
    for d in range(1, len(sched["rows"])):
        total, form = sched["rows"][d] * B, sched["form"][d]
        for base in range(0, total, 4 * cus):
            rot = "reg-rotation" if min(total - base, 4 * cus) > cus else "lds-rotation"
            want.add("k_blind_rotate_v6_rows(%s)" % "+".join(p for p in (form, rot) if p))
        if guard and total:
            want.add("k_blind_rotate_v4_rows(%s)" % "+".join(p for p in (form, "guard") if p))
        if sched["ks"][d]:
            want.add("k_keyswitch_small" if sched["ks"][d] * B <= 12 else "k_keyswitch_v5(")
    return want


# ---------------------------------------------------------------- what a circuit contains

def features_of(C, full_add_wires=()):
    sched = schedule(C)
    n_w, depth, src = sched["wires"], sched["depth"], sched["src"]
    nodes = [C.node(w) for w in range(n_w)]
    many = {w: C.lut_many_node(w) for w in range(n_w) if nodes[w][1] == LUT_MANY_GATE}
    first = lambda w: w not in many or many[w][4] == 0      # not a further wire of a many-LUT node
    boot = [w for w in range(n_w) if nodes[w][0] == 1 and first(w)]
    free = [w for w in range(n_w) if nodes[w][0] == 2 and nodes[w][1] != CONST]
    readers = {w: [] for w in range(n_w)}
    for w in range(n_w):
        if nodes[w][0] != 0 and first(w):
            for i in set(nodes[w][4]):
                if i >= 0:
                    readers[i].append(w)
    F = set()
    by_level = {}
    for w in boot:
        by_level.setdefault(depth[w], []).append(w)
    for ws in by_level.values():
        gates = [nodes[w][1] for w in ws]
        if MUX in gates:
            if LUT_GATE in gates:
                F.add("mux+lut-row")
            if any(nodes[w][1] == LUT_MANY_GATE and w not in full_add_wires for w in ws):
                F.add("mux+many-row")
            if any(w in full_add_wires for w in ws):
                F.add("mux+full-add")
        thetas = {many[w][2] for w in ws if w in many}
        if len(thetas) >= 2 and any(g >= -1 and g != MUX for g in gates):
            F.add("two-log-nu+gate-row")
    for w in boot:
        kind, gate, c0, s, ins = nodes[w]
        if gate == MUX:
            if ins[0] == ins[1] == ins[2]:
                F.add("mux-one-wire")
            if nodes[ins[0]][1] == CONST:
                F.add("mux-const-select")
            if any(nodes[i][1] in (NOT, AFFINE_GATE) and src[i] is not None for i in ins):
                F.add("mux-over-not-affine")
            continue
        live = [i for i in ins if i >= 0]
        if all(src[i] is None for i in live):
            F.add("row-const-inputs")
        if len(live) == 3 and ins[0] == ins[1] == ins[2]:
            F.add("row-one-wire-x3")
        for j in range(3):
            for k in range(3):
                if ins[j] >= 0 and ins[k] >= 0 and nodes[ins[k]][1] == NOT and nodes[ins[k]][4][0] == ins[j] \
                        and s[j] == s[k] != 0:
                    F.add("row-cancel")
        if w in many:
            F.add("many(%d,%d)" % (many[w][2], many[w][3]))
    chain = {}
    for w in free:
        kind, gate, c0, s, ins = nodes[w]
        chain[w] = 1 + chain.get(ins[0], 0)
        if chain[w] >= 3:
            F.add("free-chain-depth3")
        if gate == AFFINE_GATE and s[0] == 0:
            F.add("affine-s0")
        if gate == AFFINE_GATE and s[0] == 1 << 16 and nodes[ins[0]][1] == AFFINE_GATE and nodes[ins[0]][3][0] == 1 << 16:
            F.add("affine-chain-2^16")
        if ins[0] in many and many[ins[0]][4] >= 1:
            F.add("free-on-many-extra")
        if nodes[ins[0]][0] == 0:
            F.add("free-on-inputs")

    def consumers(w, seen):
        """depths of the bootstrapped nodes that read w, directly or through bootstrap-free nodes"""
        out = set()
        for r in readers[w]:
            if nodes[r][0] == 1:
                out.add(depth[r])
            elif r not in seen:
                seen.add(r)
                out |= consumers(r, seen)
        return out
    for w, m in many.items():
        if m[4] >= 1:
            used = consumers(w, set())
            if depth[w] + 1 in used:
                F.add("extra-next-level")
            if depth[w] + 2 in used:
                F.add("extra-two-levels-later")
            if not readers[w]:
                F.add("extra-never")
    if any(not readers[w] for w in range(n_w) if nodes[w][0] != 0):
        F.add("wire-unread")
    return F


# ---------------------------------------------------------------- the generator

class _Gen:
    def __init__(self, seed):
        import tfhe_amd as T
        self.rng = np.random.default_rng(int(seed))
        self.C = T.Circuit()
        self.by_depth = {}        # depth -> wires a later node may read
        self.hold = {}            # wire -> first level that may read it
        self.due = {}             # level -> wires some bootstrapped node of it must read
        self.fa = set()           # first wires of full_add cells
        self.tables = []
        self.n_boot = 0
        self.dep, self.scale = {}, {}

    # ---- random words
    def word(self):
        return int(self.rng.integers(-2**31, 2**31))

    def coef(self):
        if self.rng.random() < 0.65:
            return int(self.rng.choice([0, 1, -1, 2, -2, 3, 1 << 16, 2**31 - 1, -2**31]))
        return self.word()

    def nz_coef(self):
        c = self.coef()
        return c if c else 1

    def c0(self):
        """a rotation edge (0 and 1/8; the words whose modulus switch gives N - 1, N, 2N - 1; the
        rounding boundary 2^20, and 2^32 - 2^20, which wraps to 0) or a random word"""
        if self.rng.random() < 0.6:
            return _i32(int(self.rng.choice([0, E8, 1 << 20, (N - 1) << 21, N << 21, (2 * N - 1) << 21,
                                             2**32 - (1 << 20)])))
        return self.word()

    def table(self):
        """a table of uniformly random words: a new one, or one that other rows already use"""
        if not self.tables or self.rng.random() < 0.4:
            tv = self.rng.integers(-2**31, 2**31, N, dtype=np.int64).astype(np.int32)
            self.tables.append(self.C.lut_table(tv))
            return self.tables[-1]
        return int(self.rng.choice(self.tables))

    # ---- bookkeeping: depths follow schedule()'s rules, from the generator's own arguments
    def put(self, w, d, n=1, scale=1):
        for f in range(n):
            self.by_depth.setdefault(d, []).append(w + f)
            self.dep[w + f], self.scale[w + f] = d, scale
        return w

    def open(self, d):
        """wires of depth d that a node may still read (not kept for "never")"""
        return [w for w in self.by_depth.get(d, []) if self.hold.get(w, 0) < 1 << 30]

    def pool(self, d):
        """wires a node of level d may read without leaving it: depth < d, released"""
        return [w for k, ws in self.by_depth.items() if k < d for w in ws if self.hold.get(w, 0) <= d]

    def pick(self, d, k):
        """k input wires for a bootstrapped node of level d: one of depth d - 1, a due wire if one
        waits, the rest anywhere below d"""
        front = [w for w in self.by_depth.get(d - 1, []) if self.hold.get(w, 0) <= d]
        ins = [int(self.rng.choice(front))]
        if k > 1 and self.due.get(d):
            ins.append(self.due[d].pop())
        pool = self.pool(d)
        while len(ins) < k:
            ins.append(int(self.rng.choice(pool)))
        return ins

    def lin(self, kind, x, c0=0, s=1):
        """a bootstrap-free node on wire x: it keeps x's depth and release level, unless the composed
        scale is 0 mod 2^32, which makes it a constant"""
        if kind == "affine":
            w, k = self.C.affine(c0, s, x), s
        else:
            w, k = self.C.gate(kind, x), (-1 if kind == "NOT" else 1)
        scale = (self.scale[x] * k) % 2**32
        if self.hold.get(x):
            self.hold[w] = self.hold[x]
        return self.put(w, self.dep[x] if scale else 0, scale=scale)

    def const(self, bit):
        return self.put(self.C.gate("CONST", bit), 0, scale=0)

    # ---- bootstrapped nodes of level d
    def gate(self, d):
        if self.rng.random() < 0.3:
            a, b, c = self.pick(d, 3)
            w = self.C.gate(str(self.rng.choice(GATES3)), a, b, c)
        else:
            a, b = self.pick(d, 2)
            w = self.C.gate(str(self.rng.choice(GATES2)), a, b)
        self.n_boot += 1
        return self.put(w, d)

    def lincomb(self, d):
        a, b, c = self.pick(d, 3)
        self.n_boot += 1
        return self.put(self.C.lincomb(self.c0(), self.nz_coef(), a, self.coef(), b, self.coef(), c), d)

    def mux(self, d, ins=None):
        a, b, c = ins or self.pick(d, 3)
        self.n_boot += 2
        return self.put(self.C.gate("MUX", a, b, c), d)

    def lut(self, d, ins=None, coefs=None):
        a, b, c = ins or self.pick(d, 3)
        sa, sb, sc = coefs or (self.nz_coef(), self.coef(), self.coef())
        self.n_boot += 1
        return self.put(self.C.lut(self.table(), self.c0(), sa, a, sb, b, sc, c), d)

    def many(self, d, shape=None, last=None):
        """a many-LUT row; last: the level of the circuit's last but one level, for the obligations
        on its further outputs (read in the next level, two levels later, never)"""
        log_nu, n_out = shape or MANY_SHAPES[int(self.rng.integers(len(MANY_SHAPES)))]
        a, b, c = self.pick(d, 3)
        w = self.C.lut_many(self.table(), log_nu, n_out, self.c0(), self.nz_coef(), a, self.coef(), b, self.coef(), c)
        self.n_boot += 1
        self.put(w, d, n_out)
        if last is not None and n_out >= 2:
            plan = ["never", "next", "later"] if n_out >= 3 else [str(self.rng.choice(["never", "next", "later"]))]
            for f, what in zip(range(n_out - 1, 0, -1), plan):
                if what == "never":
                    self.hold[w + f] = 1 << 30
                elif what == "next" and d + 1 <= last:
                    self.due.setdefault(d + 1, []).append(w + f)
                elif what == "later" and d + 2 <= last:
                    self.hold[w + f] = d + 2
                    self.due.setdefault(d + 2, []).append(w + f)
        return w

    def full_add(self, d):
        import tfhe_amd as T
        a, b, c = self.pick(d, 3)
        enc = (T.ENC_GATE, T.ENC_HALF)
        s, co = self.C.full_add(a, b, c if self.rng.random() < 0.7 else -1, enc[int(self.rng.integers(2))],
                                enc[int(self.rng.integers(2))])
        self.fa.add(s)
        self.n_boot += 1
        return self.put(s, d, 2)

    # ---- bootstrap-free nodes over wires of depth d
    def free(self, d, x=None):
        x = int(self.rng.choice(self.open(d))) if x is None else x
        r = self.rng.random()
        if r < 0.3:
            return self.lin("NOT", x)
        if r < 0.45:
            return self.lin("COPY", x)
        return self.lin("affine", x, self.c0(), self.nz_coef())

    # ---- the corners no builder emits
    def special(self, name, d):
        rng = self.rng
        if name == "mux-one-wire":
            x = self.pick(d, 1)[0]
            self.mux(d, (x, x, x))
        elif name == "mux-const-select":
            a, b = self.pick(d, 2)
            self.mux(d, (self.const(int(rng.integers(2))), a, b))
        elif name == "mux-over-not-affine":
            a, b, c = self.pick(d, 3)
            self.mux(d, (a, self.lin("NOT", b), self.lin("affine", c, self.c0(), self.nz_coef())))
        elif name == "row-const-inputs":      # lands in level 1 wherever it is asked for
            k1 = self.const(1)
            k2 = self.lin("affine", k1, self.word(), self.nz_coef())
            self.put(self.C.lut(self.table(), self.c0(), self.nz_coef(), k1, self.nz_coef(), k2), 1)
            self.put(self.C.lincomb(self.c0(), self.nz_coef(), k2, self.nz_coef(), self.const(0)), 1)
            self.n_boot += 2
        elif name == "row-one-wire-x3":
            x = self.pick(d, 1)[0]
            self.lut(d, (x, x, x), (self.nz_coef(), self.nz_coef(), self.nz_coef()))
        elif name == "row-cancel":
            x, y = self.pick(d, 2)
            s = self.nz_coef()
            self.lut(d, (x, self.lin("NOT", x), y), (s, s, self.nz_coef()))
        elif name == "affine-s0":
            z = self.lin("affine", int(rng.choice(self.open(d - 1))), self.c0(), 0)
            self.lin("affine", z, self.word(), self.nz_coef())
        elif name == "affine-chain-2^16":
            y = self.lin("affine", int(rng.choice(self.open(d - 1))), self.word(), 1 << 16)
            self.lin("affine", y, self.word(), 1 << 16)
        elif name == "free-chain-depth3":
            x = None
            for _ in range(int(rng.integers(3, 6))):
                x = self.free(d - 1, x)
        else:
            raise KeyError(name)

    def free_on_extras(self, d):
        """bootstrap-free nodes on further outputs of level d's many-LUT rows that may be read"""
        for w in self.open(d):
            kind, gate, _, _, _ = self.C.node(w)
            if gate == LUT_MANY_GATE and self.C.lut_many_node(w)[4] >= 1 and self.rng.random() < 0.5:
                self.free(d, w)


SPECIALS = ["mux-one-wire", "mux-const-select", "mux-over-not-affine", "row-const-inputs", "row-one-wire-x3",
            "row-cancel", "affine-s0", "affine-chain-2^16", "free-chain-depth3"]


def _small(g):
    """about 12 inputs, 30 to 40 bootstraps, depth 4 to 6; the last level holds one row and the one
    before three, so that B = 1 and B = 3 reach both small key-switch kernels"""
    rng = g.rng
    ins = g.C.inputs(int(rng.integers(11, 14)))
    for w in ins:
        g.put(w, 0)
    for _ in range(int(rng.integers(2, 5))):          # level 0: bootstrap-free nodes over inputs
        g.free(0)
    depth = int(rng.integers(4, 7))
    big = depth - 2
    specials = {name: int(rng.integers(1, big + 1)) for name in SPECIALS if rng.random() < 0.6}
    target = int(rng.integers(30, 37)) - 4
    for d in range(1, big + 1):
        for name, at in specials.items():
            if at == d:
                g.special(name, d)
        makers = [g.mux, g.lut, g.gate]               # every level: a MUX beside a table row
        makers.append((lambda dd: g.many(dd, last=depth - 1)) if rng.random() < 0.8 else g.full_add)
        if rng.random() < 0.5:
            makers.append(g.full_add)
        if rng.random() < 0.5:
            makers.append(lambda dd: g.many(dd, last=depth - 1))
        for m in makers:
            m(d)
        while g.n_boot < target * d // big or g.due.get(d):
            [g.gate, g.lincomb, g.lut, g.mux][int(rng.integers(4))](d)
        g.free_on_extras(d)
        for _ in range(int(rng.integers(1, 4))):
            g.free(d)
    for _ in range(3):
        [g.gate, g.lincomb, g.lut][int(rng.integers(3))](depth - 1)
    while g.due.get(depth - 1):
        g.lut(depth - 1)
    g.free(depth - 1)
    g.gate(depth)
    return ins


def _one_level(g, R, last):
    """level 1 of exactly R rows holding every row kind, its last rows a MUX pair (last = "mux") or
    a many-LUT row (last = "many"); inputs only, so that the level's size is known"""
    ins = g.C.inputs(10)
    for w in ins:
        g.put(w, 0)
    g.free(0)
    tail = 2 if last == "mux" else 1
    kinds = [g.gate, g.lincomb, g.mux, g.lut, g.full_add, lambda d: g.many(d, (1, 2)), lambda d: g.many(d, (2, 3)),
             lambda d: g.many(d, (4, 16))]
    assert R >= 9 + tail
    for m in kinds:
        m(1)
    while g.n_boot < R - tail:
        room = R - tail - g.n_boot
        [g.gate, g.lincomb, g.lut, g.full_add, g.mux][int(g.rng.integers(5 if room >= 2 else 4))](1)
    return ins, (g.mux(1) if last == "mux" else g.many(1, (2, 3)))


def _wide(g, R=13):
    ins, _ = _one_level(g, R, "mux")
    return ins


def seam_shape(cus):
    """(R, B) with R B = 4 CUs + 3: the smallest R >= 11 that divides it (all in one instance when
    none does)"""
    total = 4 * cus + 3
    for R in range(11, 200):
        if total % R == 0:
            return R, total // R
    return total, 1


def _seam(g, R, last):
    """one level of R rows; with R B = 4 CUs + 3 slots the second launch starts inside the instances
    of the level's last row.  A small second level reads that row's outputs."""
    ins, w = _one_level(g, R, last)
    g.free(1, w)
    if last == "many":
        g.lut(2, (w, w + 1, w + 2), (1, g.nz_coef(), g.nz_coef()))
        g.mux(2, (w + 2, w, g.pick(2, 1)[0]))
    else:
        g.lut(2, (w, g.pick(2, 1)[0], w), (1, g.nz_coef(), g.nz_coef()))
        g.mux(2, (w, w, g.pick(2, 1)[0]))
    return ins


def make_case(seed, profile, cus=256):
    """-> (Circuit, input wires, features).  profile: "small", "wide" (one level of 13 rows; run
    it at wide_B(cus)) or "seam" (one level of seam_shape(cus)[0] rows and a small second level; run
    it at seam_shape(cus)[1])."""
    g = _Gen(seed)
    if profile == "small":
        ins = _small(g)
    elif profile == "wide":
        ins = _wide(g)
    elif profile == "seam":
        ins = _seam(g, seam_shape(cus)[0], "mux" if seed % 2 else "many")
    else:
        raise KeyError(profile)
    return g.C, ins, features_of(g.C, g.fa)


def wide_B(cus, R=13):
    """rows x B just above one workgroup per CU"""
    return cus // R + 1


def grow(C, seed):
    """three more nodes on a circuit that has run: a MUX, a many-LUT row and an affine node, over
    its last wires"""
    rng = np.random.default_rng(int(seed) + 7)
    n_w = DO.count_wires(C)
    a, b, c = (int(v) for v in rng.choice(np.arange(n_w), 3, replace=False))
    m = C.gate("MUX", a, b, n_w - 1)
    tv = rng.integers(-2**31, 2**31, N, dtype=np.int64).astype(np.int32)
    y = C.lut_many(C.lut_table(tv), 2, 3, int(rng.integers(-2**31, 2**31)), 1, m, -2, c, 3, n_w - 1)
    return [m, y, y + 1, y + 2, C.affine(E8, 3, y + 2)]


def random_inputs(seed, ins, B):
    """uniformly random Torus32 words on every input wire: {wire: (a [B][500], b [B])}"""
    rng = np.random.default_rng([int(seed), int(B)])
    r32 = lambda shape: rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)
    return {w: (r32((B, n_lwe)), r32(B)) for w in ins}
