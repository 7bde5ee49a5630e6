"""The node-by-node CPU evaluator of tests/dag_oracle.py with the select node added (TEST
INFRASTRUCTURE: the expected values of tests/test_circuit_select.py and
tests/test_circuit_select_gpu.py; pinned to dag_oracle.eval_circuit word for word on a select-free
circuit by tests/test_circuit_select.py).

Every wire is materialised as an LWE sample (a [B][500], b [B]) and every node is computed from the
samples of its input wires.  The node kinds of dag_oracle are evaluated as there (the same oracle
calls on the same operands); a select node (gate -5) is

    W = acc_oracle.select(candidates as written to their wires, (0, c0) + s W[sel])
      = KS(woKS from the accumulator box_fill(pack(candidate m at coefficient m N / p)))

on the materialised candidate and selector samples: nothing is folded, so the comparison checks the
compiler's folding of the selector, its levelling, the grouping by p and the gather.  The circuit is
read only through node(), lut_node(), lut_many_node(), lut_table_get() and select_node().

Order of evaluation: the wavefront over data readiness of dag_oracle; the select nodes that are
ready in a round go to the oracle together, one call per p (the packing key is converted once per
call, and the blind rotations fill the thread pool)."""
import numpy as np

import acc_oracle as AO
import dag_oracle as DO
import lut_oracle as LO
import many_lut_oracle as MO
import oracle_ctypes as O

N, n_lwe = O.N, O.n_lwe
E8 = DO.E8
MUX, NOT, COPY, CONST = DO.MUX, DO.NOT, DO.COPY, DO.CONST
LUT_GATE, LUT_MANY_GATE, AFFINE_GATE = DO.LUT_GATE, DO.LUT_MANY_GATE, DO.AFFINE_GATE
SELECT_GATE = -5

_u32, _lin, count_wires = DO._u32, DO._lin, DO.count_wires


def select_wires(C, w):
    """(p, candidate wires, c0, s, selector wire) of the select node w"""
    kind, gate, c0, s, ins = C.node(w)
    assert kind == 1 and gate == SELECT_GATE, (w, kind, gate)
    p, cand, c0n = C.select_node(w)
    assert c0n == c0 and len(cand) == p and ins[1] == ins[2] == -1, (w, c0, c0n, cand, ins)
    return p, cand, c0, s[0], ins[0]


def eval_selects(okey, pack_key, jobs, B):
    """Select nodes of one p, each job (candidate samples [(a, b)] * p, c0, s, selector sample), as ONE
    call of acc_oracle.select's two halves over the nodes' instances side by side: packed_boxes on the
    candidates [p][n B], bootstrap_batch of accumulator i by selector i.  (acc_oracle.select itself
    takes one (c, sa) per call; its selector (0, c) + sa Y is formed here per node with the same
    lut_oracle.lin.)  -> [(r_a [B][500], r_b [B])] per job"""
    p = len(jobs[0][0])
    cand_a = np.stack([np.concatenate([np.asarray(c[m][0], dtype=np.int32) for c, _, _, _ in jobs]) for m in range(p)])
    cand_b = np.stack([np.concatenate([np.asarray(c[m][1], dtype=np.int32) for c, _, _, _ in jobs]) for m in range(p)])
    xs = [LO.lin(int(c0), [(int(s), (sel[0], sel[1]))], B) for _, c0, s, sel in jobs]
    r_a, r_b = AO.bootstrap_batch(okey, AO.packed_boxes(pack_key, cand_a, cand_b), np.concatenate([x[0] for x in xs]),
                                  np.concatenate([x[1] for x in xs]))
    return [(r_a[j * B:(j + 1) * B], r_b[j * B:(j + 1) * B]) for j in range(len(jobs))]


def eval_circuit(C, okey, inputs, B, pack_key=None, known=None):
    """C: tfhe_amd.Circuit; inputs: {wire: (a [B][500] int32, b [B] int32)}; pack_key: the packing
    key's coefficients (SecretKeyset.pack_key()), needed if C holds a select node; returns
    {wire: (a, b)} for every wire.  known: wires already evaluated, whole nodes only."""
    n_w = count_wires(C)
    nodes = [C.node(w) for w in range(n_w)]
    W = dict(known or {})
    todo = [w for w in range(n_w) if w not in W]
    tables = {}

    def table(t):
        if t not in tables:
            tables[t] = C.lut_table_get(t)
        return tables[t]

    def row_input(c0, s, ins):
        return _lin(c0, [(s[k], W[ins[k]]) for k in range(3) if ins[k] >= 0], B)

    while todo:
        ready, later = [], []
        for w in todo:
            kind, gate, c0, s, ins = nodes[w]
            if w in W:                                   # a further wire of a many-LUT node
                continue
            if kind == 0:
                W[w] = tuple(np.ascontiguousarray(np.asarray(v, dtype=np.int32)) for v in inputs[w])
            elif kind == 2:
                if gate == CONST:
                    W[w] = _lin(c0, [], B)
                elif ins[0] not in W:
                    later.append(w)
                elif gate == AFFINE_GATE:
                    W[w] = _lin(c0, [(s[0], W[ins[0]])], B)
                elif gate == NOT:
                    W[w] = _lin(0, [(-1, W[ins[0]])], B)
                else:
                    assert gate == COPY, (w, gate)
                    W[w] = (W[ins[0]][0].copy(), W[ins[0]][1].copy())
            elif gate == LUT_MANY_GATE and C.lut_many_node(w)[4] > 0:
                later.append(w)                          # filled with the node's first wire
            elif gate == SELECT_GATE:
                p, cand, _, _, sel = select_wires(C, w)
                (ready if sel in W and all(c in W for c in cand) else later).append(w)
            elif all(i in W for i in ins if i >= 0):
                ready.append(w)
            else:
                later.append(w)
        gates, luts, manys, selects = [], [], {}, []     # (wire, x ...) jobs of this round
        for w in ready:
            kind, gate, c0, s, ins = nodes[w]
            if gate == MUX:
                a, b, c = (W[i] for i in ins)
                gates.append((w, [_lin(-E8, [(1, a), (1, b)], B), _lin(-E8, [(-1, a), (1, c)], B)]))
            elif gate == LUT_GATE:
                t, c0 = C.lut_node(w)
                luts.append((w, t, row_input(c0, s, ins)))
            elif gate == LUT_MANY_GATE:
                t, c0, theta, n_out, index = C.lut_many_node(w)
                assert index == 0
                manys.setdefault((theta, n_out), []).append((w, t, row_input(c0, s, ins)))
            elif gate == SELECT_GATE:
                selects.append(w)
            else:
                gates.append((w, [row_input(c0, s, ins)]))
        out = {}                                         # this round's results: they read the round's start
        if gates:
            xs = [x for _, rows in gates for x in rows]
            u_a, u_b = okey.woks_batch(E8, np.concatenate([x[0] for x in xs]), np.concatenate([x[1] for x in xs]))
            k_a, k_b, r = [], [], 0
            for w, rows in gates:
                a, b = _u32(u_a[r * B:(r + 1) * B]), _u32(u_b[r * B:(r + 1) * B])
                if len(rows) == 2:                       # MUX: (0, 1/8) + u1 + u2
                    a = a + _u32(u_a[(r + 1) * B:(r + 2) * B])
                    b = b + _u32(u_b[(r + 1) * B:(r + 2) * B]) + np.uint32(E8)
                k_a.append(a.view(np.int32))
                k_b.append(b.view(np.int32))
                r += len(rows)
            r_a, r_b = okey.keyswitch_batch(np.concatenate(k_a), np.concatenate(k_b))
            for j, (w, _) in enumerate(gates):
                out[w] = (r_a[j * B:(j + 1) * B], r_b[j * B:(j + 1) * B])

        def batch(jobs):
            ids = sorted({t for _, t, _ in jobs})
            tvs = np.stack([table(t) for t in ids])
            idx = np.concatenate([np.full(B, ids.index(t), np.int64) for _, t, _ in jobs])
            return tvs, np.concatenate([x[0] for _, _, x in jobs]), np.concatenate([x[1] for _, _, x in jobs]), idx
        if luts:
            r_a, r_b = LO.bootstrap_batch(okey, *batch(luts))
            for j, (w, _, _) in enumerate(luts):
                out[w] = (r_a[j * B:(j + 1) * B], r_b[j * B:(j + 1) * B])
        for (theta, n_out), jobs in manys.items():
            tvs, x_a, x_b, idx = batch(jobs)
            r_a, r_b = MO.bootstrap_batch(okey, tvs, x_a, x_b, theta, n_out, idx)
            for j, (w, _, _) in enumerate(jobs):
                for f in range(n_out):
                    out[w + f] = (r_a[f, j * B:(j + 1) * B], r_b[f, j * B:(j + 1) * B])
        by_p = {}
        for w in selects:
            assert pack_key is not None, f"wire {w} is a select node: the evaluator needs the packing key"
            p, cand, c0, s, sel = select_wires(C, w)
            by_p.setdefault(p, []).append((w, ([W[c] for c in cand], c0, s, W[sel])))
        for p, jobs in by_p.items():
            for (w, _), r in zip(jobs, eval_selects(okey, pack_key, [j for _, j in jobs], B)):
                out[w] = r
        W.update(out)
        later = [w for w in later if w not in W]
        assert len(later) < len(todo), f"no progress: wires {later[:8]} wait for inputs that never come"
        todo = later
    return W


def mixed_circuit(seed=11):
    """gate rows, a MUX, a LUT row, a many-LUT row and select rows of p = 2, 4, 2 in one level, and a
    second level that reads the select outputs as a selector, as a candidate and through NOT / affine;
    uniformly random tables -> (Circuit, input wires, the select wires)"""
    rng = np.random.default_rng(seed)
    word = lambda: int(rng.integers(-2**31, 2**31))
    tv = lambda: rng.integers(-2**31, 2**31, 1024, dtype=np.int64).astype(np.int32)
    import tfhe_amd as T
    C = T.Circuit()
    ins = C.inputs(8)
    a, b, c, d, e, f, g, h = ins
    g1 = C.gate("NAND", a, b)
    g2 = C.gate("XOR3", a, c, d)
    m = C.gate("MUX", a, b, c)
    lu = C.lut(C.lut_table(tv()), word(), 1, d, 3, e)
    my = C.lut_many(C.lut_table(tv()), 2, 3, word(), 1, f, -2, g)
    s2 = C.select([a, h], b, c0=1 << 30)
    s4 = C.select([c, C.gate("NOT", d), e, C.affine(word(), 3, f)], C.affine(word(), 2, g), c0=word(), s=-1)
    s2b = C.select([h, g], C.gate("COPY", a), c0=word(), s=word())
    sels = [s2, s4, s2b]
    # level 2
    t1 = C.select([g1, s2, my + 1, m], s4, c0=word())                        # a select output as selector and candidate
    t2 = C.select([C.gate("NOT", s4), C.affine(word(), -3, s2b)], C.affine(word(), 5, s2), c0=word())
    t3 = C.gate("NAND", s2, C.gate("NOT", s4))
    t4 = C.lut(C.lut_table(tv()), word(), 1, s2b, 1, lu, 1, g2)
    return C, ins, sels + [t1, t2], [t3, t4]


_lut2 = {}


def lut2_case(keyset, okey, B=32, seed=3909):
    """The lut2 decode case of tests/test_circuit_select.py, all on the oracle, once per process: two
    fresh p = 4 digit batches x, y at the key-switch noise, a random table f[y][x] in [0, 4), the
    circuit lut2(lut_encode(f), x, y) and every wire of it under acc_oracle.chain_pack_key.  -> dict"""
    import tfhe_amd as T
    if "case" not in _lut2:
        rng = np.random.default_rng(seed)
        x, y = rng.integers(0, 4, B), rng.integers(0, 4, B)
        f = rng.integers(0, 4, (4, 4))                   # f[j][m]: the value at y = j, x = m
        C = T.Circuit()
        wx, wy = C.inputs(2)
        out = C.lut2(T.lut_encode(f.reshape(-1), 4), wx, wy)
        enc = {wx: keyset.encrypt_digits(x, 4, rng), wy: keyset.encrypt_digits(y, 4, rng)}
        key = AO.chain_pack_key(keyset)
        W = eval_circuit(C, okey, enc, B, pack_key=key)
        _lut2["case"] = dict(B=B, x=x, y=y, f=f, C=C, enc=enc, key=key, W=W, many=wy + 1, out=out)
    return _lut2["case"]
