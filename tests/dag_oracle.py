"""One node-by-node CPU evaluator for every node kind a circuit can hold (TEST INFRASTRUCTURE: the
expected values of tests/test_circuit_fuzz_gpu.py; pinned to the three older evaluators by
tests/test_dag_oracle.py).

tests/circuit_oracle.py evaluates gates and MUX, tests/lut_oracle.py / many_lut_oracle.py /
fa_oracle.py evaluate LUT, many-LUT and affine nodes but no MUX; a circuit that mixes them has no
checker.  This one covers all of them and folds nothing: every wire is materialised as an LWE
sample (a [B][500], b [B]) and every node is computed from the samples of its input wires,
  * input:                 the caller's sample;
  * CONST:                 (0, c0);
  * NOT / COPY:            -W[in], W[in];
  * affine (gate -4):      (0, c0) + s W[in];
  * gate / lincomb row:    KS(woKS_{1/8}((0, c0) + sum_k s_k W[in_k]));
  * MUX:                   KS((0, 1/8) + woKS_{1/8}(-1/8 + a + b) + woKS_{1/8}(-1/8 - a + c));
  * LUT row:               KS(woKS_tv((0, c0) + sum_k s_k W[in_k]))          (lut_oracle);
  * many-LUT row:          all n_out wires from ONE blind rotation           (many_lut_oracle),
in uint32 arithmetic (mod 2^32).  It reads a circuit only through node(), lut_node(),
lut_many_node() and lut_table_get().

Order of evaluation: a wavefront over data readiness.  Each round first computes, in wire order,
every bootstrap-free node whose input is known, then hands the oracle EVERY bootstrapped node whose
inputs are known at once: one threaded woKS call for all gate rows and MUX halves, one LUT call
over a per-sample table index, one many-LUT call per (log_nu, n_out), and one key switch for the
gate and MUX results — so that a batch of B = 1 still fills the thread pool.  Nothing here knows
about levels, rows, merged bases or folded constants: those are the compiler's, and the comparison
checks them."""
import numpy as np

import lut_oracle as LO
import many_lut_oracle as MO
import oracle_ctypes as O

N, n_lwe = O.N, O.n_lwe
E8 = 1 << 29
MUX, NOT, COPY, CONST = 10, 13, 14, 15
LUT_GATE, LUT_MANY_GATE, AFFINE_GATE = -2, -3, -4


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _scale(s, x):
    """s * x mod 2^32 over a sample x = (a, b)"""
    k = np.uint32(int(s) & 0xFFFFFFFF)
    return _u32(x[0]) * k, _u32(x[1]) * k


def _lin(c, terms, B):
    """(0, c) + sum_k s_k X_k mod 2^32 -> int32 sample"""
    a = np.zeros((B, n_lwe), np.uint32)
    b = np.full(B, int(c) & 0xFFFFFFFF, np.uint32)
    for s, x in terms:
        ta, tb = _scale(s, x)
        a = a + ta
        b = b + tb
    return a.view(np.int32), b.view(np.int32)


def count_wires(C):
    """the number of wires, from node() alone"""
    import tfhe_amd as T
    w = 0
    while True:
        try:
            C.node(w)
        except T.TfheAmdError:
            return w
        w += 1


def eval_circuit(C, okey, inputs, B, known=None):
    """C: tfhe_amd.Circuit; inputs: {wire: (a [B][500] int32, b [B] int32)}; returns {wire: (a, b)}
    for every wire.  known: wires already evaluated, whole nodes only (a circuit that grew: only the
    rest is computed)."""
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
        # bootstrap-free nodes in wire order (a chain resolves in one pass), then what is ready
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
            elif all(i in W for i in ins if i >= 0):
                ready.append(w)
            else:
                later.append(w)
        gates, luts, manys = [], [], {}                  # (wire, x ...) jobs of this round
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
            else:
                gates.append((w, [row_input(c0, s, ins)]))
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
                W[w] = (r_a[j * B:(j + 1) * B], r_b[j * B:(j + 1) * B])

        def batch(jobs):
            ids = sorted({t for _, t, _ in jobs})
            tvs = np.stack([table(t) for t in ids])
            idx = np.concatenate([np.full(B, ids.index(t), np.int64) for _, t, _ in jobs])
            return tvs, np.concatenate([x[0] for _, _, x in jobs]), np.concatenate([x[1] for _, _, x in jobs]), idx
        if luts:
            r_a, r_b = LO.bootstrap_batch(okey, *batch(luts))
            for j, (w, _, _) in enumerate(luts):
                W[w] = (r_a[j * B:(j + 1) * B], r_b[j * B:(j + 1) * B])
        for (theta, n_out), jobs in manys.items():
            tvs, x_a, x_b, idx = batch(jobs)
            r_a, r_b = MO.bootstrap_batch(okey, tvs, x_a, x_b, theta, n_out, idx)
            for j, (w, _, _) in enumerate(jobs):
                for f in range(n_out):
                    W[w + f] = (r_a[f, j * B:(j + 1) * B], r_b[f, j * B:(j + 1) * B])
        later = [w for w in later if w not in W]
        assert len(later) < len(todo), f"no progress: wires {later[:8]} wait for inputs that never come"
        todo = later
    return W
