"""Seeded random call SEQUENCES for the differential fuzz of what lies between the library's calls
(TEST INFRASTRUCTURE: tests/test_seq_fuzz.py checks the generator without a GPU,
tests/test_seq_fuzz_gpu.py runs the programs against the oracles the per-feature tests use).

make_program(seed, start_kernel) builds a program from np.random.default_rng(seed) alone: a dict
(seed, start_kernel, steps) of plain ints, strings, tuples and dicts, the same in every process.  A
step is a CALL of one device or host entry point, placed on a context ("A": the session's, "B": a
second one on the same device; pack key, TGSW set and automaton are shared by both), on a stream
(0: the context's own, 1 .. 3: three torch streams) and with inputs that are fresh data or the
output of an earlier call (same stream: stream order alone; another stream: behind an event the
runner records and waits on), or a STATE step: reserve, the two process-wide switches flipped and
put back, guard_stats(reset), ctx.sync(), an object destroyed and imported again, a third context
created and destroyed.  Batch sizes are 1 .. 5; at most two steps of a program sit at a threshold
("rot": CUs + 1 gates, the register / paired rotation and the context's scratch regrown; "ks": 13
key switches, a split form), their inputs tiled from 5 distinct rows.

features_of(program) names what a program contains by simulating it step by step (which streams
still have work in flight, which owner of device scratch was used last from where, what each
scratch holds), never by what the generator meant to build.  The owners and their growth rules are
those of engine.cpp tfhe_amd_reserve (64 2^k slots), pack.cpp / acc.cpp / circuit_select.cpp (digit
and accumulator outputs), tgsw.cpp (tree words), tgsw_dfa.cpp (state words), circuit.cpp (u slots).

run_program(program, ...) is the checker: every call alone first (synchronised, on the session
context and objects of its own: the kernels it names), then the program as written, ONE
torch.cuda.synchronize(), and then every output word of every call against the oracle, every guard
band, every input, the recomputed count and the kernel names (its docstring).

Adding a seed: append it to SEEDS (test_seq_fuzz.py tells which features the list then covers); a
seed that once failed stays in the list."""
import time

import numpy as np

N, n_lwe = 1024, 500
COUNT = 24                        # TGSW samples of the pool
NOMINAL_CUS = 256

# Measured on an MI355X (256 CUs, 16 host threads), oracle included: test_program 0.8 .. 2.6 s (the slowest:
# seed 75, of which the oracle is 2.5 s, the solo runs 0.04 s and the program 0.04 s); the other two forms
# reuse the seed's oracle results and take 0.07 .. 0.18 s each.
SEEDS = [13, 75, 78, 144, 211, 291]      # 78, 144 and 211 alone cover FEATURES; every feature is in two seeds
SKEW_SEEDS = [144, 291]           # run a second time with word-aligned arenas: both chain kinds, and a key switch
                                  # that reads a woKS output (whose u_a keeps its 16 bytes)
STEPS = 25

GATES2 = ["NAND", "OR", "AND", "XOR", "XNOR", "NOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
OWNERS = ("context", "pack", "tgsw", "dfa", "circuit")
OBJECTS = ("pack", "tgsw", "dfa", "circuit")

# kind -> (owners whose fence the call takes, objects it uses, chain type it can read, chain type it
# writes, host form, has a key switch behind a context-scratch rotation)
_K = {}


def _kind(name, owners=(), objects=(), cin=None, cout=None, host=False, ctx_ks=False):
    _K[name] = dict(owners=tuple(owners), objects=tuple(objects), cin=cin, cout=cout, host=host, ctx_ks=ctx_ks)


_kind("gate", ["context"], cin="lwe", cout="lwe", ctx_ks=True)
_kind("mux", ["context"], cin="lwe", cout="lwe", ctx_ks=True)
_kind("gate_host", ["context"], host=True, ctx_ks=True)
_kind("mixed_host", ["context"], host=True, ctx_ks=True)
_kind("woks", ["context"], cin="lwe", cout="ext")
_kind("bootstrap", ["context"], cin="lwe", cout="lwe", ctx_ks=True)
_kind("keyswitch", [], cin="ext", cout="lwe")
_kind("lut_woks", ["context"], cin="lwe", cout="ext")
_kind("lut_boot", ["context"], cin="lwe", cout="lwe", ctx_ks=True)
_kind("many_woks", ["context"], cin="lwe")
_kind("many_boot", ["context"], cin="lwe", ctx_ks=True)
_kind("full_add", ["context"], cin="lwe", ctx_ks=True)
_kind("acc_woks", ["context"], cin="tlwe", cout="ext")
_kind("acc_boot", ["context"], cin="tlwe", cout="lwe", ctx_ks=True)
_kind("select", ["context", "pack"], ["pack"], cout="lwe", ctx_ks=True)
_kind("lookup", ["context"], ["tgsw"], ctx_ks=True)
_kind("lookup_woks", [], ["tgsw"])
_kind("lookup_tree", ["context", "tgsw"], ["tgsw"], ctx_ks=True)
_kind("lookup_tree_woks", ["tgsw"], ["tgsw"])
_kind("cmux", [], ["tgsw"], cin="tlwe", cout="tlwe")
_kind("dfa", ["context", "dfa"], ["tgsw", "dfa"], ctx_ks=True)
_kind("dfa_woks", ["dfa"], ["tgsw", "dfa"])
_kind("pack", ["pack"], ["pack"], cout="tlwe")
_kind("box_fill", [], cin="tlwe", cout="tlwe")
_kind("circuit", ["circuit"], ["circuit"])
_kind("select_circuit", ["circuit", "pack"], ["pack", "select_circuit"])

CALL_KINDS = tuple(_K)
WOKS_LOOKUPS = ("lookup_woks", "lookup_tree_woks")
STATE_OPS = ("reserve", "guard_flip", "guard_back", "kernel_flip", "kernel_back", "guard_stats", "sync", "reimport",
             "ctx_cycle")

FEATURES = tuple(
    [f"kind:{k}" for k in CALL_KINDS] +
    [f"two-streams:{o}" for o in OWNERS] +          # an owner used from two streams back to back, no host sync
    [f"regrow:{o}" for o in OWNERS] +               # an owner regrown while another stream is in flight
    [f"reimport:{o}" for o in OBJECTS] +            # an object destroyed and imported again with its work in flight
    ["toggle:guard", "toggle:kernel",               # a switch flipped between two unsynchronised calls
     "chain:same-stream", "chain:cross-stream",
     "host-between-dev",                            # a host form between two device forms on one context
     "pack-key-three-streams",                      # select_dev, a select circuit and pack_dev on three streams
     "object-two-contexts",                         # one object used by both contexts, no sync between
     "woks-lookup-next-to-ks",                      # the woKS lookup (no context fence) next to a key-switched call
     "threshold:rot", "threshold:ks"])


def resolve_B(B, cus=NOMINAL_CUS):
    return cus + 1 if B == "rot" else 13 if B == "ks" else int(B)


# ---------------------------------------------------------------- the generator

class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.steps = []
        self.thresholds = 0

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def streams(self, k):
        """k distinct streams, at most one of them the context's own"""
        return [int(s) for s in self.rng.permutation(4)[:k]]

    def ctx(self):
        return "A" if self.rng.random() < 0.55 else "B"

    def params(self, kind):
        r = self.rng
        if kind in ("gate", "gate_host"):
            return {"gate": self.pick(GATES2)}
        if kind == "mixed_host":
            return {"mux_every": int(r.integers(2, 4))}
        if kind in ("many_woks", "many_boot"):
            return dict(zip(("log_nu", "n_out"), self.pick([(1, 2), (2, 3)])))
        if kind == "full_add":
            return {"third": int(r.integers(0, 2))}
        if kind in ("acc_woks", "acc_boot"):
            return {"n_acc": 2}
        if kind == "select":
            return {"p": self.pick([2, 4])}
        if kind in ("lookup", "lookup_woks"):
            return {"d": int(r.integers(1, 3)), "n_poly": 1, "log_stride": 1, "n_out": int(r.integers(1, 3))}
        if kind in ("lookup_tree", "lookup_tree_woks"):
            return {"d": 2, "n_poly": self.pick([2, 4]), "log_stride": 0, "n_out": 1}
        if kind in ("dfa", "dfa_woks"):
            return {"len": int(r.integers(2, 4)), "n_out": int(r.integers(1, 3))}
        if kind == "pack":
            return {"P": int(r.integers(1, 4))}
        if kind == "box_fill":
            return {"log_w": int(r.integers(0, 11))}
        if kind == "cmux":
            return {"d0": int(r.integers(0, 2))}
        return {}

    def call(self, kind, B=None, ctx=None, stream=None, chain=None, **over):
        """chain: None, or (producer step, "same" | "cross")"""
        P = self.params(kind)
        P.update(over)
        ctx = self.ctx() if ctx is None else ctx
        stream = int(self.rng.integers(0, 4)) if stream is None else stream
        if B is None:
            B = int(self.rng.integers(1, 3)) if kind in ("select_circuit", "circuit") else int(self.rng.integers(1, 6))
        inputs = None
        if chain is not None:
            src, mode = chain
            p = self.steps[src]
            assert _K[p["kind"]]["cout"] == _K[kind]["cin"] and not isinstance(p["B"], str)
            B = p["B"]
            if kind in ("acc_woks", "acc_boot"):
                P["n_acc"] = p["B"]
                B = int(self.rng.integers(1, 6))
            if mode == "same":
                ctx, stream = (p["ctx"], p["stream"]) if p["stream"] == 0 else (ctx, p["stream"])
            else:
                stream = self.pick([s for s in range(4) if s != p["stream"]])
            inputs = (src, mode)
        if isinstance(B, str):
            self.thresholds += 1
        if _K[kind]["host"]:
            stream = 0
        self.steps.append({"step": "call", "kind": kind, "B": B, "ctx": ctx, "stream": stream, "P": P, "chain": inputs})
        return len(self.steps) - 1

    def state(self, op, **kw):
        self.steps.append(dict({"step": "state", "op": op}, **kw))

    # ---- motifs: short sequences; features_of decides afterwards what they amount to
    def m_regrow(self, owner):
        """small, larger (the owner grows with the first still in flight), small again on a third
        stream (no growth: the fence alone orders it behind the second)"""
        s1, s2, s3 = self.streams(3)
        if owner == "context":
            if self.thresholds >= 2:
                return
            small = ["gate", "bootstrap", "lut_boot", "woks"]
            self.call(self.pick(small), B=2, ctx="B", stream=s1)
            self.call(self.pick(["gate", "mux"]), B="rot", ctx="B", stream=s2)
            self.call(self.pick(small), B=3, ctx="B", stream=s3)
        elif owner == "pack":
            k = self.pick(["select", "pack"])
            self.call(k, B=1, stream=s1)
            self.call(k, B=4, stream=s2)
            self.call(k, B=2, stream=s3)
        elif owner == "tgsw":
            kinds = ["lookup_tree", "lookup_tree_woks"]
            self.call(self.pick(kinds), B=1, stream=s1, n_poly=2)
            self.call(self.pick(kinds), B=3, stream=s2, n_poly=4)
            self.call(self.pick(kinds), B=2, stream=s3, n_poly=2)
        elif owner == "dfa":
            kinds = ["dfa", "dfa_woks"]
            self.call(self.pick(kinds), B=1, stream=s1)
            self.call(self.pick(kinds), B=4, stream=s2)
            self.call(self.pick(kinds), B=2, stream=s3)
        else:
            c = self.ctx()
            self.call("circuit", B=1, ctx=c, stream=s1)
            self.call("circuit", B=3, ctx=c, stream=s2)
            self.call("circuit", B=2, ctx=c, stream=s3)

    def m_reimport(self, obj):
        kinds = [k for k in CALL_KINDS if obj in _K[k]["objects"]]
        self.call(self.pick(kinds), stream=self.pick([1, 2, 3]))
        self.state("reimport", obj=obj)
        self.call(self.pick(kinds))

    def m_toggle(self, switch):
        rot = ["gate", "mux", "bootstrap", "lut_boot", "many_boot", "full_add", "acc_boot", "woks"]
        s1, s2 = self.streams(2)
        self.call(self.pick(rot), stream=s1)
        self.state(switch + "_flip")
        self.call(self.pick(rot), stream=s2)
        if self.rng.random() < 0.5:
            self.call(self.pick(rot))
        self.state(switch + "_back")

    def m_host_between(self):
        c = self.ctx()
        dev = ["gate", "mux", "bootstrap", "lut_woks", "many_boot", "acc_woks", "lookup"]
        self.call(self.pick(dev), ctx=c, stream=self.pick([1, 2, 3]))
        self.call(self.pick(["gate_host", "mixed_host"]), ctx=c)
        self.call(self.pick(dev), ctx=c)

    def m_pack3(self):
        self.call("select", B=5)                             # the key's scratch large enough for the three below
        s = self.streams(3)
        for kind, st in zip([str(k) for k in self.rng.permutation(["select", "select_circuit", "pack"])], s):
            self.call(kind, stream=st, B=1 if kind == "select_circuit" else int(self.rng.integers(1, 4)))

    def m_two_ctx(self):
        obj = self.pick(["pack", "tgsw", "dfa"])
        kinds = [k for k in CALL_KINDS if obj in _K[k]["objects"] and k != "select_circuit"]
        s1, s2 = self.streams(2)
        kind = self.pick(kinds)
        first = self.steps[self.call(kind, ctx="A", stream=s1)]
        self.call(kind, B=first["B"], ctx="B", stream=s2, **first["P"])       # the same shape: nothing grows between them

    def m_woks_next(self):
        c = self.ctx()
        s1, s2 = self.streams(2)
        pair = [(self.pick(list(WOKS_LOOKUPS)), s1), (self.pick(["gate", "bootstrap", "lookup", "lut_boot"]), s2)]
        for k in self.rng.permutation(2):
            self.call(pair[int(k)][0], ctx=c, stream=pair[int(k)][1])

    def m_chain(self, mode):
        t = self.pick(["lwe", "ext", "tlwe"])
        prod = self.pick([k for k in CALL_KINDS if _K[k]["cout"] == t])
        cons = self.pick([k for k in CALL_KINDS if _K[k]["cin"] == t])
        src = self.call(prod)
        self.call(cons, chain=(src, mode))
        if self.rng.random() < 0.4 and _K[cons]["cout"] is not None:        # a chain of three
            nxt = [k for k in CALL_KINDS if _K[k]["cin"] == _K[cons]["cout"]]
            self.call(self.pick(nxt), chain=(len(self.steps) - 1, self.pick(["same", "cross"])))

    def m_threshold_ks(self):
        if self.thresholds < 2:
            self.call("keyswitch", B="ks")

    def m_filler(self, deck):
        op = self.pick(["sync", "guard_stats", "reserve", "ctx_cycle", None, None])
        if op == "reserve":
            self.state("reserve", ctx=self.ctx(), B=self.pick([16, 100, "rot"]))
        elif op in ("sync", "guard_stats"):
            self.state(op, ctx=self.ctx())
        elif op == "ctx_cycle":
            self.state("ctx_cycle")
        if deck:
            self.call(deck.pop())


def make_program(seed, start_kernel=0, steps=STEPS):
    g = _Gen(seed)
    motifs = [("regrow", o) for o in OWNERS] + [("reimport", o) for o in OBJECTS] + \
             [("toggle", "guard"), ("toggle", "kernel"), ("host_between",), ("pack3",), ("two_ctx",), ("woks_next",),
              ("chain", "same"), ("chain", "cross"), ("threshold_ks",)]
    order = [motifs[int(i)] for i in g.rng.permutation(len(motifs))]
    deck = [CALL_KINDS[int(i)] for i in g.rng.permutation(len(CALL_KINDS))]
    while len(g.steps) < steps:
        if order and g.rng.random() < 0.8:
            m = order.pop()
            getattr(g, "m_" + m[0])(*m[1:])
        else:
            used = {s["kind"] for s in g.steps if s["step"] == "call"}
            deck = [k for k in deck if k not in used]
            g.m_filler(deck)
    return {"seed": int(seed), "start_kernel": int(start_kernel), "steps": g.steps}


# ---------------------------------------------------------------- what a program contains

def _need(kind, B, P):
    """{scratch: size in the owner's own unit} the call asks of each owner it takes"""
    out = {}
    n_out = P.get("n_out", 1)
    if "context" in _K[kind]["owners"]:
        out["context"] = B * (n_out if kind in ("many_woks", "many_boot", "lookup", "lookup_tree", "dfa") else
                              2 if kind == "full_add" else 1)
    if kind == "pack":
        out["pack.dig"] = B
    elif kind == "select":
        out["pack.dig"] = out["pack.acc"] = B
    elif kind == "select_circuit":
        out["pack.dig"] = out["pack.acc"] = 3 * B            # mixed_circuit: three select rows in its first level
    if kind in ("lookup_tree", "lookup_tree_woks"):
        out["tgsw"] = 3 * B * P["n_poly"]
    if kind in ("dfa", "dfa_woks"):
        out["dfa"] = B
    if kind in ("circuit", "select_circuit"):
        out["circuit"] = B
    return out


def _ctx_cap(need, cap):
    if need <= cap:
        return cap
    cap = cap or 64
    while cap < need:
        cap *= 2
    return cap


def stream_key(step):
    return ("own", step["ctx"]) if step["stream"] == 0 else ("t", step["stream"])


def features_of(program, cus=NOMINAL_CUS):
    F = set()
    steps = program["steps"]
    inflight = {}                    # stream key -> [call steps enqueued since that stream was last known idle]
    cap = {("context", "A"): float("inf"), ("context", "B"): 64}
    last_user = {}                   # owner instance -> (step, stream key)
    obj_user = {}                    # object -> [(step, ctx)] of its unsynchronised users
    pack_users = {}                  # kind -> stream key, since the last device-wide synchronisation
    pending = None                   # (switch, the call in flight when it was flipped)
    prev_call = None                 # the previous call step, None behind a device-wide synchronisation
    ctx_calls = {"A": [], "B": []}   # per context: (step, is host, in flight on a caller stream) since a device sync

    def flying(i):
        return any(i in v for v in inflight.values())

    def device_sync():
        nonlocal prev_call, pending
        inflight.clear(); obj_user.clear(); pack_users.clear()
        ctx_calls["A"].clear(); ctx_calls["B"].clear()
        prev_call, pending = None, None

    for i, s in enumerate(steps):
        if s["step"] == "state":
            op = s["op"]
            if op == "sync":
                inflight.pop(("own", s["ctx"]), None)
            elif op == "reserve":
                key = ("context", s["ctx"])
                need = resolve_B(s["B"], cus)
                if need > cap[key]:
                    if inflight:
                        F.add("regrow:context")
                    cap[key] = _ctx_cap(need, cap[key])
                    device_sync()
            elif op in ("guard_flip", "kernel_flip", "guard_back", "kernel_back"):
                if prev_call is not None and flying(prev_call):
                    pending = (op.split("_")[0], prev_call)
            elif op == "reimport":
                if any(flying(j) for j, _ in obj_user.get(s["obj"], [])):
                    F.add(f"reimport:{s['obj']}")
                for key in [k for k in cap if (k[0] == s["obj"] and (k[0] != "circuit" or k[1] == "circuit"))
                            or k[0].startswith(s["obj"] + ".")]:
                    del cap[key]                             # the new object starts without scratch
                device_sync()
            else:                    # guard_stats, ctx_cycle: the device is synchronised
                device_sync()
            continue
        kind, P, c = s["kind"], s["P"], s["ctx"]
        B = resolve_B(s["B"], cus)
        sk = stream_key(s)
        F.add(f"kind:{kind}")
        if isinstance(s["B"], str):
            F.add(f"threshold:{s['B']}")
        if s["chain"] is not None:
            F.add("chain:same-stream" if stream_key(steps[s["chain"][0]]) == sk else "chain:cross-stream")
        if pending is not None and flying(pending[1]):
            F.add(f"toggle:{pending[0]}")
        pending = None
        # growth first (it synchronises the device), then the fences
        for what, need in _need(kind, B, P).items():
            owner = what.split(".")[0]
            key = (what, c) if owner in ("context", "circuit") else (what,)
            if owner == "circuit":
                key = (what, kind, c)
            have = cap.get(key, 0)
            if need > have:
                if have > 0 and any(k != sk for k in inflight):
                    F.add(f"regrow:{owner}")
                cap[key] = _ctx_cap(need, have) if owner == "context" else need
                device_sync()                                # every growth path synchronises the device first
        for owner in _K[kind]["owners"]:
            key = (owner, c) if owner == "context" else (owner, kind, c) if owner == "circuit" else (owner,)
            if key in last_user and last_user[key][1] != sk and flying(last_user[key][0]):
                F.add(f"two-streams:{owner}")
            last_user[key] = (i, sk)
        for obj in _K[kind]["objects"]:
            if any(cc != c and flying(j) for j, cc in obj_user.get(obj, [])):
                F.add("object-two-contexts")
            obj_user.setdefault(obj, []).append((i, c))
        if kind in ("select", "select_circuit", "pack"):
            pack_users[kind] = sk
            if len(pack_users) == 3 and len(set(pack_users.values())) == 3:
                F.add("pack-key-three-streams")
        if prev_call is not None:
            p = steps[prev_call]
            if p["ctx"] == c and stream_key(p) != sk and flying(prev_call):
                a, b = p["kind"], kind
                if (a in WOKS_LOOKUPS and _K[b]["ctx_ks"]) or (b in WOKS_LOOKUPS and _K[a]["ctx_ks"]):
                    F.add("woks-lookup-next-to-ks")
        seq = ctx_calls[c]
        if not _K[kind]["host"] and len(seq) >= 2 and seq[-1][1] and not seq[-2][1] and seq[-2][2]:
            F.add("host-between-dev")
        seq.append((i, _K[kind]["host"], sk[0] == "t"))
        inflight.setdefault(sk, []).append(i)
        if _K[kind]["host"]:         # a host form returns with the context's own stream idle
            inflight.pop(("own", c), None)
        prev_call = i
    return F


def summary(program):
    """one line per step, for a failing test's message"""
    out = []
    for i, s in enumerate(program["steps"]):
        if s["step"] == "state":
            out.append(f"{i:2d} state {s['op']} " + " ".join(f"{k}={v}" for k, v in s.items() if k not in ("step", "op")))
        else:
            out.append(f"{i:2d} call  {s['kind']} B={s['B']} ctx={s['ctx']} stream={s['stream']} {s['P']}"
                       + (f" <- step {s['chain'][0]} ({s['chain'][1]})" if s["chain"] else ""))
    return "\n".join(out)


# ---------------------------------------------------------------- data, calls and oracles of the kinds

def _rand32(rng, shape):
    return rng.integers(-2**31, 2**31, shape, dtype=np.int64).astype(np.int32)


def automaton():
    """Q = 5 (tests/test_write_discipline_gpu.py): a branching start state, a copy state, a self-loop
    and a state nothing leads to -> (next [5][2], start)"""
    return np.array([[1, 2], [3, 3], [2, 0], [0, 1], [3, 2]], np.int32), 0


def small_circuit():
    """one level: three gate rows, a MUX, a CONST, a NOT, an affine node and a wire nobody reads"""
    import tfhe_amd as T
    C = T.Circuit()
    a, b, c = ins = C.inputs(3)
    one = C.gate("CONST", 1)
    nb = C.gate("NOT", b)
    af = C.affine(0x12345678, -3, c)
    C.gate("NAND", a, nb), C.gate("XOR", a, one), C.gate("OR", b, c)
    C.gate("MUX", a, b, c)
    C.gate("COPY", af)
    return C, list(ins)


def select_circuit():
    import select_dag_oracle as SO
    C, ins, _, _ = SO.mixed_circuit()
    return C, list(ins)


CHAIN_IN = {"gate": ("ca_a", "ca_b"), "mux": ("ca_a", "ca_b"), "woks": ("x_a", "x_b"), "bootstrap": ("x_a", "x_b"),
            "keyswitch": ("u_a", "u_b"), "lut_woks": ("x_a", "x_b"), "lut_boot": ("x_a", "x_b"),
            "many_woks": ("x_a", "x_b"), "many_boot": ("x_a", "x_b"), "full_add": ("a_a", "a_b"),
            "acc_woks": ("acc",), "acc_boot": ("acc",), "cmux": ("d1",), "box_fill": ("tlwe",)}
CHAIN_OUT = {"lwe": ("res_a", "res_b"), "ext": ("u_a", "u_b"), "tlwe": ("out",)}
ROWWISE = ("gate", "mux", "keyswitch")           # the kinds a threshold step may take: every array is [B][...]


def chain_shapes(kind, B, P):
    """the shapes of the slots a chained input replaces (the solo run's stand-ins)"""
    t = _K[kind]["cin"]
    if t == "lwe":
        return [(B, n_lwe), (B,)]
    if t == "ext":
        return [(B, N), (B,)]
    return [(P["n_acc"] if kind.startswith("acc") else B, 2, N)]


def fresh_inputs(kind, B, P, rng, keyset, circuits, chained):
    """[(name, host array)] in the order the arena holds them; `chained`: leave the chained slots out"""
    lwe = lambda: [_rand32(rng, (B, n_lwe)), _rand32(rng, B)]
    h = []
    if kind in ("gate", "gate_host", "mux", "mixed_host"):
        nin = 3 if kind in ("mux", "mixed_host") else 2
        arr = [v for _ in range(nin) for v in keyset.encrypt(rng.integers(0, 2, B), rng)]
        h = list(zip(["ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b"], arr))
    elif kind in ("woks", "bootstrap"):
        h = list(zip(["x_a", "x_b"], lwe()))
    elif kind == "keyswitch":
        h = [("u_a", _rand32(rng, (B, N))), ("u_b", _rand32(rng, B))]
    elif kind in ("lut_woks", "lut_boot", "many_woks", "many_boot"):
        h = [("tv", _rand32(rng, (2, N))), ("lut_index", rng.integers(0, 2, B).astype(np.int32))] + \
            list(zip(["x_a", "x_b"], lwe()))
    elif kind == "full_add":
        h = list(zip(["a_a", "a_b"], lwe())) + list(zip(["b_a", "b_b"], lwe()))
        if P["third"]:
            h += list(zip(["c_a", "c_b"], lwe()))
    elif kind in ("acc_woks", "acc_boot"):
        x = keyset.encrypt_digits(rng.integers(0, 4, B), 4, rng)
        h = [("acc", _rand32(rng, (P["n_acc"], 2, N))), ("acc_index", rng.integers(0, P["n_acc"], B).astype(np.int32)),
             ("x_a", x[0]), ("x_b", x[1])]
    elif kind == "select":
        p = P["p"]
        y = keyset.encrypt_digits(rng.integers(0, p, B), p, rng)
        h = [("cand_a", _rand32(rng, (p, B, n_lwe))), ("cand_b", _rand32(rng, (p, B))), ("y_a", y[0]), ("y_b", y[1])]
    elif kind.startswith("lookup"):
        h = [("sel", rng.integers(0, COUNT, (B, P["d"])).astype(np.int32)), ("tab", _rand32(rng, (2, P["n_poly"], 1, N))),
             ("tab_index", rng.integers(0, 2, B).astype(np.int32))]
    elif kind == "cmux":
        h = [("sel", rng.integers(0, COUNT, B).astype(np.int32)), ("d1", _rand32(rng, (B, 2, N)))]
        if P["d0"]:
            h.append(("d0", _rand32(rng, (B, 2, N))))
    elif kind in ("dfa", "dfa_woks"):
        h = [("sel", rng.integers(0, COUNT, (B, P["len"])).astype(np.int32)), ("fin", _rand32(rng, (2, 5, 1, N))),
             ("fin_index", rng.integers(0, 2, B).astype(np.int32))]
    elif kind == "pack":
        h = [("in_a", _rand32(rng, (B, P["P"], n_lwe))), ("in_b", _rand32(rng, (B, P["P"]))),
             ("pos", rng.choice(N, P["P"], replace=False).astype(np.int32))]
    elif kind == "box_fill":
        h = [("tlwe", _rand32(rng, (B, 2, N)))]
    elif kind in ("circuit", "select_circuit"):
        n_in = len(circuits[kind][1])
        h = [("enc_a", _rand32(rng, (n_in, B, n_lwe))), ("enc_b", _rand32(rng, (n_in, B)))]
    else:
        raise KeyError(kind)
    drop = CHAIN_IN[kind] if chained else ()
    return [(k, v) for k, v in h if k not in drop]


def out_shapes(kind, B, P, circuits):
    n_out = P.get("n_out", 1)
    if kind in ("gate", "gate_host", "mux", "mixed_host", "bootstrap", "keyswitch", "lut_boot", "acc_boot", "select"):
        return [("res_a", (B, n_lwe)), ("res_b", (B,))]
    if kind in ("woks", "lut_woks", "acc_woks"):
        return [("u_a", (B, N)), ("u_b", (B,))]
    if kind in ("many_woks", "lookup_woks", "lookup_tree_woks", "dfa_woks"):
        return [("u_a", (n_out, B, N)), ("u_b", (n_out, B))]
    if kind in ("many_boot", "lookup", "lookup_tree", "dfa"):
        return [("res_a", (n_out, B, n_lwe)), ("res_b", (n_out, B))]
    if kind == "full_add":
        return [("res_a", (2, B, n_lwe)), ("res_b", (2, B))]
    if kind in ("cmux", "pack", "box_fill"):
        return [("out", (B, 2, N))]
    n_w = circuits[kind][0].info()["wires"]
    return [("wires_a", (n_w, B, n_lwe)), ("wires_b", (n_w, B))]


def mixed_gates(B, P):
    return ["MUX" if i % P["mux_every"] == 0 else GATES2[i % len(GATES2)] for i in range(B)]


def rotations(kind, B, P, circuits):
    """fp64-path blind rotations of the call (what guard threshold 0 recomputes)"""
    if kind == "mux":
        return 2 * B
    if kind == "mixed_host":
        return B + sum(g == "MUX" for g in mixed_gates(B, P))
    if kind in ("circuit", "select_circuit"):
        return circuits[kind][0].info()["bootstraps"] * B
    if kind in ("keyswitch", "cmux", "pack", "box_fill") or kind.startswith("lookup") or kind.startswith("dfa"):
        return 0
    return B


def oracle(kind, B, P, h, E):
    """h: {name: host array} of every input (chained ones: the producer's oracle output) ->
    {output name: expected words}; E: okey, tok (the pool's oracle key), pack_words, circuits"""
    import acc_oracle as AO
    import dag_oracle as DGO
    import dfa_oracle as DO
    import fa_oracle as FO
    import lut_oracle as LO
    import many_lut_oracle as MO
    import pack_oracle as PO
    import select_dag_oracle as SO
    import tfhe_amd as T
    import tgsw_oracle as TO
    okey, tok = E["okey"], E["tok"]
    pair = lambda names, r: dict(zip(names, r))
    if kind in ("gate", "gate_host"):
        return pair(("res_a", "res_b"), okey.gate_batch(P["gate"], h["ca_a"], h["ca_b"], h["cb_a"], h["cb_b"]))
    if kind == "mux":
        return pair(("res_a", "res_b"), okey.gate_batch("MUX", *[h[k] for k in ("ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b")]))
    if kind == "mixed_host":
        r_a, r_b = np.zeros((B, n_lwe), np.int32), np.zeros(B, np.int32)
        gates = np.array(mixed_gates(B, P))
        for g in sorted(set(gates)):
            at = np.flatnonzero(gates == g)
            names = ("ca_a", "ca_b", "cb_a", "cb_b") + (("cc_a", "cc_b") if g == "MUX" else ())
            r_a[at], r_b[at] = okey.gate_batch(str(g), *[h[k][at] for k in names])
        return {"res_a": r_a, "res_b": r_b}
    if kind == "woks":
        return pair(("u_a", "u_b"), okey.woks_batch(T.MU, h["x_a"], h["x_b"]))
    if kind == "bootstrap":
        return pair(("res_a", "res_b"), okey.keyswitch_batch(*okey.woks_batch(T.MU, h["x_a"], h["x_b"])))
    if kind == "keyswitch":
        return pair(("res_a", "res_b"), okey.keyswitch_batch(h["u_a"], h["u_b"]))
    if kind in ("lut_woks", "lut_boot"):
        w = LO.woks_batch(okey, h["tv"], h["x_a"], h["x_b"], h["lut_index"])
        return pair(("u_a", "u_b"), w) if kind == "lut_woks" else \
            pair(("res_a", "res_b"), okey.keyswitch_batch(*w, nthreads=LO.THREADS))
    if kind in ("many_woks", "many_boot"):
        w = MO.woks_batch(okey, h["tv"], h["x_a"], h["x_b"], P["log_nu"], P["n_out"], h["lut_index"])
        return pair(("u_a", "u_b"), w) if kind == "many_woks" else pair(("res_a", "res_b"), MO.keyswitch(okey, w))
    if kind == "full_add":
        third = (h["c_a"], h["c_b"]) if P["third"] else None
        return pair(("res_a", "res_b"), FO.cell(okey, FO.H, FO.G, (h["a_a"], h["a_b"]), (h["b_a"], h["b_b"]), third))
    if kind in ("acc_woks", "acc_boot"):
        w = AO.woks_batch(okey, h["acc"], h["x_a"], h["x_b"], h["acc_index"])
        return pair(("u_a", "u_b"), w) if kind == "acc_woks" else \
            pair(("res_a", "res_b"), okey.keyswitch_batch(*w, nthreads=AO.THREADS))
    if kind == "select":
        return pair(("res_a", "res_b"), AO.select(okey, E["pack_words"], h["cand_a"], h["cand_b"], 0, 1, h["y_a"], h["y_b"]))
    if kind.startswith("lookup"):
        w = TO.lookup_woks(tok, h["sel"], h["tab"], h["tab_index"], P["log_stride"], P["n_out"])
        return pair(("u_a", "u_b"), w) if kind.endswith("woks") else pair(("res_a", "res_b"), MO.keyswitch(tok, w))
    if kind == "cmux":
        return {"out": np.stack([TO.cmux(tok, int(h["sel"][w]), h["d1"][w], h["d0"][w] if P["d0"] else None)
                                 for w in range(B)])}
    if kind in ("dfa", "dfa_woks"):
        nxt, start = automaton()
        fn = DO.run_woks if kind == "dfa_woks" else DO.run
        return pair(("u_a", "u_b") if kind == "dfa_woks" else ("res_a", "res_b"),
                    fn(tok, nxt, start, h["sel"], h["fin"], h["fin_index"], P["n_out"]))
    if kind == "pack":
        fn = PO.pack_inputs if P["P"] == 1 else PO.pack_rows
        return {"out": fn(E["pack_words"], h["in_a"], h["in_b"], h["pos"])}
    if kind == "box_fill":
        return {"out": AO.box_fill(h["tlwe"], P["log_w"])}
    C, ins = E["circuits"][kind]
    enc = {w: (h["enc_a"][k], h["enc_b"][k]) for k, w in enumerate(ins)}
    W = DGO.eval_circuit(C, okey, enc, B) if kind == "circuit" else \
        SO.eval_circuit(C, okey, enc, B, pack_key=E["pack_words"])
    n_w = C.info()["wires"]
    return {"wires_a": np.stack([W[w][0] for w in range(n_w)]), "wires_b": np.stack([W[w][1] for w in range(n_w)])}


def invoke(kind, B, P, ctx, v, objs, stream):
    """the call under test on the views v (device tensors; numpy arrays for the host forms)"""
    import fa_oracle as FO
    import tfhe_amd as T
    if kind == "gate":
        ctx.gate_dev(P["gate"], v["res_a"], v["res_b"], v["ca_a"], v["ca_b"], v["cb_a"], v["cb_b"], stream=stream)
    elif kind == "mux":
        ctx.gate_dev("MUX", v["res_a"], v["res_b"], *[v[k] for k in ("ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b")],
                     stream=stream)
    elif kind == "gate_host":
        rc = T.lib.tfhe_amd_gate_batch_host(ctx.h, T.GATES[P["gate"]], B, T._p(v["res_a"]), T._p(v["res_b"]),
                                            *[T._p(v[k]) for k in ("ca_a", "ca_b", "cb_a", "cb_b")], None, None)
        assert rc == 0, ("gate_batch_host", rc)
    elif kind == "mixed_host":
        import ctypes
        g = np.array([T.GATES[x] for x in mixed_gates(B, P)], dtype=np.int32)
        rc = T.lib.tfhe_amd_gate_batch_mixed_host(ctx.h, B, g.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                  T._p(v["res_a"]), T._p(v["res_b"]),
                                                  *[T._p(v[k]) for k in ("ca_a", "ca_b", "cb_a", "cb_b", "cc_a", "cc_b")])
        assert rc == 0, ("gate_batch_mixed_host", rc)
    elif kind == "woks":
        ctx.woks_dev(T.MU, v["x_a"], v["x_b"], v["u_a"], v["u_b"], stream=stream)
    elif kind == "bootstrap":
        ctx.bootstrap_dev(T.MU, v["x_a"], v["x_b"], v["res_a"], v["res_b"], stream=stream)
    elif kind == "keyswitch":
        ctx.keyswitch_dev(v["u_a"], v["u_b"], v["res_a"], v["res_b"], stream=stream)
    elif kind == "lut_woks":
        ctx.lut_woks_dev(v["tv"], v["u_a"], v["u_b"], v["x_a"], v["x_b"], v["lut_index"], stream=stream)
    elif kind == "lut_boot":
        ctx.lut_bootstrap_dev(v["tv"], v["res_a"], v["res_b"], v["x_a"], v["x_b"], v["lut_index"], stream=stream)
    elif kind == "many_woks":
        ctx.lut_many_woks_dev(v["tv"], P["log_nu"], P["n_out"], v["u_a"], v["u_b"], v["x_a"], v["x_b"], v["lut_index"],
                              stream=stream)
    elif kind == "many_boot":
        ctx.lut_many_bootstrap_dev(v["tv"], P["log_nu"], P["n_out"], v["res_a"], v["res_b"], v["x_a"], v["x_b"],
                                   v["lut_index"], stream=stream)
    elif kind == "full_add":
        ctx.full_add_dev(FO.H, FO.G, v["res_a"], v["res_b"], (v["a_a"], v["a_b"]), (v["b_a"], v["b_b"]),
                         (v["c_a"], v["c_b"]) if P["third"] else None, stream=stream)
    elif kind == "acc_woks":
        ctx.acc_woks_dev(v["acc"], v["u_a"], v["u_b"], v["x_a"], v["x_b"], v["acc_index"], stream=stream)
    elif kind == "acc_boot":
        ctx.acc_bootstrap_dev(v["acc"], v["res_a"], v["res_b"], v["x_a"], v["x_b"], v["acc_index"], stream=stream)
    elif kind == "select":
        ctx.select_dev(objs["pack"], v["cand_a"], v["cand_b"], v["y_a"], v["y_b"], v["res_a"], v["res_b"], stream=stream)
    elif kind.startswith("lookup"):
        woks = kind.endswith("woks")
        ctx.tgsw_lookup_dev(objs["tgsw"], v["sel"], v["tab"], v["u_a" if woks else "res_a"], v["u_b" if woks else "res_b"],
                            v["tab_index"], P["log_stride"], P["n_out"], woks, stream=stream)
    elif kind == "cmux":
        ctx.tgsw_cmux_dev(objs["tgsw"], v["sel"], v["d1"], v["d0"] if P["d0"] else None, v["out"], stream=stream)
    elif kind in ("dfa", "dfa_woks"):
        woks = kind == "dfa_woks"
        ctx.dfa_run_dev(objs["tgsw"], objs["dfa"], v["sel"], v["fin"], v["u_a" if woks else "res_a"],
                        v["u_b" if woks else "res_b"], v["fin_index"], P["n_out"], woks, stream=stream)
    elif kind == "pack":
        ctx.pack_dev(objs["pack"], v["in_a"], v["in_b"], v["out"], v["pos"], stream=stream)
    elif kind == "box_fill":
        ctx.box_fill_dev(v["tlwe"], v["out"], P["log_w"], stream=stream)
    elif kind == "circuit":
        objs["circuit"][0].run_dev(ctx, B, v["wires_a"], v["wires_b"], stream)
    elif kind == "select_circuit":
        objs["select_circuit"][0].run_dev(ctx, B, v["wires_a"], v["wires_b"], stream, pack_key=objs["pack"])
    else:
        raise KeyError(kind)


# ---------------------------------------------------------------- the checker

_session = {}


def session(ctx, keyset, okey):
    """what every program of a test session shares: the pool and packing key words, the pool's oracle
    key, and the objects of the solo runs (the programs import their own)"""
    import tgsw_oracle as TO
    if _session.get("ctx") is not ctx:
        _session.clear()
        pack_words = _rand32(np.random.default_rng(3803), (n_lwe, 6, 2, N))
        pool = _rand32(np.random.default_rng(2420), (COUNT, 4, 2, N))
        circuits = {"circuit": small_circuit(), "select_circuit": select_circuit()}
        _session.update(ctx=ctx, keyset=keyset, okey=okey, pack_words=pack_words, pool=pool,
                        tok=TO.key(pool, keyset.ksk), circuits=circuits,
                        solo=_import_objects(ctx, pack_words, pool, circuits), oracle_cache={})
    return _session


def _import_objects(ctx, pack_words, pool, circuits=None):
    nxt, start = automaton()
    return {"pack": ctx.pack_key_import(pack_words), "tgsw": ctx.tgsw_import(pool), "dfa": ctx.dfa_create(nxt, start, 8),
            "circuit": circuits["circuit"] if circuits else small_circuit(),
            "select_circuit": circuits["select_circuit"] if circuits else select_circuit()}


def _tile(a, B):
    return np.ascontiguousarray(a[np.arange(B) % a.shape[0]])


def _switches(kernel, guard0):
    import tfhe_amd as T
    T.select_kernel(kernel)
    T.set_guard_threshold(0.0 if guard0 else 0.125)


def expected_outputs(program, S, cus):
    """per call step: (host inputs [(name, array)] without the chained slots, {output: expected}); the
    threshold steps are computed on their 5 distinct rows and tiled"""
    key = (program["seed"], cus)
    if key in S["oracle_cache"]:
        return S["oracle_cache"][key]
    E = dict(okey=S["okey"], tok=S["tok"], pack_words=S["pack_words"], circuits=S["circuits"])
    hosts, wants = {}, {}
    for i, s in enumerate(program["steps"]):
        if s["step"] != "call":
            continue
        kind, P = s["kind"], s["P"]
        B = resolve_B(s["B"], cus)
        Bd = min(B, 5) if isinstance(s["B"], str) else B
        assert Bd == B or kind in ROWWISE, (kind, s["B"])
        rng = np.random.default_rng([program["seed"], i])
        small = fresh_inputs(kind, Bd, P, rng, S["keyset"], S["circuits"], s["chain"] is not None)
        full = dict(small)
        if s["chain"] is not None:
            src = program["steps"][s["chain"][0]]
            for slot, name in zip(CHAIN_IN[kind], CHAIN_OUT[_K[src["kind"]]["cout"]]):
                full[slot] = wants[s["chain"][0]][name]
        want = oracle(kind, Bd, P, full, E)
        hosts[i] = [(k, _tile(a, B) if Bd != B else a) for k, a in small]
        wants[i] = {k: (_tile(a, B) if Bd != B else np.asarray(a)) for k, a in want.items()}
    S["oracle_cache"][key] = (hosts, wants)
    return hosts, wants


def run_program(program, ctx, keyset, okey, skew=False):
    """Enqueue the program as written — only its own state steps synchronise — then one
    torch.cuda.synchronize(), then assert, in this order:
      (Q1) after each call last_kernels() named what the same call named alone under the same switches;
      (Q2) every output word of every call equals the oracle's (a chained input is the oracle's
           output of its producer), no tolerance, no step left out;
      (Q3) every band of every step's arena is intact (the poison alternates const / index from step
           to step) and every input that is not a chained output is unchanged;
      (Q4) per context, guard_stats' recomputed count equals the fp64-path rotations enqueued while the
           threshold was 0 (0 rotations count under select_kernel(4): the exact kernel needs no guard).
    skew: every view 1 .. 3 words behind its 512-byte multiple, but the key switch's u_a.
    -> {"oracle_s", "solo_s", "program_s"}"""
    import torch
    import dev_arena as DA
    import tfhe_amd as T
    what = f"seq fuzz seed {program['seed']}, start kernel {program['start_kernel']}" + (", skewed" if skew else "")
    steps = program["steps"]
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    S = session(ctx, keyset, okey)
    t0 = time.perf_counter()
    hosts, wants = expected_outputs(program, S, cus)
    t1 = time.perf_counter()
    calls = [i for i, s in enumerate(steps) if s["step"] == "call"]
    ks_feed = {steps[i]["chain"][0] for i in calls if steps[i]["kind"] == "keyswitch" and steps[i]["chain"]}

    def arena_of(i, poison, solo):
        s = steps[i]
        B = resolve_B(s["B"], cus)
        inps = list(hosts[i])
        if solo and s["chain"] is not None:                 # stand-ins of the right shape: the names do not depend on data
            rng = np.random.default_rng([program["seed"], i, 1])
            inps += [(slot, _rand32(rng, shp)) for slot, shp in zip(CHAIN_IN[s["kind"]], chain_shapes(s["kind"], B, s["P"]))]
        aligned = ("u_a",) if s["kind"] == "keyswitch" or i in ks_feed else ()
        return DA.Arena.of("cpu" if _K[s["kind"]]["host"] else "cuda", poison, out_shapes(s["kind"], B, s["P"], S["circuits"]),
                           inps, skew=skew, aligned=aligned)

    def views_for_call(i, arena, v, objs):
        s = steps[i]
        if _K[s["kind"]]["host"]:
            return {k: arena.numpy(t) for k, t in v.items()}
        if s["kind"] in ("circuit", "select_circuit"):
            for k, w in enumerate(objs[s["kind"]][1]):
                v["wires_a"][w].copy_(v["enc_a"][k])
                v["wires_b"][w].copy_(v["enc_b"][k])
        return v

    def switch_states():
        """(kernel, guard0) at each step, from the program alone"""
        kernel, guard0, out = program["start_kernel"], False, []
        for s in steps:
            if s["step"] == "state":
                if s["op"] == "kernel_flip":
                    kernel = 4 - program["start_kernel"]
                elif s["op"] == "kernel_back":
                    kernel = program["start_kernel"]
                elif s["op"] in ("guard_flip", "guard_back"):
                    guard0 = s["op"] == "guard_flip"
            out.append((kernel, guard0))
        return out

    states = switch_states()
    ctx_b, objs, tmp_streams = None, None, []
    try:
        # ---- every call alone, on the session context and the session's own objects
        solo_names = {}
        for i in calls:
            s = steps[i]
            _switches(*states[i])
            arena, v = arena_of(i, "const", True)
            v = views_for_call(i, arena, v, S["solo"])
            torch.cuda.synchronize()
            invoke(s["kind"], resolve_B(s["B"], cus), s["P"], ctx, v, S["solo"], None)
            solo_names[i] = ctx.last_kernels()
            ctx.sync()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        # ---- the program: its own context B and objects, every arena before the first call
        _switches(program["start_kernel"], False)
        ctx_b = T.Context.replica_of(ctx, ctx.device)
        C = {"A": ctx, "B": ctx_b}
        objs = _import_objects(ctx, S["pack_words"], S["pool"])
        streams = {}
        for name, c in C.items():
            streams[("own", name)] = torch.cuda.ExternalStream(c.stream)
        for k in (1, 2, 3):
            streams[("t", k)] = torch.cuda.Stream()
        arenas, views = {}, {}
        for n, i in enumerate(calls):
            arenas[i], v = arena_of(i, DA.POISONS[n % 2], False)
            views[i] = views_for_call(i, arenas[i], v, objs)
        for i in calls:                                     # the chained slots: the producer's output views
            s = steps[i]
            if s["chain"] is not None:
                src = s["chain"][0]
                for slot, name in zip(CHAIN_IN[s["kind"]], CHAIN_OUT[_K[steps[src]["kind"]]["cout"]]):
                    views[i][slot] = views[src][name]
        cross = {}                                          # producer step -> event, where another stream reads it
        for i in calls:
            s = steps[i]
            if s["chain"] is not None and stream_key(steps[s["chain"][0]]) != stream_key(s):
                cross[s["chain"][0]] = None
        redo_want, redo_got = {"A": 0, "B": 0}, {"A": 0, "B": 0}
        names_got = {}
        ctx.guard_stats(reset=True)
        ctx_b.guard_stats(reset=True)
        torch.cuda.synchronize()
        for i, s in enumerate(steps):
            if s["step"] == "state":
                op = s["op"]
                if op == "reserve":
                    C[s["ctx"]].reserve(resolve_B(s["B"], cus))
                elif op in ("guard_flip", "guard_back", "kernel_flip", "kernel_back"):
                    _switches(*states[i])
                elif op == "guard_stats":
                    redo_got[s["ctx"]] += C[s["ctx"]].guard_stats(reset=True)[1]
                elif op == "sync":
                    C[s["ctx"]].sync()
                elif op == "ctx_cycle":
                    T.Context.replica_of(ctx, ctx.device).close()
                elif s["obj"] == "circuit":
                    objs["circuit"][0].close()
                    objs["circuit"] = small_circuit()
                else:
                    objs[s["obj"]].close()
                    nxt, start = automaton()
                    objs[s["obj"]] = ctx.pack_key_import(S["pack_words"]) if s["obj"] == "pack" else \
                        ctx.tgsw_import(S["pool"]) if s["obj"] == "tgsw" else ctx.dfa_create(nxt, start, 8)
                continue
            kind, sk = s["kind"], stream_key(s)
            B = resolve_B(s["B"], cus)
            st = streams[sk]
            if s["chain"] is not None and cross.get(s["chain"][0]) is not None and stream_key(steps[s["chain"][0]]) != sk:
                st.wait_event(cross[s["chain"][0]])         # the caller's duty, not the library's
            invoke(kind, B, s["P"], C[s["ctx"]], views[i], objs, None if s["stream"] == 0 else st.cuda_stream)
            names_got[i] = C[s["ctx"]].last_kernels()
            if i in cross:
                cross[i] = torch.cuda.Event()
                cross[i].record(st)
            if states[i][1] and states[i][0] != 4:
                redo_want[s["ctx"]] += rotations(kind, B, s["P"], S["circuits"])
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for name, c in C.items():
            redo_got[name] += c.guard_stats(reset=True)[1]
        # ---- the verdict
        for i in calls:
            assert names_got[i] == solo_names[i], (f"{what}: Q1 step {i} ({steps[i]['kind']}) named {names_got[i]}, alone "
                                                   f"{solo_names[i]}\n{summary(program)}")
        for i in calls:
            for name, want in wants[i].items():
                got = views[i][name] if _K[steps[i]["kind"]]["host"] else views[i][name].cpu().numpy()
                assert got.shape == want.shape, (what, i, name, got.shape, want.shape)
                bad = np.argwhere(got != want)
                assert bad.shape[0] == 0, (f"{what}: Q2 step {i} ({steps[i]['kind']}) {name} != oracle at {bad.shape[0]} "
                                           f"words, the first at {bad[0].tolist()}\n{summary(program)}")
        for i in calls:
            try:
                arenas[i].check()
            except AssertionError as e:
                raise AssertionError(f"{what}: Q3 step {i} ({steps[i]['kind']}, {arenas[i].kind} poison): {e}\n"
                                     f"{summary(program)}") from None
        assert redo_got == redo_want, f"{what}: Q4 recomputed {redo_got}, enqueued at threshold 0 {redo_want}\n{summary(program)}"
        return {"oracle_s": t1 - t0, "solo_s": t2 - t1, "program_s": t3 - t2}
    finally:
        _switches(0, False)
        torch.cuda.synchronize()
        if objs is not None:
            for k in ("pack", "tgsw", "dfa"):
                objs[k].close()
            objs["circuit"][0].close()
            objs["select_circuit"][0].close()
        if ctx_b is not None:
            ctx_b.close()
