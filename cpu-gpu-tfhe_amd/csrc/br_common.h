// br_common.h — what the two blind-rotation generations (blind_rotate_v6.hip, blind_rotate_v4.hip)
// share: the device-side input decoding and gate prologue, and the launchers' dispatch from a
// launch's runtime choices to a kernel instantiation and its trace name.
#pragma once
#include <cstdio>
#include <initializer_list>
#include <type_traits>
#include "engine.h"
#include "modarith.h"

namespace tfhe_amd {

// ------------------------------------------------------------------ device side

// The linear combination x = (0, c) + sa X + sb Y + sc Z that feeds one blind rotation (gate
// prologues boot-gates.cu:98-448; a circuit row adds a third input for MAJ / XOR3).
struct RowTerms {
    int32_t c, sa, sb, sc;
    const int32_t *xa, *xb, *ya, *yb, *za, *zb;   // a rows (kn) and b words; y / z may be null
};

// ciphertext idx of a gate-batch input.  The third input (engine.h BrInput) is read only by the
// LUT and many-LUT instantiations; the constant kernels keep two inputs.
// (in by value, here and in lut_args: the kernels pick one of two kernel arguments by half, and
// through a reference to that choice the compiler loads both records whole and selects field by
// field, which in the v4 kernels spills 40 - 90 more scalar registers to lanes; the copy of the
// chosen record is read through one selected pointer, as the kernels' own code was)
template <bool LUT>
__device__ __forceinline__ void row_terms(RowTerms &t, const BrInput in, int idx) {
    t.c = in.c; t.sa = in.sa; t.sb = in.sb; t.sc = 0;
    t.xa = in.x_a + (size_t)idx * kn; t.xb = in.x_b + idx;
    t.ya = in.sb ? in.y_a + (size_t)idx * kn : nullptr; t.yb = in.sb ? in.y_b + idx : nullptr;
    t.za = nullptr; t.zb = nullptr;
    if constexpr (LUT) {
        t.sc = in.sc;
        t.za = in.sc ? in.z_a + (size_t)idx * kn : nullptr; t.zb = in.sc ? in.z_b + idx : nullptr;
    }
}
// instance k of a circuit row over the wires [W][B] (wire index -1: absent)
__device__ __forceinline__ void row_terms(RowTerms &t, const CircRow &row, const int32_t *wa, const int32_t *wb, int B,
                                          int k) {
    auto wire = [&](int w, const int32_t *&pa, const int32_t *&pb) {
        if (w < 0) { pa = nullptr; pb = nullptr; return; }
        const size_t ws = (size_t)w * B + k;
        pa = wa + ws * kn;
        pb = wb + ws;
    };
    t.c = row.c; t.sa = row.sa; t.sb = row.sb; t.sc = row.sc;
    wire(row.x, t.xa, t.xb);
    wire(row.y, t.ya, t.yb);
    wire(row.z, t.za, t.zb);
}

// Mixed-key rows (engine.h RingKeys / RingWires).  The entry index of a ring wire, clamped into [0, n).
__device__ __forceinline__ int ring_entry(int w, int n) {
    int i = w >> 2;
    i = i < n ? i : n - 1;
    return i > 0 ? i : 0;
}
__device__ __forceinline__ void row_terms(RowTerms &t, const CircRow &row, const RingWires &wr) {
    auto wire = [&](int w, const int32_t *&pa, const int32_t *&pb) {
        const int seg = w & 3;
        // (selects, not an indexed array of the kernel argument: that would go through scratch)
        const int32_t *a = seg == 0 ? wr.a0 : seg == 1 ? wr.a1 : seg == 2 ? wr.a2 : nullptr;
        const int32_t *b = seg == 0 ? wr.b0 : seg == 1 ? wr.b1 : seg == 2 ? wr.b2 : nullptr;
        if (w < 0 || !a || !b || wr.n <= 0) { pa = nullptr; pb = nullptr; return; }
        const size_t i = (size_t)ring_entry(w, wr.n);
        pa = a + i * kn;
        pb = b + i;
    };
    t.c = row.c; t.sa = row.sa; t.sb = row.sb; t.sc = row.sc;
    wire(row.x, t.xa, t.xb);
    wire(row.y, t.ya, t.yb);
    wire(row.z, t.za, t.zb);
}
// The key of row r: its slot from device memory, clamped into [0, n_keys) before any address is
// formed, then the slot's pointer made wave-uniform half by half (fft_wave.h uni), so that what the
// body builds from it (v6: the key's buffer resource) stays in scalar registers.
template <class T>
__device__ __forceinline__ const T *ring_key(const RingKeys &kr, long r) {
    int k = kr.row_key[r];
    k = k < kr.n_keys ? k : kr.n_keys - 1;
    k = k > 0 ? k : 0;
    const unsigned long long bits = (unsigned long long)reinterpret_cast<uintptr_t>(kr.bk[k]);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)bits);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(bits >> 32));
    return reinterpret_cast<const T *>((uintptr_t)(((unsigned long long)hi << 32) | lo));
}

// The key of instance k of a mixed-key circuit level (engine.h RingInstKeys): the same rule, the slot
// read from inst_key[k].
template <class T>
__device__ __forceinline__ const T *ring_inst_key(const RingInstKeys &kr, int k) {
    return ring_key<T>(RingKeys{kr.bk, kr.inst_key, kr.n_keys}, k);
}

// The test vector and the extra outputs of one ciphertext.  Compile-time null / default for the
// constant instantiations, which form no table address.
struct LutArgs {
    const int32_t *tv = nullptr;
    ManyOut mo;
};
// gate batch: ciphertext idx of its half, gct of the launch.  Many-LUT launches have one half:
// output f of ciphertext gct is u sample f B + gct.
template <bool LUT, bool MANY>
__device__ __forceinline__ LutArgs lut_args(const BrInput in, int B, int idx, int gct, int32_t *u_a, int32_t *u_b) {
    LutArgs l;
    if constexpr (LUT) l.tv = lut_table(in.tv, in.lut_index, in.n_lut, idx);
    if constexpr (MANY)
        l.mo = ManyOut{in.log_nu, in.n_out, u_a + ((size_t)B + gct) * kN, u_b + (size_t)B + gct, (size_t)B};
    return l;
}
// circuit row `row` (the record at `rec`), instance k: a LUT row's test vector lies row.lut words
// after its own record; outputs f >= 1 of a many-LUT row go to the u rows row.urow + f - 1, every
// other row of a many-LUT launch is th = 0, n_out = 1 (engine.h CircRow)
template <bool LUT, bool MANY>
__device__ __forceinline__ LutArgs lut_args(const CircRow *rec, const CircRow &row, int B, int k, int32_t *u_a,
                                            int32_t *u_b) {
    LutArgs l;
    if constexpr (LUT) l.tv = row.lut ? reinterpret_cast<const int32_t *>(rec) + row.lut : nullptr;
    if constexpr (MANY) {
        const size_t s1 = (size_t)row.urow * B + k;
        l.mo = ManyOut{row.many & 7, row.many ? (row.many >> 8) & 31 : 1, u_a + s1 * kN, u_b + s1, (size_t)B};
    }
    return l;
}

// The accumulator sample of ciphertext idx of an encrypted-accumulator launch (engine.h BrInput.acc):
// the index comes from device memory unchecked by the host, so it is clamped into [0, n_acc) before
// it forms an address.  Compile-time null for every other instantiation.
template <bool TLWE>
__device__ __forceinline__ const int32_t *acc_sample(const BrInput in, int idx) {
    if constexpr (TLWE) {
        int t = in.acc_index ? in.acc_index[idx] : in.n_acc == 1 ? 0 : idx;
        t = t < in.n_acc ? t : in.n_acc - 1;
        t = t > 0 ? t : 0;
        return in.acc + (size_t)t * 2 * kN;
    }
    return nullptr;
}

// gate prologue + modulus switching (lwe-bootstrapping-functions-fft.cu:1851-1858) by the THREADS
// threads of one ciphertext: bara[0 .. kn) and barb, rotation amounts < 2N (MANY: multiples of 2^th)
template <bool MANY, int THREADS, typename T>
__device__ __forceinline__ void br_prologue(const RowTerms &t, int th, int tid, T *bara, int &barb) {
    for (int i = tid; i < kn; i += THREADS) {
        uint32_t x = t.xa ? (uint32_t)t.sa * (uint32_t)t.xa[i] : 0u;
        if (t.ya) x += (uint32_t)t.sb * (uint32_t)t.ya[i];
        if (t.za) x += (uint32_t)t.sc * (uint32_t)t.za[i];
        bara[i] = (T)(MANY ? modswitch_nu(x, th) : modswitch_2N(x));
    }
    if (tid == 0) {
        uint32_t xb = (uint32_t)t.c + (t.xb ? (uint32_t)t.sa * (uint32_t)t.xb[0] : 0u);
        if (t.yb) xb += (uint32_t)t.sb * (uint32_t)t.yb[0];
        if (t.zb) xb += (uint32_t)t.sc * (uint32_t)t.zb[0];
        barb = MANY ? modswitch_nu(xb, th) : modswitch_2N(xb);
    }
}

// ------------------------------------------------------------------ launchers

namespace {   // host helpers of the two launcher files, not library symbols

// A launcher's runtime choices as compile-time constants: f is called with the mode, or the flag,
// as a std::integral_constant, and names the kernel instantiation from it.
template <class F>
void with_mode(BrMode mode, F &&f) {
    switch (mode) {
    case BrMode::Tlwe: return f(std::integral_constant<BrMode, BrMode::Tlwe>{});
    case BrMode::Many: return f(std::integral_constant<BrMode, BrMode::Many>{});
    case BrMode::Lut: return f(std::integral_constant<BrMode, BrMode::Lut>{});
    default: return f(std::integral_constant<BrMode, BrMode::Const>{});
    }
}
template <class F>
void with_flag(bool flag, F &&f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}
constexpr bool mode_lut(BrMode m) { return m == BrMode::Lut || m == BrMode::Many; }
constexpr bool mode_many(BrMode m) { return m == BrMode::Many; }
constexpr bool mode_tlwe(BrMode m) { return m == BrMode::Tlwe; }

// The trace name of a launch (engine.h trace_kernel), from the same choices: the kernel's name,
// then in parentheses the mode (lut / lut-many / tlwe; nothing for the constant form) and the form's
// non-null parts, joined by '+'; the bare name when there is nothing to say.
struct KernelLabel {
    char s[96];
    KernelLabel(const char *name, BrMode mode, std::initializer_list<const char *> form) {
        size_t n = (size_t)snprintf(s, sizeof s, "%s", name);
        const char *sep = "(";
        auto add = [&](const char *part) {
            if (!part || n >= sizeof s) return;
            n += (size_t)snprintf(s + n, sizeof s - n, "%s%s", sep, part);
            sep = "+";
        };
        add(mode == BrMode::Many ? "lut-many" : mode == BrMode::Lut ? "lut" : mode == BrMode::Tlwe ? "tlwe" : nullptr);
        for (const char *part : form) add(part);
        if (*sep == '+' && n < sizeof s) snprintf(s + n, sizeof s - n, ")");
    }
};

}  // namespace

}  // namespace tfhe_amd
